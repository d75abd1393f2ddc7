"""CPU side of tests/test_gpu_fv_wide_stretched_edges.py (NumPy only; tests/fv_wide_stretched_probe.py): what the GPU file
relies on is asserted here, on the restatement alone.

The zero-mode rule of the restated eigen-decompositions reaches 1024 cells and still refuses a table with two zero modes; the
work-vector table of the chip chain is pinned against the device sources; the seeded states have both signs among the inner
fluxes of either direction and wall faces of exactly 0.0; for every capped case the restatement caps every solve, moves by at
most 1e-10 when its linear_solver_tol goes from 1e-12 to 1e-13, and every lost-share mutant named for the case moves a field
by at least 1e-7 (the GPU tolerance, 1e-9, lies between); the copied loops with every sum whole are the originals bit for bit;
the comparison function of the capped GPU tests fails on every mutant held against the unmutated restatement; the threshold
cases tell a lost share in either norm of the stop test; the NaN case goes non-finite inside the first chunk.  Each test
prints its figures (profiles/fv_wide_stretched_edges.md)."""
import re
import sys
import time
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import fv_krylov_probe as K  # noqa: E402
import fv_separable_numpy as SN  # noqa: E402
import fv_stretched_numpy as GN  # noqa: E402
import fv_stretched_probe as S  # noqa: E402
import fv_wide_stretched_probe as P  # noqa: E402
from conftest import PKG  # noqa: E402

CSRC = PKG / "csrc"


def _finite(r):
    return all(np.all(np.isfinite(r[k])) for k in K.FIELDS) and np.all(np.isfinite(r["rows"]))


# ---------------------------------------------------------------------------------------------- 0. the zero-mode rule
def _axis(n, L, beta):
    return GN.axis_tables(GN.tanh_vertices(n, L, beta))[1:]


def _raw_eig(m, w):
    """lam of the Neumann stiffness with the inner-face weights ``w`` against diag(m), no rule applied."""
    from scipy.linalg import eigh
    n = m.size
    Kmat = np.zeros((n, n))
    i = np.arange(n - 1)
    Kmat[i, i] += w
    Kmat[i + 1, i + 1] += w
    Kmat[i, i + 1] -= w
    Kmat[i + 1, i] -= w
    return eigh(Kmat, np.diag(m), eigvals_only=True)


@pytest.mark.parametrize("beta", [0.0, 1.0, 1.5, 2.5])
def test_every_size_the_ratio_rule_accepted_still_passes(beta):
    """8 ... 560 cells, L 0.5, 1, 2, rho 1 and 2: wherever lam[1] > 1e-6 lam[-1] held, the rule of ``generalised_eig_host``
    (lam[1] > rho (pi / L)^2 / 2) holds too, so ``generalised_eig`` and ``separable_eig`` (with the weights of a square fit)
    construct; the smallest lam[1] / (rho (pi / L)^2) is printed."""
    low, accepted = np.inf, 0
    for n in (8, 9, 13, 24, 37, 50, 77, 131, 256, 264, 300, 420, 560):
        for L in (0.5, 1.0, 2.0):
            h, d, g = _axis(n, L, beta)
            a, _, _ = SN.separable_fit(h, d, h, d)
            af = g[1:n] * a[1:] + (1.0 - g[1:n]) * a[:-1]
            for rho in (1.0, 2.0):
                for m, w, restated in ((h, rho / d[1:n], lambda: GN.generalised_eig(h, d, rho)[0]),
                                       (h * a, rho * af / d[1:n], lambda: SN.separable_eig(h, d, g, a, rho)[0])):
                    lam = _raw_eig(m, w)
                    if abs(lam[0]) < 1e-9 * lam[-1] and lam[1] > 1e-6 * lam[-1]:             # the former rule
                        accepted += 1
                        assert np.allclose(restated(), lam, rtol=1e-9, atol=1e-9 * lam[-1])
                        low = min(low, lam[1] / (rho * (np.pi / L) ** 2))
    print(f"beta {beta}: {accepted} tables accepted by the ratio rule, least lam[1] / (rho (pi / L)^2) {low:.3f}")
    assert accepted >= 2 * 36 and low > 0.5                  # (at least: both kinds of table, every size up to 77 cells)


@pytest.mark.parametrize("Lx", [1.0, 2.0])
@pytest.mark.parametrize("beta", [0.0, 1.5])
def test_the_restatement_constructs_at_1024_cells(Lx, beta):
    t0 = time.perf_counter()
    o = SN.FVSeparableState(1024, 72, 400.0, Lx=Lx, grid_stretch=beta)
    dt = time.perf_counter() - t0
    ref = o.rho * (np.pi / Lx) ** 2
    print(f"1024 x 72, Lx {Lx}, beta {beta}: {dt:.1f} s; lam[1] / (rho (pi / Lx)^2) {o.lamx[1] / ref:.3f} (grid), "
          f"{o.slamx[1] / ref:.3f} (separable fit); lam[1] / lam[-1] {o.lamx[1] / o.lamx[-1]:.1e}, {o.slamx[1] / o.slamx[-1]:.1e}")
    for lam in (o.lamx, o.slamx):
        assert abs(lam[0]) < 1e-9 * lam[-1] and lam[1] > 0.5 * ref
    if beta > 0:
        assert o.lamx[1] < 1e-6 * o.lamx[-1]                 # (the former rule refused this table)


@pytest.mark.parametrize("n", [50, 1024])
def test_a_table_with_two_zero_modes_is_refused(n):
    """An inner face of weight zero (d = inf) cuts the axis in two: two constants, lam[1] = 0 to rounding."""
    h, d, g = _axis(n, 1.0, 1.5)
    a, _, _ = SN.separable_fit(h, d, h, d)
    GN.generalised_eig(h, d)
    SN.separable_eig(h, d, g, a)
    cut = d.copy()
    cut[n // 3] = np.inf
    with pytest.raises(AssertionError, match="one zero mode"):
        GN.generalised_eig(h, cut)
    with pytest.raises(AssertionError, match="one zero mode"):
        SN.separable_eig(h, cut, g, a)


# ---------------------------------------------------------------------------------------------- 1. the layout
def _enum_fvvec():
    text = (CSRC / "ldc_fv_common.inc").read_text()
    body = re.search(r"enum FvVec \{(.*?)\};", text, re.S).group(1)
    names = [w for w in re.sub(r"//[^\n]*", "", body).replace("\n", " ").split(",") if w.strip()]
    return {name.strip(): k for k, name in enumerate(names)}


def _aliases(text, names):
    """``NAME = FV_...`` of a ``constexpr FvVec`` line."""
    out = {}
    for line in text.splitlines():
        if line.startswith("constexpr FvVec "):
            out.update(re.findall(r"(\w+) = (FV_\w+)", line))
    assert set(names) <= set(out), (names, out)
    return {k: out[k] for k in names}


def test_the_probe_reads_the_vectors_the_chip_chain_writes():
    enum = _enum_fvvec()
    assert enum["FV_GPX"] == 0 and enum["FV_NVEC"] == len(enum) - 1 == 32
    pcg = _aliases((CSRC / "ldc_fv_pressure_cells.inc").read_text(), ("PCG_MS", "PCG_R", "PCG_Z", "PCG_P", "PCG_Q"))
    sep = _aliases((CSRC / "ldc_fv_wide_separable.inc").read_text(), ("WSEP_S", "WSEP_SR"))
    index = dict(enum, **{k: enum[v] for k, v in dict(pcg, **sep).items()})
    for name, k in P.INDEX.items():
        assert index[name] == k, (name, index[name], k)
    assert "SEP_S" not in P.INDEX and (P.INDEX["WSEP_S"], P.INDEX["WSEP_SR"]) == (18, 19)
    # the two copies of p and q: the one-CU kernel's SEP_S (15) is the second copy of p here
    assert P.INDEX["PCG_P"] + P.PCG_P_COPIES == P.INDEX["PCG_Q"] == 16 and S.INDEX["SEP_S"] == P.INDEX["PCG_P"] + 1
    want = dict(grad_p=(0, 1), diag=(2, 3, 4, 5, 6), b=(30, 31), u_star=(7,), v_star=(8,), mdot_star=(9,), rhs_p=(23,),
                p_prime=(26,), u_prime=(27,), v_prime=(28,), omega=(29,), sep_s=(18,), sep_sr=(19,), cg_r=(12,))
    assert {k: tuple(P.INDEX[n] for n in v) for k, v in P.VEC.items()} == want
    # mdot* ends where the CG residual begins; what the GEMMs of either pressure solve use as scratch (FV_W1, FV_W2), z, p
    # and q are clear of everything the probe reads
    assert index["PCG_MS"] + P.MS_VECTORS == index["PCG_R"]
    for nx, ny in ((8, 8), (8, 1024), (1024, 1024)):
        assert ny * (nx + 1) + (ny + 1) * nx <= P.MS_VECTORS * nx * ny
    read = {k for v in want.values() for k in v} | {10, 11}
    assert len(read) == sum(len(v) for v in want.values()) + 2
    assert not read & {index["FV_W1"], index["FV_W2"], index["PCG_Z"], 14, 15, 16}


def test_no_vector_of_the_chip_chain_holds_b00():
    """The one key of the one-CU probe that the chip chain cannot show (``NOT_STORED``): cell 0's right-hand side is stored as
    0.0 by the faces phase of every chain, and the first GEMM of the reference solve substitutes b00 from the slot sum."""
    assert P.NOT_STORED == dict(reference=("b00",), laplacian=(), separable=())
    assert "rhs = c == 0 ? 0.0 :" in (CSRC / "ldc_fv_stretched_cells.inc").read_text()
    assert "if (FIRST && k == 0 && bc == 0) b = b00;" in (CSRC / "ldc_fv_cells.inc").read_text()
    wide = (CSRC / "ldc_fv_wide.hip").read_text()
    assert "b00 = -csum[0];" in wide and "fv_wide_gemm<true, false>" in wide


def test_the_chains_are_the_three_chip_settings():
    assert P.CHAINS == ("reference", "laplacian", "separable")
    for chain, mode in P.CHIP_MODE.items():
        assert (mode["grid"], mode["mapping"], mode["chip_grid"]) == ("tanh", "chip", "tables")
        assert mode["pressure_equation"] == ("reference" if chain == "reference" else "consistent")
        assert mode.get("chip_preconditioner") == ("separable" if chain == "separable" else None)
    m, _ = P.phase_case("37x50")
    kw = P.phase_solver_kwargs(m, "separable")
    assert (kw["Lx"], kw["Ly"], kw["lid_velocity"], kw["Re"], kw["grid_stretch"]) == (2.0, 0.5, 2.0, 400.0, 1.0)
    assert kw["convection_scheme"] == "TVD" and kw["pressure_tol"] == 1e-13 and kw["mapping"] == "chip"
    assert "pressure_preconditioner" not in kw


# ---------------------------------------------------------------------------------------------- 2. the seed
ALL_SHAPES = P.CG_SHAPES + [P.BIG]


@pytest.mark.parametrize("nx,ny", ALL_SHAPES, ids=[f"{a}x{b}" for a, b in ALL_SHAPES])
def test_every_seeded_state_has_both_signs_and_closed_walls(nx, ny):
    o = P._state("reference", nx, ny, None, None, "none", 1e-12, K.PRESSURE_TOL, P.BETA)
    u, v, p, mdot = P.seeded_stretched(o)
    assert p[0] == 0.0 and np.max(np.abs(u)) > 0.4 and np.max(np.abs(v)) > 0.3
    fx, fy = o.fx, o.fy
    assert np.all(fx[:, 0] == 0.0) and np.all(fx[:, -1] == 0.0) and np.all(fy[0, :] == 0.0) and np.all(fy[-1, :] == 0.0)
    for f in (fx[:, 1:-1], fy[1:-1, :]):
        assert (f > 0).any() and (f < 0).any()
    assert np.linalg.norm(o.divergence(fx, fy)) > 1e-4                       # non-solenoidal: the pressure solve has work
    assert np.array_equal(mdot, np.concatenate([fx.ravel(), fy.ravel()]))    # the [fx | fy] layout of include/ldc_fv.h
    # the formula of the uniform seed: at beta = 0 the stretched seed is the uniform one to rounding
    if nx * ny < 4000:
        from fv_numpy import FVState
        flat = P.seeded_stretched(P._state("reference", nx, ny, None, None, "none", 1e-12, K.PRESSURE_TOL, 0.0))
        for a, b in zip(flat, K.seeded(FVState(nx, ny, K.RE, **K.SETTINGS))):
            assert np.allclose(a, b, rtol=0, atol=1e-14)


# ---------------------------------------------------------------------------------------------- 3. the capped cases
def test_the_case_lists_hold_the_planned_cases():
    assert P.CG_SHAPES == [(37, 50), (300, 9), (8, 1024), (272, 260), (1024, 72)] and P.CG_CAPS == (1, 3)
    assert len(P.CG_CASES) == 2 * 5 * 2 + 1 and P.CG_CASES[-1] == ("separable", 1024, 1024, 3)
    assert P.cg_mutants(*P.BIG) == ("rz",) and P.cg_mutants(37, 50) == ("rz", "pq")
    assert P.BICG_CASES == [(c, nx, ny) for c in ("reference", "laplacian") for nx, ny in ((37, 50), (300, 9), (272, 260))]
    assert (P.BICG_CAP, P.CAP_K, P.BETA, K.RE, K.PRESSURE_TOL) == (2, 2, 1.5, 400.0, 1e-13)
    assert K.SETTINGS == dict(convection_scheme="TVD", alpha_uv=0.4, alpha_p=0.2, linear_solver_tol=1e-12)
    assert (P.TOL, P.SENSITIVITY_BOUND, P.MUTANT_BOUND) == (1e-9, 1e-10, 1e-7)
    assert [e[:3] + e[4:] for e in P.EDGES] == [(37, 50, 1.0, 12, "TVD"), (24, 40, 2.5, 12, "TVD"), (131, 77, 1.5, 6, "TVD"),
                                               (1024, 72, 1.5, 3, "TVD"), (40, 24, 1.5, 6, "Upwind")]
    assert dict(P.EDGES[0][3]) == dict(Lx=2.0, Ly=0.5, lid_velocity=2.0) and dict(P.EDGES[2][3]) == dict(corner_treatment="smoothing")


@pytest.mark.parametrize("case", P.CG_CASES, ids=P.case_id)
def test_cg_capped_references_carry_the_gpu_tolerance(case):
    chain, nx, ny, cap = case
    t0 = time.perf_counter()
    ref = P.capped_reference(chain, nx, ny, cap)
    dt = time.perf_counter() - t0
    assert _finite(ref)
    assert ref["cg_caps"] == P.CAP_K and ref["cg_iters"] == (cap,) * P.CAP_K      # every pressure solve accepted at the cap
    assert "cap" not in ref["exits"] and len(ref["iters"]) == 2 * P.CAP_K         # (the momentum solves converge)
    sens = K.distance(P.capped_reference(chain, nx, ny, cap, None, "none", 1e-13), ref)
    line = f"cg {P.case_id(case)}: reference {dt:.1f} s, sensitivity {max(sens.values()):.1e}"
    assert max(sens.values()) <= P.SENSITIVITY_BOUND, sens
    mutants = {}
    for which in P.cg_mutants(nx, ny):
        mutants[which] = P.capped_reference(chain, nx, ny, cap, None, which)
        d = K.distance(mutants[which], ref)
        line += f", {which} {max(d.values()):.1e}"
        assert max(d.values()) >= P.MUTANT_BOUND, (which, d)
    print(line)
    # the GPU test's own comparison: the restatement passes it, every mutant in the restatement's place fails it
    P.hold_capped("restatement", ref["rows"], ref, ref, mutants)
    for which, m in mutants.items():
        with pytest.raises(AssertionError):
            P.hold_capped(f"mutant {which}", m["rows"], m, ref, mutants)
    if (nx, ny) != P.BIG:
        for which in ("rr", "bb"):                                              # only the stop test reads them
            m = P.capped_reference(chain, nx, ny, cap, None, which)
            assert all(np.array_equal(m[k], ref[k]) for k in K.FIELDS) and m["cg_iters"] == ref["cg_iters"], which


@pytest.mark.parametrize("case", P.BICG_CASES, ids=P.case_id)
def test_bicgstab_capped_references_carry_the_gpu_tolerance(case):
    chain, nx, ny = case
    ref = P.capped_reference(chain, nx, ny, None, P.BICG_CAP)
    assert _finite(ref)
    assert ref["exits"] == ("cap",) * (2 * P.CAP_K) and ref["iters"] == (P.BICG_CAP,) * (2 * P.CAP_K)
    if chain != "reference":
        assert ref["cg_caps"] == 0 and len(ref["cg_iters"]) == P.CAP_K        # (the pressure solves converge)
    sens = K.distance(P.capped_reference(chain, nx, ny, None, P.BICG_CAP, "none", 1e-13), ref)
    line = f"bicgstab {P.case_id(case)} cap {P.BICG_CAP}: sensitivity {max(sens.values()):.1e}"
    assert max(sens.values()) <= P.SENSITIVITY_BOUND, sens
    mutants = {}
    for which in P.BICG_MOVING:
        mutants[which] = P.capped_reference(chain, nx, ny, None, P.BICG_CAP, which)
        d = K.distance(mutants[which], ref)
        line += f", {which[5:]} {max(d.values()):.1e}"
        assert max(d.values()) >= P.MUTANT_BOUND, (which, d)
    print(line)
    P.hold_capped("restatement", ref["rows"], ref, ref, mutants)
    for which, m in mutants.items():
        with pytest.raises(AssertionError):
            P.hold_capped(f"mutant {which}", m["rows"], m, ref, mutants)
    for which in ("bicg_rr", "bicg_ss", "bicg_bb"):
        m = P.capped_reference(chain, nx, ny, None, P.BICG_CAP, which)
        assert all(np.array_equal(m[k], ref[k]) for k in K.FIELDS) and m["iters"] == ref["iters"], which


@pytest.mark.parametrize("chain", P.CHAINS)
def test_the_copied_loops_with_every_sum_whole_are_the_stretched_restatement_bit_for_bit(chain):
    """``lost_share(cls, None)`` of ``FVStretchedState`` and ``FVSeparableState`` at 37 x 50."""
    runs = [(None, P.BICG_CAP)] if chain == "reference" else [(3, None), (None, P.BICG_CAP), (None, None)]
    for cg_cap, bicg_cap in runs:
        ref = P.capped_reference(chain, 37, 50, cg_cap, bicg_cap)
        copy = P.capped_reference(chain, 37, 50, cg_cap, bicg_cap, None)
        for k in K.FIELDS + ("rows",):
            assert np.array_equal(copy[k], ref[k]), (chain, cg_cap, bicg_cap, k)
        for k in ("iters", "exits", "cg_iters", "cg_caps"):
            assert copy[k] == ref[k], (chain, cg_cap, bicg_cap, k)
    assert issubclass(P.lost_share(SN.FVSeparableState, "rz"), SN.FVSeparableState)
    with pytest.raises(ValueError):
        P.capped_reference("spectral", 37, 50, 3)


# ---------------------------------------------------------------------------------------------- 4. the stop test's norms
@pytest.mark.parametrize("chain", P.CONSISTENT)
def test_a_threshold_beside_the_fifth_residual_tells_a_lost_share_in_either_norm(chain):
    nx, ny = P.THRESHOLD_SHAPE
    c = P.threshold_case(chain, nx, ny)
    assert 0.0 < c["tol_rr"] < c["rho"] < c["tol_bb"] < 1.0
    assert 0.5 * c["d_rr"] >= P.THRESHOLD_MARGIN and 0.5 * c["d_bb"] >= P.THRESHOLD_MARGIN, c
    got = {(w, lost): P.threshold_count(chain, nx, ny, w, lost) for w in ("rr", "bb") for lost in ("none", w)}
    print(f"threshold {chain} {nx}x{ny}: rho {c['rho']:.3e}, lost share of |r_5| {c['d_rr']:.1e}, of |b| {c['d_bb']:.1e}; "
          f"counts {got}")
    assert got["bb", "none"] == P.THRESHOLD_K and got["bb", "bb"] > P.THRESHOLD_K
    assert got["rr", "none"] > P.THRESHOLD_K and got["rr", "rr"] == P.THRESHOLD_K
    for w in ("rr", "bb"):
        assert P.threshold_count(chain, nx, ny, w, "none", 1e-13) == got[w, "none"], w


# ---------------------------------------------------------------------------------------------- 5. edge shapes from rest
@pytest.mark.parametrize("edge", P.EDGES, ids=P.EDGE_IDS)
def test_edge_references_are_finite_and_uncapped(edge):
    nx, ny, beta, geo, K_, scheme = edge
    t0 = time.perf_counter()
    runs = {chain: P.edge_reference(edge, chain) for chain in P.CHAINS}
    dt = time.perf_counter() - t0
    for chain, r in runs.items():
        assert r["rows"].shape == (K_, 8) and np.all(np.isfinite(r["rows"])), chain
        assert all(np.all(np.isfinite(v)) for v in r["state"].values()), chain
        assert "cap" not in r["exits"] and len(r["exits"]) == 2 * K_, chain
        assert r["cg_caps"] == 0 and len(r["cg_iters"]) == (0 if chain == "reference" else K_), chain
        kw = P.edge_solver_kwargs(edge, chain)
        assert (kw["nx"], kw["ny"], kw["grid_stretch"], kw["max_iterations"], kw["convection_scheme"]) == (nx, ny, beta, K_, scheme)
        assert all(kw[k] == v for k, v in geo) and kw["mapping"] == "chip" and kw["Re"] == 400.0
    a, b = runs["laplacian"], runs["separable"]
    fields = max(float(np.max(np.abs(a["state"][k] - b["state"][k]))) for k in a["state"])
    print(f"edge {nx}x{ny} beta {beta} {scheme}: three references {dt:.1f} s; laplacian against separable fields {fields:.1e}; CG "
          f"{a['cg_iters'][-1]} and {b['cg_iters'][-1]}")
    assert fields <= 1e-11


@pytest.mark.parametrize("chain", P.CONSISTENT)
def test_the_count_bound_at_beta_2_5_rests_on_the_restatements_own_sensitivity(chain):
    assert P.COUNTS_EDGE[:5] == S.COUNTS
    assert S.counts_sensitivity(chain) == S.COUNT_SENSITIVITY[chain]
    assert S.count_bound(chain) == dict(separable=1, laplacian=20)[chain]


# ---------------------------------------------------------------------------------------------- 6. NaN, loose solves
@pytest.mark.parametrize("chain", P.CHAINS)
def test_the_nan_case_goes_non_finite_within_the_first_chunk(chain):
    at = S.nan_reference(chain)
    kw = P.nan_solver_kwargs(chain)
    assert at == P.NAN_AT[chain] and at + 1 < kw["check_every"] == P.NAN_CHUNK
    c = S.NAN_CASE
    assert (kw["nx"], kw["ny"], kw["Re"], kw["alpha_uv"], kw["alpha_p"], kw["grid_stretch"]) == (16, 16, 1000.0, 1.0, 1.0, c["beta"])
    assert kw["mapping"] == "chip" and kw["chip_grid"] == "tables"


@pytest.mark.parametrize("chain", P.CHAINS)
def test_the_loose_case_has_unequal_u_v_counts(chain):
    r = S.loose_reference(chain)
    it = np.array(r["iters"]).reshape(-1, 2)
    assert int((it[:, 0] != it[:, 1]).sum()) >= 10 and "cap" not in r["exits"] and r["cg_caps"] == 0
    kw = P.loose_solver_kwargs(chain)
    assert (kw["nx"], kw["ny"], kw["grid_stretch"], kw["linear_solver_tol"], kw["max_iterations"]) == (30, 21, 1.0, 1e-6, 40)
    assert kw["mapping"] == "chip"
