"""The stretched chip chain (grid="tanh", mapping="chip", chip_grid="tables", with either pressure equation and either chip
preconditioner; csrc/ldc_fv_wide_stretched.inc, csrc/ldc_fv_wide_separable.inc) on the GPU, phase by phase and at its edges:
every phase of one iteration from a seeded state with both signs among the face fluxes, read from the work vectors; CG and
BiCGSTAB iterates accepted at a low cap from a seeded state, up to 1024 x 1024 cells, where a dot product that lost a
work-group's share shows in the fields; the two norms of the CG stop test at a threshold; trajectories from rest on a
rectangle with another lid speed, at grid_stretch 2.5, with a smoothed lid, at 1024 x 72 and with upwinding; the NaN latch;
loose momentum solves with unequal u / v counts.  "reference", "laplacian" and "separable" name the three chains throughout.

Every tolerance is that of the same comparison in tests/test_gpu_fv_stretched_edges.py (the one-CU stretched kernels) or
tests/test_gpu_fv_krylov_caps.py (the uniform chip chain).  The restatement runs are the probe's
(tests/fv_wide_stretched_probe.py), made once per case; tests/test_fv_wide_stretched_edges_cpu.py asserts their preconditions
and that the capped comparison fails on every mutant.  The mutants are test doubles of the restatement; no faulty kernel is
built.  Each test prints its largest error over the tolerance, the mutants' distances, the counters and its time on the card
(profiles/fv_wide_stretched_edges.md)."""
import sys
import time
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import fv_krylov_probe as K  # noqa: E402
import fv_stretched_probe as S  # noqa: E402
import fv_wide_stretched_probe as P  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(float).eps)
FIELDS = K.FIELDS
CONSISTENT_COLS = K.REC_COLS                    # |div mdot| (3) of a converged CG has no digits: held against max |mdot|


@pytest.fixture(scope="module")
def fv():
    import __graft_entry__ as g
    g.build()
    from solvers.fv.solver import FVSolver
    return FVSolver


def _walls(m, nx, ny):
    fx, fy = m[: ny * (nx + 1)].reshape(ny, nx + 1), m[ny * (nx + 1):].reshape(ny + 1, nx)
    return fx[:, 0], fx[:, -1], fy[0], fy[-1]


def _trajectory_devs(rows, state, ref_rows, ref_state, chain):
    """(record columns relative, column 3 over max |mdot|, fields relative) against a restatement run."""
    assert rows.shape == ref_rows.shape, (rows.shape, ref_rows.shape)
    assert np.all(np.isfinite(rows[:, :7]))
    cols = list(range(7)) if chain == "reference" else CONSISTENT_COLS
    devs = dict(rows=P.rows_rel(rows[:, cols], ref_rows[:, cols]),
                div=float(np.max(np.abs(rows[:, 3] - ref_rows[:, 3])) / np.max(np.abs(ref_state["mdot"]))))
    devs.update({k: P.rel(state[k], ref_state[k]) for k in FIELDS})
    return devs


def _assert_trajectory(what, devs, bound):
    print(f"WIDE-EDGE {what}: error / tolerance {max(devs.values()) / bound:.2e}; " + ", ".join(f"{k} {v:.2e}" for k, v in devs.items())
          + f" (bound {bound:.0e})")
    for k, v in devs.items():
        assert v <= bound, (what, k, v)


def _is_chain(s, chain):
    return (s.chip and s.stretched and s.chip_tables and s.chip_separable == (chain == "separable")
            and s.consistent == (chain != "reference") and not s.consistent_cu)


# ------------------------------------------------------------------------------------------- a. phases from a seeded state
@pytest.mark.parametrize("chain", P.CHAINS)
@pytest.mark.parametrize("tag", P.PHASE_TAGS)
def test_every_phase_of_one_iteration_from_a_seeded_state(fv, tag, chain):
    """tests/test_gpu_fv_stretched_edges.py::test_every_phase_of_one_iteration_from_a_seeded_state on the chip chain: the seeds
    of g17's step fixtures (13 x 17 at beta 1.5, one work-group; 37 x 50 = 1850 cells at beta 1, Lx 2, Ly 0.5, lid 2, Re 400,
    eight work-groups) with TVD on both sides, one ``step(capture)`` of the restatement with the dense pressure solve against one
    ``_advance(1)``.  Relative to max |ref|: 1e-10 up to rhs_p, 1e-8 for the reference chain's p', 1e-9 for u', v', mdot, omega,
    the record row and u, v, p; the first key that departs names the phase.  A consistent chain's p' by the residual condition:
    x* the dense solve of the chain's own right-hand side with the restatement's A, |x - x*| <= pressure_tol |b| / lam1 +
    64 eps |x*|; the recurrence residual left in PCG_R obeys the stop test.  The separable chain: s to 1e-12, and the vector
    s . r equal to s times that residual bit for bit (``xr*`` writes both in one statement: an s . r left stale by one CG
    iteration fails here).  Then ten more iterations on both sides to 1e-9."""
    from solvers.fv import ldc_fv_lib as F
    m, seed = P.phase_case(tag)
    nx, ny = m["nx"], m["ny"]
    consistent = chain != "reference"
    tol = P.PHASE_TOL["pressure_tol"]
    ref = P.phase_reference(tag, consistent)
    cap = ref["cap"]
    s = fv(**P.phase_solver_kwargs(m, chain))
    assert _is_chain(s, chain)
    assert F.wide_groups(nx, ny) == {221: 1, 1850: 8}[nx * ny]
    s.set_state(*seed)
    s._begin(1e-30)
    t0 = time.perf_counter()
    rows, done, total = s._advance(1)
    dt = time.perf_counter() - t0
    assert total == 1 and not done and rows.shape == (1, 8) and np.all(np.isfinite(rows[:, :7]))
    got = P.intermediates(s, chain)
    st = s.state()
    c = s.counters()
    devs = {}
    for k in ("grad_p", "diag", "b", "u_star", "v_star", "mdot_star", "rhs_p"):            # in the order of the phases
        if k == "mdot_star" and not consistent:
            continue
        assert np.all(np.isfinite(got[k])), k
        devs[k] = (P.rel(got[k], cap[k]), 1e-10)
    if consistent:
        assert got["rhs_p"][0] == 0.0
        for f in (got["mdot"], got["mdot_star"]):                                         # walls: exactly 0.0
            for wall in _walls(f, nx, ny):
                assert not wall.any()
        b = got["rhs_p"].reshape(ny, nx).copy()
        b.flat[0] = -np.sum(b.ravel()[1:])
        A = ref["A"]
        o = S.restatement("laplacian", nx, ny, m["Re"], grid_stretch=m["beta"], **S.phase_geometry(m))      # (for apply)
        xs = np.zeros(nx * ny)
        xs[1:] = np.linalg.solve(A[1:, 1:], b.ravel()[1:])
        x = got["y"]
        xm, xsm = x - x.mean(), xs - xs.mean()
        err = float(np.linalg.norm(xm - xsm))
        bound = tol * np.linalg.norm(b) / ref["lam1"] + 64 * EPS * np.linalg.norm(xsm)
        devs["p_prime"] = (err, float(bound))
        far = float(np.linalg.norm(xm - (ref["xs"].ravel() - ref["xs"].mean())))
        print(f"WIDE-EDGE phases {tag} {chain}: CG {c['pressure_last']} iterations, |x - x*| {err:.2e} (x* of the restatement's "
              f"b: {far:.2e}), bound {bound:.2e}")
        assert c["pressure_caps"] == 0 and c["pressure_solves"] == 1 and c["pressure_last"] >= 1
        r_true = b - o.apply(ref["wx"], ref["wy"], x.reshape(ny, nx))
        ratio = float(np.linalg.norm(r_true) / (tol * np.linalg.norm(b)))
        rec = float(np.linalg.norm(got["cg_r"]) / (tol * np.linalg.norm(b)))
        print(f"WIDE-EDGE phases {tag} {chain}: |b - A y| / (pressure_tol |b|) {ratio:.3f}, the recurrence's |r| likewise {rec:.3f}")
        assert rec <= 1.0 + 4 * nx * ny * EPS            # the stop test itself, the norms summed in another order
        if chain == "separable":
            devs["sep_s"] = (P.rel(got["sep_s"], ref["s"]), 1e-12)
            devs["true_residual"] = (ratio, 2.0)         # pressure_tol |b| and a factor of 2 for residual drift
            stale = int(np.count_nonzero(got["sep_sr"] != got["sep_s"] * got["cg_r"]))
            print(f"WIDE-EDGE phases {tag} {chain}: cells where s . r is not s times r, bit for bit: {stale}")
            assert stale == 0 and np.any(got["sep_sr"] != 0.0)
    else:
        # (no ``b00``: the first GEMM, fv_wide_gemm<true, false>, takes it from the slot sum of the faces launch as it loads
        # entry (0, 0); no work vector holds it -- fv_wide_stretched_probe.NOT_STORED)
        assert "b00" not in got and got["rhs_p"][0] == 0.0
        devs["p_prime"] = (P.rel(got["p_prime"], cap["p_prime"]), 1e-8)
    for k in ("u_prime", "v_prime", "mdot"):
        devs[k] = (P.rel(got[k], cap[k]), 1e-9)
    devs["omega"] = (P.rel(got["omega"], ref["omega"]), 1e-9)
    cols = CONSISTENT_COLS if consistent else list(range(7))
    devs["row"] = (P.rows_rel(got["row"][cols], ref["row"][cols]), 1e-9)
    devs["row_div"] = (abs(got["row"][3] - ref["row"][3]) / float(np.max(np.abs(cap["mdot"]))), 1e-9)
    for k in ("u", "v", "p"):
        devs[k] = (P.rel(st[k], ref["state"][k]), 1e-9)
    worst = max(devs, key=lambda k: devs[k][0] / devs[k][1])
    print(f"WIDE-EDGE phases {tag} {chain} ({dt * 1e3:.1f} ms): error / tolerance {devs[worst][0] / devs[worst][1]:.2e} ({worst}); "
          + ", ".join(f"{k} {v:.2e}/{b_:.0e}" for k, (v, b_) in devs.items()))
    for k, (v, bound) in devs.items():                   # dicts keep the order: the first failure names the phase
        assert v <= bound, (tag, chain, k, v, bound)
    rows, _, total = s._advance(P.PHASE_MORE)
    assert total == 1 + P.PHASE_MORE
    _assert_trajectory(f"phases+{P.PHASE_MORE} {tag} {chain}",
                       _trajectory_devs(rows, s.state(), ref["rows"], ref["state_after"], chain), 1e-9)
    assert s.counters()["linear_giveups"] == 0
    s.close()


# ------------------------------------------------------------------------------------------- b, c. iterates accepted at a cap
def _run_seeded(FVSolver, chain, nx, ny, advances=P.CAP_K, **kw):
    """The stretched seed through ``set_state``, ``_begin``, then ``advances`` calls of ``_advance(1)``: (rows, state, counters,
    the counters after every call, seconds on the card)."""
    s = FVSolver(**P.solver_kwargs(chain, nx, ny, **kw))
    assert _is_chain(s, chain)
    s.set_state(*P.seed_of(nx, ny))
    s._begin(1e-30)
    rows, after = [], []
    t0 = time.perf_counter()
    for k in range(advances):
        r, done, total = s._advance(1)                 # (a cap hit is accepted: no overflow, no retry of the pressure budget)
        assert total == k + 1 and not done and r.shape == (1, 8)
        rows.append(r)
        after.append(s.counters())
    dt = time.perf_counter() - t0
    out = (np.concatenate(rows, axis=0), s.state(), s.counters(), after, dt)
    s.close()
    return out


def _assert_ran(c):
    assert c["nan"] == 0 and c["done"] == 0 and c["iterations"] == P.CAP_K and c["momentum_solves"] == 2 * P.CAP_K


@pytest.mark.parametrize("case", P.CG_CASES, ids=P.case_id)
def test_cg_iterates_accepted_at_a_cap(fv, case):
    """pressure_max_iters 1 and 3, two iterations from the stretched seed: fields and record columns within 1e-9 of the capped
    restatement, and farther than that from its ``rz`` and ``pq`` mutants (a sum without the first 1 / 256 of the cells).  Every
    solve counted at its cap.  37 x 50: eight groups, ragged GEMM tiles; 300 x 9 and 8 x 1024: one axis past the one-CU range,
    the other beside MIN_N; 272 x 260: 256 work-groups and a second pass of the grid-stride loop; 1024 x 72; and one
    1024 x 1024 run (separable, cap 3, ``rz``)."""
    from solvers.fv import ldc_fv_lib as F
    chain, nx, ny, cap = case
    assert F.wide_groups(nx, ny) == {1850: 8, 2700: 11, 8192: 32, 70720: 256, 73728: 256, 1 << 20: 256}[nx * ny]
    t0 = time.perf_counter()
    ref = P.capped_reference(chain, nx, ny, cap)
    mutants = {w: P.capped_reference(chain, nx, ny, cap, None, w) for w in P.cg_mutants(nx, ny)}
    cpu = time.perf_counter() - t0
    rows, st, c, _, dt = _run_seeded(fv, chain, nx, ny, pressure_max_iters=cap)
    print(f"WIDE-EDGE cg-cap {P.case_id(case)}: card {dt:.2f} s, references {cpu:.1f} s, {c}")
    P.hold_capped(f"WIDE-EDGE cg-cap {P.case_id(case)}", rows, st, ref, mutants)
    _assert_ran(c)
    assert (c["pressure_iterations"], c["pressure_solves"], c["pressure_caps"], c["pressure_last"]) == (cap * P.CAP_K, P.CAP_K,
                                                                                                        P.CAP_K, cap)
    assert c["linear_giveups"] == 0 and c["linear_iterations"] == sum(ref["iters"])
    assert c["pressure_budget_retries"] == 0
    for wall in _walls(st["mdot"], nx, ny):
        assert not wall.any()


@pytest.mark.parametrize("case", P.BICG_CASES, ids=P.case_id)
def test_bicgstab_iterates_accepted_at_a_cap(fv, monkeypatch, case):
    """max_lin_iters 2: all four momentum solves give up at the cap and their iterates are accepted; fields and record columns
    within 1e-9 of the restatement and farther from its ``bicg_rho``, ``bicg_rv``, ``bicg_ts`` and ``bicg_tt`` mutants."""
    import solvers.fv.solver as Sv
    monkeypatch.setattr(Sv, "LINEAR_MAX_ITERATIONS", P.BICG_CAP)
    chain, nx, ny = case
    ref = P.capped_reference(chain, nx, ny, None, P.BICG_CAP)
    mutants = {w: P.capped_reference(chain, nx, ny, None, P.BICG_CAP, w) for w in P.BICG_MOVING}
    rows, st, c, _, dt = _run_seeded(fv, chain, nx, ny)
    print(f"WIDE-EDGE bicg-cap {P.case_id(case)}: card {dt:.2f} s, {c}")
    P.hold_capped(f"WIDE-EDGE bicg-cap {P.case_id(case)}", rows, st, ref, mutants)
    _assert_ran(c)
    assert c["linear_giveups"] == ref["exits"].count("cap") == 2 * P.CAP_K
    assert c["linear_iterations"] == sum(ref["iters"]) == 2 * P.CAP_K * P.BICG_CAP
    if chain != "reference":                           # the pressure solves converge (restatement: ref["cg_iters"])
        assert c["pressure_solves"] == P.CAP_K and c["pressure_caps"] == 0


# ------------------------------------------------------------------------------------------- d. the stop test's own norms
@pytest.mark.parametrize("chain", P.CONSISTENT)
def test_cg_stops_where_the_whole_norms_say(fv, chain):
    """|r|^2 (``xr*``, ``pcg_xr``) and |b|^2 (``init*``, ``pcg_init``) enter only the stop test: no capped iterate shows them.
    272 x 260 with pressure_tol set beside |r_5| / |b| of the first solve (``threshold_case``: at least 1e-6 away, relative):
    the card's count is the restatement's exactly, and not that of its ``rr`` or ``bb`` mutant."""
    nx, ny = P.THRESHOLD_SHAPE
    case = P.threshold_case(chain, nx, ny)
    for which in ("rr", "bb"):
        want, mutant = P.threshold_count(chain, nx, ny, which), P.threshold_count(chain, nx, ny, which, which)
        _, _, c, _, dt = _run_seeded(fv, chain, nx, ny, advances=1, pressure_tol=case["tol_" + which])
        print(f"WIDE-EDGE threshold {chain} {nx}x{ny} pressure_tol {case['tol_' + which]:.6e} ({which}): CG count "
              f"{c['pressure_last']}, restatement {want}, its {which} mutant {mutant}; card {dt:.2f} s")
        assert want != mutant and P.THRESHOLD_K in (want, mutant)
        assert c["pressure_last"] == want and c["pressure_caps"] == 0 and c["pressure_solves"] == 1 and c["nan"] == 0


# ------------------------------------------------------------------------------------------- e. edge shapes from rest
@pytest.mark.parametrize("chain", P.CHAINS)
@pytest.mark.parametrize("edge", P.EDGES, ids=P.EDGE_IDS)
def test_trajectories_from_rest_at_the_settings_nobody_ran(fv, edge, chain):
    """Re 400, linear_solver_tol 1e-12, pressure_tol 1e-13, from rest, against the restatement with the chain's own pressure
    solve; fields and record columns to 1e-9, |div mdot| against max |mdot|: 37 x 50 at beta 1 on a 2 x 0.5 rectangle with a lid
    of 2; 24 x 40 at grid_stretch 2.5; 131 x 77 with corner_treatment "smoothing"; 1024 x 72 (the first stretched chip run at
    1024 cells that is held against NumPy); 40 x 24 with upwinding.  One iteration per call, so every solve's CG count is read:
    at beta 2.5 each is within ``fv_stretched_probe.count_bound`` of the restatement's (1 with the separable preconditioner; 20
    with the laplacian one, ten times what the restatement's own counts move by under input rounding, measured on the CPU)."""
    nx, ny, beta, geo, K_, scheme = edge
    ref = P.edge_reference(edge, chain)
    s = fv(**P.edge_solver_kwargs(edge, chain))
    assert _is_chain(s, chain)
    s._begin(1e-30)
    rows, per_solve = [], []
    t0 = time.perf_counter()
    for _ in range(K_):
        rows.append(s._advance(1)[0])
        per_solve.append(s.counters().get("pressure_last"))
    dt = time.perf_counter() - t0
    rows = np.concatenate(rows, axis=0)
    c = s.counters()
    what = f"edge {nx}x{ny} beta {beta} {scheme} {chain}"
    print(f"WIDE-EDGE {what}: card {dt:.2f} s for {K_} iterations, {c}")
    _assert_trajectory(what, _trajectory_devs(rows, s.state(), ref["rows"], ref["state"], chain), 1e-9)
    assert c["iterations"] == K_ and c["nan"] == 0 and c["linear_giveups"] == 0 and c["momentum_solves"] == 2 * K_
    if chain != "reference":
        worst = max(abs(a - b) for a, b in zip(per_solve, ref["cg_iters"]))
        print(f"WIDE-EDGE {what}: CG per solve, card {per_solve}, restatement {list(ref['cg_iters'])}, worst {worst}")
        assert c["pressure_caps"] == 0 and c["pressure_solves"] == K_ and c["pressure_iterations"] == sum(per_solve)
        for wall in _walls(s.state()["mdot"], nx, ny):
            assert not wall.any()
        if edge == P.COUNTS_EDGE:
            assert worst <= S.count_bound(chain), (per_solve, ref["cg_iters"])
    s.close()


# ------------------------------------------------------------------------------------------- f. the NaN latch
@pytest.mark.parametrize("chain", P.CHAINS)
def test_a_lone_nan_trial_raises(fv, chain):
    """16 x 16, beta 1.5, Re 1000 without under-relaxation (tests/test_gpu_fv_stretched_edges.py::test_a_lone_nan_trial_raises):
    a numerical blow-up of the SIMPLE iteration.  The restatement's first non-finite record row is row 10 (consistent) or 11
    (reference), counted from 0; the chain's NaN latch stops the trial within its first chunk of 32."""
    from solvers.spectral.ldc_lib import LdcError
    kw = P.nan_solver_kwargs(chain)
    s = fv(**kw)
    assert _is_chain(s, chain)
    t0 = time.perf_counter()
    with pytest.raises(LdcError, match="NaN"):
        s.solve()
    dt = time.perf_counter() - t0
    c = s.counters()
    print(f"WIDE-EDGE nan {chain}: card {dt:.2f} s, {c} (restatement: iteration {P.NAN_AT[chain]})")
    assert c["nan"] == 1 and c["done"] == 0 and c["iterations"] < kw["check_every"]
    s.close()


# ------------------------------------------------------------------------------------------- g. loose linear solves
@pytest.mark.parametrize("chain", P.CHAINS)
def test_loose_linear_solves_with_unequal_u_v_counts(fv, chain):
    """linear_solver_tol 1e-6 at 30 x 21, Re 400, beta 1: u and v leave the shared BiCGSTAB loop at different iterations in 16
    or 17 of the 40 iterations (the restatement).  The counters are the restatement's; fields to 1e-8, the bound of
    tests/test_gpu_fv_stretched_edges.py::test_loose_linear_solves_with_unequal_u_v_counts."""
    K_ = S.LOOSE["K"]
    ref = S.loose_reference(chain)
    s = fv(**P.loose_solver_kwargs(chain))
    assert _is_chain(s, chain)
    t0 = time.perf_counter()
    s.solve()
    dt = time.perf_counter() - t0
    c = s.counters()
    print(f"WIDE-EDGE loose {chain}: card {dt:.2f} s, linear iterations {c['linear_iterations']}, restatement {sum(ref['iters'])}")
    assert c["linear_giveups"] == ref["exits"].count("cap") == 0 and c["momentum_solves"] == 2 * K_ and c["iterations"] == K_
    assert c["linear_iterations"] == sum(ref["iters"])
    if chain != "reference":
        assert c["pressure_solves"] == K_ and c["pressure_caps"] == ref["cg_caps"] == 0
    _assert_trajectory(f"loose {chain}", _trajectory_devs(s.history, s.state(), ref["rows"], ref["state"], chain), 1e-8)
    s.close()
