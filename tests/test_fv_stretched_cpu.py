"""Wall-clustered (tanh) grids of one-CU finite-volume trials (grid="tanh", ldc_fv_set_grid, csrc/ldc_fv_stretched.hip), CPU
side: the NumPy restatement (tests/fv_stretched_numpy.py) against the reference's own code on such a mesh (g17,
tests/golden/make_golden_fv_stretched.py), against the uniform restatement at beta = 0 and against dense solves; the host
pieces of the solver (tables, eigenpairs, psi); the C ABI without a device; the parameter surface."""
import ctypes as C
import json
import re
import sys
from pathlib import Path

import numpy as np
import pytest

from conftest import PKG  # noqa: E402
from fv_consistent_numpy import FVConsistentState
from fv_stretched_numpy import (FVStretchedState, axis_tables, generalised_eig, lid_profile_at, streamfunction_matrix,
                                tanh_vertices)

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"
E_ARG, E_STATE = -1, -2
STEP_KEYS = ("grad_p", "diag", "b", "u_star", "v_star", "mdot_star", "rhs_p", "p_prime", "u_prime", "v_prime", "mdot")


@pytest.fixture(scope="module")
def g17():
    return np.load(GOLD / "g17_fv_stretched.npz"), json.loads((GOLD / "g17_fv_stretched.json").read_text())


def state_of(m, **kw):
    args = dict(Lx=m.get("Lx", 1.0), Ly=m.get("Ly", 1.0), lid_velocity=m.get("lid_velocity", 1.0), corner_treatment=m["lid"],
                alpha_uv=m["alpha_uv"], alpha_p=m["alpha_p"], linear_solver_tol=m["linear_solver_tol"],
                convection_scheme=m["convection_scheme"], grid_stretch=m["beta"], pressure_equation="reference")
    args.update(kw)
    return FVStretchedState(m["nx"], m["ny"], m["Re"], **args)


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def _rec_close(ra, rb, tol, flux_scale):
    """Record columns 0 - 6 relative to the other run; |div mdot| (column 3) against the size of the fluxes, since with the
    consistent equation it is zero to the CG tolerance and has no digits of its own to compare."""
    cols = [0, 1, 2, 4, 5, 6]
    return (np.max(np.abs(ra[:, cols] - rb[:, cols]) / np.abs(rb[:, cols])) <= tol
            and np.max(np.abs(ra[:, 3] - rb[:, 3])) <= tol * flux_scale)


def test_fixture_covers_the_cases(g17):
    g, meta = g17
    steps = {t: m for t, m in meta.items() if m["kind"] == "step"}
    trajs = {t: m for t, m in meta.items() if m["kind"] == "traj"}
    assert {(m["nx"], m["ny"], m["beta"]) for m in steps.values()} == {(13, 17, 1.5), (37, 50, 1.0)}
    assert steps["37x50"]["Lx"] == 2.0 and steps["37x50"]["Ly"] == 0.5 and steps["37x50"]["lid_velocity"] == 2.0
    assert {(m["nx"], m["ny"], m["lid"], m["K"], m["beta"]) for m in trajs.values()} == {
        (16, 16, "none", 40, 1.5), (16, 16, "saad", 40, 1.5), (13, 17, "none", 40, 1.5), (8, 67, "none", 30, 1.0),
        (37, 50, "smoothing", 25, 1.0)}
    for m in meta.values():
        assert m["convection_scheme"] == "Upwind" and m["linear_solver_tol"] == 1e-12
    for t in trajs:
        assert g[f"{t}_rec"].shape == (trajs[t]["K"], 4)      # E, Z, P of the reference are uniform formulas: left out


@pytest.mark.parametrize("tag", ["13x17", "37x50"])
def test_restatement_step_matches_reference_intermediates(g17, tag):
    """One iteration from the seeded state, every intermediate.  Measured distance to the reference, relative to the largest
    entry: at most 1.5e-12 (u*, v*: the two BiCGSTAB solves stop at 1e-12 |b|), 1e-13 and below for everything else.  The
    bound is ten times the measured value."""
    g, meta = g17
    s = state_of(meta[tag])
    s.set_state(g[f"{tag}_u0"], g[f"{tag}_v0"], g[f"{tag}_p0"], g[f"{tag}_mdot0"])
    cap = {}
    s.step(cap)
    for k in STEP_KEYS:
        assert _rel(cap[k], g[f"{tag}_{k}"]) <= 1.5e-11, k
    for k in ("u", "v", "p"):
        assert _rel(getattr(s, k).ravel(), g[f"{tag}_{k}"]) <= 1.5e-11, k


def test_restatement_trajectories_match_reference(g17):
    """K iterations from rest, the fields, mdot and record columns 0 - 3.  Measured: record rows 7.7e-11 relative at most,
    u 3.2e-11, v 2.2e-12, p 2.2e-11, mdot 6.1e-13 absolute at most (max |u| <= 2); the reference's pressure solve is BiCGSTAB
    to 1e-12 with an LU preconditioner, this one exact.  The bound is ten times the measured value."""
    g, meta = g17
    for tag, m in meta.items():
        if m["kind"] != "traj":
            continue
        s = state_of(m)
        rec = s.run(m["K"])
        ref = g[f"{tag}_rec"]
        assert np.max(np.abs(rec[:, :4] - ref) / np.abs(ref)) <= 8e-10, tag
        for k, bound in (("u", 3.5e-10), ("v", 3.5e-10), ("p", 3.5e-10)):
            assert np.max(np.abs(getattr(s, k).ravel() - g[f"{tag}_{k}"])) <= bound, (tag, k)
        assert np.max(np.abs(np.concatenate([s.fx.ravel(), s.fy.ravel()]) - g[f"{tag}_mdot"])) <= 3.5e-10, tag


@pytest.mark.parametrize("mode", ["reference", "consistent"])
@pytest.mark.parametrize("nx,ny,kw", [(16, 16, {}), (13, 17, dict(Lx=2.0, Ly=0.5, lid_velocity=2.0))])
def test_beta_zero_is_the_uniform_restatement(mode, nx, ny, kw):
    """grid_stretch = 0 through the stretched statements against ``FVConsistentState``: the fields, mdot and the whole record
    row, E / Z / P included (the Gauss rule with equal widths and a constant lid is the ghost-cell rule), at the 1e-9 that
    tests/test_fv_cpu.py asks of a restatement against a g14 trajectory."""
    common = dict(alpha_uv=0.4, alpha_p=0.2, linear_solver_tol=1e-12, convection_scheme="TVD", pressure_equation=mode,
                  pressure_tol=1e-12, **kw)
    a = FVStretchedState(nx, ny, 100.0, grid_stretch=0.0, **common)
    b = FVConsistentState(nx, ny, 100.0, **common)
    ra, rb = a.run(20), b.run(20)
    assert _rec_close(ra, rb, 1e-9, np.max(np.abs(b.fx)))
    for k in ("u", "v", "p", "fx", "fy"):
        assert _rel(getattr(a, k), getattr(b, k)) <= 1e-9, k
    # and on a field that is not a solution: the two rules for omega, E, Z, P agree to rounding
    rng = np.random.default_rng(3)
    a.u, a.v = rng.normal(size=(ny, nx)), rng.normal(size=(ny, nx))
    b.u, b.v = a.u.copy(), a.v.copy()
    assert np.max(np.abs(a.vorticity() - b.vorticity())) <= 1e-12 * np.max(np.abs(b.vorticity()))
    assert np.allclose(a.quantities(), b.quantities(), rtol=1e-12, atol=0)


def test_generalised_fast_diagonalisation_against_a_dense_solve():
    """The exact pressure solve on 9 x 30, beta = 1.5: the pinned system of Hy (x) Kx + Ky (x) Hx by a dense solve."""
    s = FVStretchedState(9, 30, 100.0, grid_stretch=1.5, pressure_equation="reference")
    for lam, Q, h in ((s.lamx, s.Qx, s.hx), (s.lamy, s.Qy, s.hy)):
        assert np.max(np.abs(Q.T @ np.diag(h) @ Q - np.eye(h.size))) < 1e-12
        assert abs(lam[0]) < 1e-9 * lam[-1] and np.all(np.diff(lam) >= 0)       # (wall modes come in pairs that round together)
        assert np.max(np.abs(Q[:, 0] - Q[0, 0])) < 1e-9 * abs(Q[0, 0])       # the zero mode is a constant
    rng = np.random.default_rng(1)
    rhs = rng.normal(size=(30, 9))
    rhs.flat[0] = 0.0
    x = s.pressure_solve(rhs)
    A = s.reference_dense()
    ref = np.zeros(rhs.size)
    ref[1:] = np.linalg.solve(A[1:, 1:], rhs.ravel()[1:])
    assert x.flat[0] == 0.0
    assert np.max(np.abs(x.ravel() - ref)) <= 1e-10 * np.max(np.abs(ref))
    # h_wall / h_uniform of profiles/fv_stretched.md: 0.33 at beta = 1.5 and 32 cells
    assert tanh_vertices(32, 1.0, 1.5)[1] * 32 == pytest.approx(0.33, abs=0.01)


def test_pcg_against_the_direct_solve():
    """20 TVD iterations with the consistent equation at 13 x 17, beta = 1.5: CG to 1e-12 against the dense pinned solve."""
    common = dict(alpha_uv=0.7, alpha_p=0.3, linear_solver_tol=1e-12, convection_scheme="TVD", grid_stretch=1.5,
                  pressure_equation="consistent", pressure_tol=1e-12)
    a = FVStretchedState(13, 17, 100.0, pressure_solver="cg", **common)
    b = FVStretchedState(13, 17, 100.0, pressure_solver="direct", **common)
    ra, rb = a.run(20), b.run(20)
    assert a.cg_caps == 0 and 0 < max(a.cg_iters) < 100
    assert _rec_close(ra, rb, 1e-8, np.max(np.abs(b.fx)))
    for k in ("u", "v", "p", "fx", "fy"):
        assert _rel(getattr(a, k), getattr(b, k)) <= 1e-9, k
    # the corrected fluxes conserve mass to the CG tolerance, and the walls carry exactly nothing
    assert ra[-1, 3] < 1e-10 and not a.fx[:, 0].any() and not a.fx[:, -1].any() and not a.fy[0].any() and not a.fy[-1].any()


def test_stretched_streamfunction_is_second_order():
    """The non-uniform 5-point Dirichlet problem against psi = sin(pi x) sin(pi y) on the ring-anchored domain (the ring of
    cell centres is where psi = 0, as in the uniform rule), beta = 1.5, 24 and 48 cells.  Measured order: 1.97."""
    sys.path.insert(0, str(PKG / "src"))
    from solvers.fv.solver import stretched_streamfunction_matrix
    from scipy.sparse.linalg import spsolve
    errs = []
    for n in (24, 48):
        xc, _, d, _ = axis_tables(tanh_vertices(n, 1.0, 1.5))
        a, L = xc[0], xc[-1] - xc[0]
        X, Y = np.meshgrid((xc - a) / L, (xc - a) / L)
        exact = np.sin(np.pi * X) * np.sin(np.pi * Y)
        omega = 2.0 * (np.pi / L) ** 2 * exact                      # -laplace psi
        A = stretched_streamfunction_matrix(d, d)
        assert np.max(np.abs(A.toarray() - streamfunction_matrix(d, d))) < 1e-9 * np.max(np.abs(A.toarray()))
        psi = spsolve(A, -omega[1:-1, 1:-1].ravel()).reshape(n - 2, n - 2)
        errs.append(np.max(np.abs(psi - exact[1:-1, 1:-1])))
    order = np.log2(errs[0] / errs[1])
    print("order", order, errs)
    assert order >= 1.8


def test_host_tables_are_the_restatements():
    sys.path.insert(0, str(PKG / "src"))
    from solvers.fv import solver as S
    for n, L, beta in ((13, 2.0, 1.5), (50, 0.5, 1.0), (16, 1.0, 0.0)):
        xv = S.tanh_vertices(n, L, beta)
        assert np.array_equal(xv, tanh_vertices(n, L, beta)) and xv[0] == 0.0 and xv[-1] == pytest.approx(L, rel=1e-15)
        assert np.all(np.diff(xv) > 0) and np.allclose(np.diff(xv), np.diff(xv)[::-1], rtol=1e-12)
        for a, b in zip(S.axis_tables(xv), axis_tables(xv)):
            assert np.array_equal(a, b)
        _, h, d, g = S.axis_tables(xv)
        assert d[0] == 0.5 * h[0] and d[-1] == 0.5 * h[-1] and np.all((g[1:-1] > 0) & (g[1:-1] < 1))
        lam, Q = S.generalised_eig_host(h, d)
        lam2, Q2 = generalised_eig(h, d)
        assert np.array_equal(lam, lam2) and np.array_equal(Q, Q2)
        for lid in ("none", "saad", "smoothing"):
            xf = 0.5 * (xv[:-1] + xv[1:])
            assert np.array_equal(S.lid_profile_at(xf, L, 2.0, lid, 0.15), lid_profile_at(xf, L, 2.0, lid, 0.15))
    # uniform vertices: the lid of the uniform builder
    xv = S.tanh_vertices(13, 2.0, 0.0)
    assert np.allclose(S.lid_profile_at(0.5 * (xv[:-1] + xv[1:]), 2.0, 2.0, "smoothing", 0.15),
                       S.lid_profile(13, 2.0, 2.0, "smoothing", 0.15), rtol=0, atol=1e-14)
    assert S.GRIDS == ("uniform", "tanh")


# ---------------------------------------------------------------------- the C ABI without a device
@pytest.fixture(scope="module")
def fvlib():
    import __graft_entry__ as g
    g.build()
    from solvers.fv import ldc_fv_lib
    return ldc_fv_lib


class HostFv(C.Structure):
    """The library's host-side ``struct ldc_fv`` (csrc/ldc_fv_common.inc), the grid mode at its end."""
    _fields_ = [("dev", C.c_void_p), ("ctrl", C.c_void_p), ("rec_cap", C.c_int), ("device", C.c_int), ("nx", C.c_int),
                ("ny", C.c_int), ("dx", C.c_double), ("dy", C.c_double), ("pressure_mode", C.c_int), ("grid_mode", C.c_int)]


def test_set_grid_is_declared_exported_and_bound(fvlib):
    hdr = (ROOT / "include" / "ldc_fv.h").read_text()
    L = fvlib.lib()
    assert "ldc_fv_set_grid" in fvlib.EXPORTS and re.search(r"int ldc_fv_set_grid\(", hdr)
    assert L.ldc_fv_set_grid.restype is C.c_int and callable(fvlib.set_grid)
    val = lambda name: int(re.search(rf"#define {name} \(?(-?\d+)", hdr).group(1))        # noqa: E731
    assert (val("LDC_FV_GRID_UNIFORM"), val("LDC_FV_GRID_TABLES")) == (0, 1) and fvlib.GRID_MODES == dict(uniform=0, tanh=1)
    assert fvlib.grid_table_len(13) == 41 and "#define LDC_FV_GRID_TABLE_LEN(n) (3 * (int64_t)(n) + 2)" in hdr
    assert "csrc/ldc_fv_stretched.hip" in hdr.split(" *\n", 1)[0]              # the unit list at the head
    assert "Stretched grids of a one-CU trial" in hdr and "ldc_fv_stretched_launch" not in hdr
    import __graft_entry__ as g
    assert g.SRC_FV_STRETCHED.name == "ldc_fv_stretched.hip" and g.SRC_FV_STRETCHED.exists()
    # the blocks of the descriptor slot do not overlap, and the descriptor has not grown
    inc = (PKG / "csrc" / "ldc_fv_common.inc").read_text()
    assert "constexpr int kFvGridOffset = 328;" in inc and "constexpr int kFvCuPcgOffset = 384;" in inc
    assert C.sizeof(fvlib.Grid) == 40


def test_set_grid_validation_needs_no_device(fvlib):
    L = fvlib.lib()
    G = fvlib.Grid
    fake = 8                                                     # never dereferenced by a refused call
    call = L.ldc_fv_set_grid
    assert HostFv.grid_mode.offset == 52
    good = dict(mode=1, pad=0, x_tables=fake, y_tables=fake, x_len=3 * 13 + 2, y_len=3 * 17 + 2)
    assert call(None, C.byref(G(**good))) == E_STATE
    for start in (0, 1):                                         # a refused call leaves the modes alone
        h = HostFv(dev=None, ctrl=None, rec_cap=4, device=63, nx=13, ny=17, dx=1 / 13, dy=1 / 17, pressure_mode=1,
                   grid_mode=start)
        hp = C.c_void_p(C.addressof(h))
        for bad in (dict(mode=2), dict(mode=-1), dict(x_tables=None), dict(y_tables=None), dict(x_len=3 * 13 + 1),
                    dict(y_len=3 * 17 + 1), dict(x_len=0)):
            assert call(hp, C.byref(G(**dict(good, **bad)))) == E_ARG, bad
            assert (h.grid_mode, h.pressure_mode) == (start, 1), bad
    # back to the uniform kernels: by mode and by NULL, neither touches the device; the pressure mode stays
    h = HostFv(device=63, nx=13, ny=17, rec_cap=4, pressure_mode=1, grid_mode=1)
    hp = C.c_void_p(C.addressof(h))
    assert call(hp, C.byref(G(mode=0))) == 0 and (h.grid_mode, h.pressure_mode) == (0, 1)
    h.grid_mode = 1
    assert call(hp, None) == 0 and h.grid_mode == 0
    # the debug kernel is the uniform reference iteration
    h.grid_mode, h.pressure_mode = 1, 0
    assert L.ldc_fv_step_debug(hp, 0, None, None) == E_ARG


# ---------------------------------------------------------------------- the parameter surface
def test_parameter_surface_and_rejections(monkeypatch):
    from solvers.datastructures import FVParameters
    from solvers.fv import solver as S
    from solvers.fv.fsg import _LEVEL_FIELDS, FVFSGSolver
    from solvers.spectral import ldc_lib
    p = FVParameters()
    assert (p.grid, p.grid_stretch) == ("uniform", 1.5)
    ml = FVParameters(grid="tanh", grid_stretch=1.0).to_mlflow()
    assert (ml["grid"], ml["grid_stretch"]) == ("tanh", 1.0)
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)        # every ValueError comes before the device
    base = dict(name="fv", Re=100.0, nx=16, ny=16)
    for ok in (dict(), dict(grid_stretch=0.0), dict(pressure_equation="consistent_cu"), dict(nx=13, ny=17, Lx=2.0, Ly=0.5),
               dict(vortex_metrics="host", streamfunction="reference", vortex_refine="none", acceleration="none")):
        with pytest.raises(ldc_lib.LdcError, match="no CPU fallback"):
            S.FVSolver(**dict(base, grid="tanh", **ok))
    with pytest.raises(ldc_lib.LdcError, match="no CPU fallback"):        # read only with grid="tanh"
        S.FVSolver(**dict(base, grid_stretch=-1.0))
    with pytest.raises(ValueError, match="'uniform' or 'tanh'"):
        S.FVSolver(**dict(base, grid="cosine"))
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="grid_stretch"):
            S.FVSolver(**dict(base, grid="tanh", grid_stretch=bad))
    rejected = [(dict(mapping="chip"), "mapping"), (dict(mapping="shared"), "mapping"),
                (dict(acceleration="anderson"), "acceleration"),
                (dict(mapping="chip", acceleration="anderson_chip"), "mapping|acceleration"),
                (dict(vortex_metrics="device"), "vortex_metrics"),
                (dict(mapping="chip", vortex_metrics="chip"), "mapping|vortex_metrics"),
                (dict(streamfunction="wall"), "streamfunction"),
                (dict(streamfunction="wall", vortex_refine="quadratic"), "streamfunction|vortex_refine")]
    for kw, word in rejected:
        with pytest.raises(ValueError, match=f"grid='tanh' with ({word})"):
            S.FVSolver(**dict(base, grid="tanh", **kw))
    with pytest.raises(ValueError, match="grid='tanh' with solver=fv/fsg"):
        FVFSGSolver(**dict(base, grid="tanh"))
    assert "grid" in _LEVEL_FIELDS and "grid_stretch" in _LEVEL_FIELDS
    # start_from and prolong name the option too (no device is touched before the check)
    ns = lambda stretched: type("T", (), dict(stretched=stretched, device=torch.device("cpu")))()        # noqa: E731
    with pytest.raises(ValueError, match="start_from with grid='tanh'"):
        S.prolong([(ns(False), ns(True))])
    with pytest.raises(ValueError, match="grid='tanh'"):
        S.postprocess([ns(True)])


def test_the_launcher_composes_the_keys():
    sys.path.insert(0, str(PKG))
    from utilities.config import compose as Cmp
    comp = Cmp.Composer(PKG / "conf")
    plain = Cmp.resolve(Cmp.compose_job(comp, ["solver=fv", "N=16"], []))
    got = Cmp.resolve(Cmp.compose_job(comp, ["solver=fv", "N=16", "+solver.grid=tanh", "+solver.grid_stretch=1.5"], []))
    assert got["solver"] == dict(plain["solver"], grid="tanh", grid_stretch=1.5)
    assert "grid" not in plain["solver"]                        # the default: uniform
