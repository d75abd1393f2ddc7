"""Finite-volume prolongation and grid sequencing, CPU side: the NumPy restatement (tests/fv_prolong_numpy.py) on
analytic fields, the level hierarchy, the parameter surface and configuration of ``solver=fv/fsg``, the C ABI of
ldc_fv_prolong_enqueue without a device, and the sequenced solve 16^2 -> 32^2 on the restatement."""
import ctypes as C
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
import fv_prolong_numpy as P  # noqa: E402
from fv_numpy import FVState  # noqa: E402

from conftest import PKG  # noqa: E402

PAIRS = [((8, 8), (16, 16)), ((12, 8), (25, 17)), ((9, 13), (9, 13))]


def _centres(s):
    return np.meshgrid((np.arange(s.nx) + 0.5) * s.dx, (np.arange(s.ny) + 0.5) * s.dy)


def _pair(coarse, fine, lid="none", seed=0):
    rng = np.random.default_rng(seed)
    c = FVState(coarse[0], coarse[1], 100.0, corner_treatment=lid)
    f = FVState(fine[0], fine[1], 100.0, corner_treatment=lid)
    c.u, c.v, c.p = (rng.standard_normal((c.ny, c.nx)) for _ in range(3))
    f.u, f.v, f.p = (np.full((f.ny, f.nx), np.nan) for _ in range(3))
    return c, f


@pytest.mark.parametrize("coarse,fine", PAIRS)
def test_a_bilinear_pressure_is_reproduced_up_to_the_shift(coarse, fine):
    c, f = _pair(coarse, fine)
    bil = lambda X, Y: 0.7 - 1.3 * X + 0.45 * Y + 2.1 * X * Y        # noqa: E731
    c.p = bil(*_centres(c))
    P.prolong(c, f)
    # fine cells whose four coarse nodes are all cell centres: the stencil does not touch the ring
    kx, _ = P.locate(c.nx, c.dx, f.nx, f.dx)
    ky, _ = P.locate(c.ny, c.dy, f.ny, f.dy)
    inner = ((ky >= 1) & (ky + 1 <= c.ny))[:, None] & ((kx >= 1) & (kx + 1 <= c.nx))[None, :]
    assert inner.sum() >= (f.nx - 4) * (f.ny - 4) > 0
    shift = (f.p - bil(*_centres(f)))[inner]
    err = float(np.max(np.abs(shift - shift[0])))
    print(coarse, fine, "bilinear p: max deviation from one shift", err)
    assert err <= 1e-13
    assert f.p[0, 0] == 0.0


def test_the_same_grid_is_the_identity():
    c, f = _pair((9, 13), (9, 13), lid="saad")
    P.prolong(c, f)
    assert np.max(np.abs(f.u - c.u)) <= 1e-13 and np.max(np.abs(f.v - c.v)) <= 1e-13
    assert np.max(np.abs(f.p - (c.p - c.p[0, 0]))) <= 1e-13
    assert f.p[0, 0] == 0.0


@pytest.mark.parametrize("coarse,fine", PAIRS)
@pytest.mark.parametrize("lid", ["none", "saad"])
def test_pinned_cell_and_fluxes(coarse, fine, lid):
    c, f = _pair(coarse, fine, lid, seed=3)
    P.prolong(c, f)
    assert f.p[0, 0] == 0.0 and np.all(np.isfinite(f.p))
    for wall in (f.fx[:, 0], f.fx[:, -1], f.fy[0, :], f.fy[-1, :]):
        assert np.all(wall == 0.0) and not np.any(np.signbit(wall))
    ux, vy = f.faces(f.u, f.v)
    assert np.array_equal(f.fx[:, 1:-1], (f.rho * ux * f.dy)[:, 1:-1])
    assert np.array_equal(f.fy[1:-1, :], (f.rho * vy * f.dx)[1:-1, :])
    assert P.mdot(f).size == f.ny * (f.nx + 1) + (f.ny + 1) * f.nx


@pytest.mark.parametrize("lid", ["none", "saad"])
def test_the_ring_carries_the_lid_profile_and_the_walls(lid):
    """Coarse u = 0: the fine row under the lid is the lid profile times its weight in y, not 0; coarse u = 1 with a
    lid at rest: the rows and columns next to the walls interpolate towards 0."""
    c, f = _pair((8, 8), (16, 16), lid)
    c.u[:] = 0.0
    P.prolong(c, f)
    kx, tx = P.locate(8, c.dx, 16, f.dx)
    top = np.concatenate([[0.0], c.ulid, [0.0]])
    want = 0.5 * (top[kx] + tx * (top[kx + 1] - top[kx]))        # y = 1 - 1/32 lies half way between 1 - 1/16 and 1
    assert np.allclose(f.u[-1], want, rtol=0, atol=1e-15) and np.all(f.u[-1, 1:-1] > 0)
    assert np.all(f.u[:-1] == 0.0)
    c.u[:] = 1.0
    c.ulid[:] = 0.0
    P.prolong(c, f)
    assert np.allclose(f.u[0, 4:12], 0.5) and np.allclose(f.u[-1, 4:12], 0.5) and np.allclose(f.u[4:12, 0], 0.5)
    assert np.allclose(f.u[0, 0], 0.25) and np.allclose(f.u[4:12, 4:12], 1.0)


def test_v_on_the_lid_is_zero():
    c, f = _pair((8, 8), (16, 16))
    c.v[:] = 1.0
    P.prolong(c, f)
    assert np.allclose(f.v[-1, 4:12], 0.5) and np.allclose(f.v[0, 4:12], 0.5)


def test_hierarchy_rule():
    from solvers.fv.fsg import hierarchy_sizes
    for rule in (hierarchy_sizes, P.hierarchy):
        sq = lambda n, levels, coarsest=16: [a for a, _ in rule(n, n, levels, coarsest)]        # noqa: E731
        assert sq(64, 3) == [16, 32, 64]
        assert sq(40, 3) == [20, 40]
        assert rule(48, 20, 2, 16) == [(48, 20)]
        assert sq(37, 2) == [18, 37] and sq(37, 3) == [18, 37]
        assert sq(64, 1) == [64] and sq(64, 2) == [32, 64]
        assert sq(32, 5, 4) == [8, 16, 32]                      # never below the kernel's smallest grid (8)
        assert rule(64, 32, 3, 16) == [(32, 16), (64, 32)]


# ------------------------------------------------------------------------------------------- parameters, configuration
FV_NODE = {"_target_": "solvers.fv.solver.FVSolver", "name": "fv", "Re": 100, "lid_velocity": 1.0, "Lx": 1.0,
           "Ly": 1.0, "nx": 32, "ny": 32, "tolerance": 1e-6, "max_iterations": 10000000,
           "convection_scheme": "TVD", "limiter": "MUSCL", "alpha_uv": 0.4, "alpha_p": 0.2,
           "linear_solver_tol": 1e-9, "corner_treatment": "none", "corner_smoothing": 0.15}


def test_parameter_surface():
    from solvers.datastructures import FVFSGParameters, FVParameters
    p = FVFSGParameters()
    assert (p.n_levels, p.coarsest_n, p.coarse_tolerance_factor) == (2, 16, 1.0)
    assert isinstance(p, FVParameters)
    ml = p.to_mlflow()
    assert ml["n_levels"] == 2 and ml["coarsest_n"] == 16 and ml["coarse_tolerance_factor"] == 1.0
    assert set(ml) == set(FVParameters().to_mlflow()) | {"n_levels", "coarsest_n", "coarse_tolerance_factor"}
    from solvers.fv.fsg import FVFSGSolver
    from solvers.fv.solver import FVSolver
    assert issubclass(FVFSGSolver, FVSolver) and FVFSGSolver.Parameters is FVFSGParameters
    with pytest.raises(TypeError):
        FVParameters(n_levels=2)                  # solver=fv does not take the sequencing keys


def test_fv_fsg_composes_and_fv_is_unchanged():
    from utilities.config import compose as Cmp
    comp = Cmp.Composer(PKG / "conf")
    fv = Cmp.resolve(Cmp.compose_job(comp, ["solver=fv", "N=32", "Re=100", "tolerance=1e-6"], []))["solver"]
    assert fv == FV_NODE
    fsg = Cmp.resolve(Cmp.compose_job(comp, ["solver=fv/fsg", "N=32", "Re=100", "tolerance=1e-6"], []))["solver"]
    assert fsg == dict(FV_NODE, _target_="solvers.fv.fsg.FVFSGSolver", name="fv_fsg", n_levels=2, coarsest_n=16,
                       coarse_tolerance_factor=1.0)
    three = Cmp.resolve(Cmp.compose_job(comp, ["solver=fv/fsg", "N=64", "solver.n_levels=3"], []))["solver"]
    assert three["n_levels"] == 3 and three["nx"] == 64


def test_launcher_batches_sequenced_trials_apart():
    sys.path.insert(0, str(PKG))
    import main as M
    cfg = lambda target, n: dict(N=n, solver=dict(_target_=target))        # noqa: E731
    assert M.batch_key(cfg(M.FV, 32)) == (M.FV,)
    assert M.batch_key(cfg(M.FV_FSG, 32)) == M.batch_key(cfg(M.FV_FSG, 64)) == (M.FV_FSG,)
    assert M.batch_sizes((M.FV_FSG,), 300, 64, False) == [256, 44] == M.batch_sizes((M.FV,), 300, 64, False)
    assert M.batch_sizes((M.FV_FSG,), 1, 64, False) == []


# ------------------------------------------------------------------------------------------- C ABI
@pytest.fixture(scope="module")
def fvlib():
    import __graft_entry__ as g
    g.build()
    from solvers.fv import ldc_fv_lib
    return ldc_fv_lib


def test_prolong_entry_is_declared_exported_and_bound(fvlib):
    hdr = (ROOT / "include" / "ldc_fv.h").read_text()
    assert "ldc_fv_prolong_enqueue" in fvlib.EXPORTS
    assert re.search(r"int ldc_fv_prolong_enqueue\(ldc_fv \*const \*coarse, ldc_fv \*const \*fine, int n, void \*stream\);", hdr)
    L = fvlib.lib()
    assert L.ldc_fv_prolong_enqueue.restype is C.c_int
    val = lambda name: int(re.search(rf"#define {name} (\d+)", hdr).group(1))        # noqa: E731
    assert L.ldc_fv_version() == fvlib.VERSION == val("LDC_FV_VERSION")
    assert fvlib.PROLONG_LAUNCH_MAX == val("LDC_FV_PROLONG_LAUNCH_MAX") <= fvlib.LAUNCH_MAX == val("LDC_FV_LAUNCH_MAX")
    assert 2 * 8 * fvlib.PROLONG_LAUNCH_MAX <= 3600              # both descriptor lists travel as kernel arguments


def test_prolong_argument_validation_needs_no_device(fvlib):
    L = fvlib.lib()
    fake = 8                                                     # never dereferenced: these checks come first
    hs = (C.c_void_p * 2)(fake, fake)
    assert L.ldc_fv_prolong_enqueue(None, hs, 1, None) == -1
    assert L.ldc_fv_prolong_enqueue(hs, None, 1, None) == -1
    assert L.ldc_fv_prolong_enqueue(hs, hs, 0, None) == -1
    assert L.ldc_fv_prolong_enqueue(hs, hs, -2, None) == -1
    null_second = (C.c_void_p * 2)(fake, None)
    assert L.ldc_fv_prolong_enqueue(null_second, hs, 2, None) == -2        # a NULL handle: LDC_E_STATE
    assert L.ldc_fv_prolong_enqueue(hs, null_second, 2, None) == -2
    with pytest.raises(ValueError):
        fvlib.prolong_enqueue([fake], [fake, fake], None)


# ------------------------------------------------------------------------------------------- the sequenced solve
@pytest.fixture(scope="module")
def runs():
    """16^2 -> 32^2 and 32^2 from rest on the restatement: Re = 100, TVD, the YAML's relaxation, tolerance 1e-6."""
    make = lambda nx, ny: FVState(nx, ny, 100.0)        # noqa: E731
    lone = make(32, 32)
    lone_rows = lone.run(20000, tol=1e-6)
    states, rows = P.sequenced_run(make, P.hierarchy(32, 32, 2, 16), 1e-6)
    return lone, lone_rows, states, rows


def test_sequenced_solve_reaches_its_latch_with_a_short_lead_in(runs):
    lone, lone_rows, states, rows = runs
    print("iterations: lone", len(lone_rows), "sequenced", [len(r) for r in rows], "first fine row", rows[1][0][0])
    assert [(s.nx, s.ny) for s in states] == [(16, 16), (32, 32)]
    for r in rows + [lone_rows]:
        assert 10 < len(r) < 20000 and r[-1][0] < 1e-6 and np.all(np.isfinite(r))
    assert rows[1][0][0] < 0.1                                   # (1.5e-2; from rest the first row is 1e12: |u0| = 0)
    assert lone_rows[0][0] > 1.0


def test_sequenced_and_lone_fields_differ_by_the_stored_figures(runs):
    """The bound of tests/test_gpu_fv_fsg.py: both runs stop on a rate-bound rule, so they end a few 1e-4 apart."""
    lone, _, states, _ = runs
    f = states[-1]
    duv = max(float(np.max(np.abs(f.u - lone.u))), float(np.max(np.abs(f.v - lone.v))))
    dp = float(np.max(np.abs(f.p - lone.p)))
    print("max |du|, |dv|:", duv, " max |dp|:", dp)
    assert abs(duv / P.SEQ_16_32_DUV - 1) < 0.05 and abs(dp / P.SEQ_16_32_DP - 1) < 0.05
