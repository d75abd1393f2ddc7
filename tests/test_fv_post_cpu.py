"""Finite-volume post-processing, CPU side: the analytic sine eigenvectors, the NumPy restatement of the device's
streamfunction solve against the solver's sparse solve and against long double, the extrema rule against the host code
path, the C ABI of ldc_fv_post_enqueue without a device, the ``vortex_metrics`` parameter and its configuration."""
import ctypes as C
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import fv_post_numpy as P  # noqa: E402
from fv_post_numpy import EPS, LD  # noqa: E402

from conftest import PKG  # noqa: E402


@pytest.mark.parametrize("m", [6, 15, 16, 17, 254])
def test_sine_eigenvectors_are_orthonormal(m):
    """S^T S = I within 8 m eps entrywise (m-term dot products of entries <= 1, a margin of 8), and T S = S diag(lam)."""
    from solvers.fv.solver import sine_eig
    lam, S = sine_eig(m)
    assert S.shape == (m, m) and lam.shape == (m,) and np.all(np.diff(lam) > 0)
    worst = float(np.max(np.abs(S.T @ S - np.eye(m))))
    print(f"m={m}: max |S^T S - I| = {worst:.2e} = {worst / (m * EPS):.2f} m eps")
    assert worst <= 8 * m * EPS
    T = 2 * np.eye(m) - np.eye(m, k=1) - np.eye(m, k=-1)
    assert np.max(np.abs(T @ S - S * lam[None, :])) <= 8 * m * EPS * 4
    lam2, S2 = P.sine_basis(m)
    assert np.array_equal(lam, lam2) and np.array_equal(S, S2)


@pytest.mark.parametrize("shape", [(8, 8, 1.0, 1.0), (13, 17, 1.0, 1.0), (37, 50, 2.0, 0.5), (64, 40, 1.0, 1.0)], ids=P.shape_id)
def test_restatement_agrees_with_the_sparse_solve(shape):
    """``psi_solve`` against ``FVSolver._streamfunction`` (called unbound on a namespace with shape_full, dx_min, dy_min)
    within 8 eps kappa max|psi|: each side is within 4 eps kappa of the exact solution (the table of the next test)."""
    from solvers.fv.solver import FVSolver
    nx, ny, Lx, Ly = shape
    ns = SimpleNamespace(shape_full=(ny, nx), dx_min=Lx / nx, dy_min=Ly / ny)
    omega = np.random.default_rng(nx * 1000 + ny).normal(size=(ny, nx))
    ref = FVSolver._streamfunction(ns, omega)
    got = P.psi_solve(omega, ns.dx_min, ns.dy_min)
    err = float(np.max(np.abs(got - ref)))
    bound = 8 * EPS * P.kappa(nx, ny, ns.dx_min, ns.dy_min) * float(np.max(np.abs(ref)))
    print(f"{nx}x{ny}: max |fast-diag - spsolve| = {err:.2e}, bound {bound:.2e}")
    assert err <= bound
    for ring in (got[0], got[-1], got[:, 0], got[:, -1]):
        assert np.all(ring == 0.0)


@pytest.mark.parametrize("shape", P.TABLE_SHAPES, ids=P.shape_id)
def test_restatement_against_long_double(shape):
    """fp64 fast diagonalisation against the long-double evaluation of the same formula, for a normal random omega:
    within 4 eps kappa max|psi| (the factor ``test_pressure_solve_against_long_double`` allows the analogous pressure
    solve).  The long-double solution must satisfy the 5-point system to 1e-14 of max|omega|."""
    assert np.finfo(LD).eps < 1.1e-19
    nx, ny, Lx, Ly = shape
    dx, dy = Lx / nx, Ly / ny
    omega = np.random.default_rng(nx * 1000 + ny).normal(size=(ny, nx))
    ld = P.psi_solve(omega, dx, dy, LD)
    cx, cy = LD(1) / (LD(dx) * LD(dx)), LD(1) / (LD(dy) * LD(dy))
    lap = cx * (2 * ld[1:-1, 1:-1] - ld[1:-1, :-2] - ld[1:-1, 2:]) + cy * (2 * ld[1:-1, 1:-1] - ld[:-2, 1:-1] - ld[2:, 1:-1])
    res = float(np.max(np.abs(lap - omega[1:-1, 1:-1].astype(LD))) / np.max(np.abs(omega)))
    err = float(np.max(np.abs(P.psi_solve(omega, dx, dy).astype(LD) - ld)))
    k = P.kappa(nx, ny, dx, dy)
    share = err / (EPS * k * float(np.max(np.abs(ld))))
    print(f"{nx}x{ny}: kappa {k:.2e}, long-double residual {res:.2e}, share of eps kappa max|psi| {share:.3f}")
    assert res < 1e-14
    assert share <= 4


def _tie_arrays():
    """8 x 10 cells with every extremum attained twice, the later copy first in memory order only for one of them."""
    nx, ny = 8, 10
    psi = np.zeros((ny, nx))
    omega = np.zeros((ny, nx))
    psi[2, 1] = psi[2, 2] = 0.25           # BL twice in one row
    psi[3, 6] = psi[1, 5] = 0.5            # BR twice: the lower row wins
    psi[7, 3] = psi[6, 4] = -1.0           # min psi twice (6, 4 is not in TL: x > 0.5)
    omega[4, 4], omega[8, 2] = -3.0, 3.0   # |omega| twice, signs differ: the first one's sign
    omega[6, 4] = 0.75
    return psi, omega


@pytest.mark.parametrize("case", ["ties", "random", "zero", "negative", "wide"])
def test_extrema_rule_equals_the_host_code_path(case):
    """The NumPy statement of the device's rule (increasing cell order, strict comparisons, masks from index bounds,
    zeros for a corner that is not > 0) gives the dict of ``FVSolver.compute_vortex_metrics`` on the same arrays."""
    Lx = Ly = 1.0
    if case == "ties":
        psi, omega = _tie_arrays()
    elif case == "wide":                   # 2 x 0.5 cavity: the masks are absolute, no cell has y > 0.5
        Lx, Ly = 2.0, 0.5
        rng = np.random.default_rng(5)
        psi, omega = rng.normal(size=(12, 9)), rng.normal(size=(12, 9))
    else:
        rng = np.random.default_rng(4)
        psi, omega = rng.normal(size=(9, 13)), rng.normal(size=(9, 13))
        if case == "zero":
            psi[:] = 0.0
            omega[:] = 0.0
        if case == "negative":
            psi = -np.abs(psi)
    ny, nx = psi.shape
    ns = P.host_namespace(nx, ny, Lx, Ly)
    xs, ys = P.cell_centres(nx, ny, Lx, Ly)
    assert np.array_equal(xs, np.sort(np.unique(ns.fields.x))) and np.array_equal(ys, np.sort(np.unique(ns.fields.y)))
    bounds = P.mask_bounds(xs, ys)
    from solvers.fv.solver import mask_bounds
    assert mask_bounds(xs, ys) == bounds
    ref = P.host_metrics(ns, omega, psi)
    got = P.extrema(psi, omega, bounds, xs, ys)
    assert got == ref
    if case == "ties":
        assert (got["psi_BL_x"], got["psi_BL_y"]) == (xs[1], ys[2]) and (got["psi_BR_x"], got["psi_BR_y"]) == (xs[5], ys[1])
        assert (got["psi_min_x"], got["psi_min_y"], got["omega_center"]) == (xs[4], ys[6], 0.75)
        assert got["omega_max"] == -3.0 and got["psi_TL"] == 0.0
    if case == "wide":
        assert bounds == (2, 2, ny, ny) and got["psi_TL"] == 0.0
    if case in ("zero", "negative"):
        assert got["psi_BR"] == got["psi_BL"] == got["psi_TL"] == 0.0
    if case == "zero":
        assert (got["psi_min_x"], got["psi_min_y"]) == (xs[0], ys[0])


@pytest.mark.parametrize("shape", P.GPU_SHAPES, ids=P.shape_id)
def test_seeded_states_have_clear_extrema(shape):
    """The precondition of the GPU metrics test, on the host path alone: for the seeded states the best and the
    second-best candidate of every extremum differ by more than twice the bound on the field (so no rounding inside the
    bound can move an extremum to another cell)."""
    nx, ny, Lx, Ly = shape
    u, v = P.random_state(nx, ny)
    ns = P.host_namespace(nx, ny, Lx, Ly, u=u, v=v)
    omega, psi = P.host_fields(ns)
    gaps = P.runner_up_gaps(psi, omega, P.mask_bounds(*P.cell_centres(nx, ny, Lx, Ly)))
    bw = P.omega_bound(u, v, 1.0, ns.dx_min, ns.dy_min)
    bp = P.psi_bound(psi, nx, ny, ns.dx_min, ns.dy_min)
    print(f"{nx}x{ny}: bounds omega {bw:.2e} psi {bp:.2e}; gaps", {k: f"{g:.2e}" for k, g in gaps.items()})
    assert gaps["omega_max"] > 2 * bw
    assert all(gaps[k] > 2 * bp for k in ("psi_min", "psi_BR", "psi_BL", "psi_TL"))
    m = P.host_metrics(ns, omega, psi)
    if Ly > 0.5:
        assert min(m["psi_BR"], m["psi_BL"], m["psi_TL"]) > 2 * bp        # no corner near the zero branch


# ------------------------------------------------------------------------------------------- C ABI
@pytest.fixture(scope="module")
def fvlib():
    import __graft_entry__ as g
    g.build()
    from solvers.fv import ldc_fv_lib
    return ldc_fv_lib


def test_post_structure_and_constants_match_the_header(fvlib):
    import re
    hdr = (Path(__file__).resolve().parent.parent / "include" / "ldc_fv.h").read_text()
    val = lambda name: int(re.search(rf"#define {name} (\d+)", hdr).group(1))        # noqa: E731
    assert fvlib.VERSION == val("LDC_FV_VERSION") == 2 and "ldc_fv_post_enqueue" in fvlib.EXPORTS
    assert C.sizeof(fvlib.Post) == 4 * 8 + 4 * 4 + 3 * 8
    assert C.sizeof(fvlib.Problem) == 24 + 72 + 96                                   # the solve's block keeps its size
    names = ["PSI_MIN", "OMEGA_CENTER", "OMEGA_MAX", "PSI_BR", "PSI_BL", "PSI_TL", "PSI_MIN_CELL", "OMEGA_MAX_CELL",
             "PSI_BR_CELL", "PSI_BL_CELL", "PSI_TL_CELL", "NONFINITE", "RESULT_LEN"]
    for n in names:
        assert val(f"LDC_FV_POST_{n}") == getattr(fvlib, f"POST_{n}"), n
    body = re.search(r"struct ldc_fv_post \{(.*?)\};", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\*?(\w+)\s*[,;]", body) == [f[0] for f in fvlib.Post._fields_]


def test_post_argument_validation_needs_no_device(fvlib):
    L = fvlib.lib()
    fake = 8                                                     # never dereferenced: validation comes first
    good = dict(Sx=fake, lamx=fake, Sy=fake, lamy=fake, ix_lt=4, ix_gt=4, jy_lt=4, jy_gt=4, psi=fake, omega=fake,
                result=fake)
    hs = (C.c_void_p * 2)(fake, fake)
    posts = (fvlib.Post * 2)(fvlib.Post(**good), fvlib.Post(**good))
    assert L.ldc_fv_post_enqueue(None, posts, 1, None) == -1
    assert L.ldc_fv_post_enqueue(hs, None, 1, None) == -1
    assert L.ldc_fv_post_enqueue(hs, posts, 0, None) == -1
    assert L.ldc_fv_post_enqueue(hs, posts, -3, None) == -1
    null_second = (C.c_void_p * 2)(fake, None)
    for name in ("Sx", "lamx", "Sy", "lamy", "psi", "omega", "result"):
        bad = (fvlib.Post * 2)(fvlib.Post(**good), fvlib.Post(**dict(good, **{name: None})))
        assert L.ldc_fv_post_enqueue(hs, bad, 2, None) == -1, name
    # a NULL handle: LDC_E_STATE, found before any handle is dereferenced
    assert L.ldc_fv_post_enqueue((C.c_void_p * 2)(None, None), posts, 2, None) == -2
    first_bad = (fvlib.Post * 2)(fvlib.Post(**dict(good, psi=None)), fvlib.Post(**good))
    assert L.ldc_fv_post_enqueue(null_second, first_bad, 2, None) == -1        # in list order: post 0 before handle 1


# ------------------------------------------------------------------------------------------- parameter, configuration
def test_vortex_metrics_parameter(monkeypatch):
    from solvers.datastructures import FVParameters
    from solvers.fv.solver import FVSolver
    monkeypatch.delenv("LDC_FV_VORTEX_METRICS", raising=False)
    p = FVParameters()
    assert p.vortex_metrics == "host"
    assert "vortex_metrics" not in p.to_mlflow() and "device" not in p.to_mlflow() and "check_every" not in p.to_mlflow()
    assert FVParameters(vortex_metrics="device").vortex_metrics == "device"
    monkeypatch.setenv("LDC_FV_VORTEX_METRICS", "device")
    assert FVParameters().vortex_metrics == "device"
    assert FVParameters(vortex_metrics="host").vortex_metrics == "host"          # the keyword wins
    monkeypatch.delenv("LDC_FV_VORTEX_METRICS")
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)               # ValueError comes before the device
    with pytest.raises(ValueError, match="vortex_metrics"):
        FVSolver(name="fv", Re=100.0, nx=16, ny=16, vortex_metrics="gpu")
    monkeypatch.setenv("LDC_FV_VORTEX_METRICS", "gpu")
    with pytest.raises(ValueError, match="vortex_metrics"):
        FVSolver(name="fv", Re=100.0, nx=16, ny=16)


def test_launcher_override_carries_the_key_and_the_default_node_is_unchanged():
    from utilities.config import compose as Cmp
    comp = Cmp.Composer(PKG / "conf")
    base = Cmp.resolve(Cmp.compose_job(comp, ["solver=fv", "N=16"], []))["solver"]
    assert "vortex_metrics" not in base
    dev = Cmp.resolve(Cmp.compose_job(comp, ["solver=fv", "N=16", "+solver.vortex_metrics=device"], []))["solver"]
    assert dev == dict(base, vortex_metrics="device")
