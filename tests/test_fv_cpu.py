"""Finite-volume solver, CPU side: the NumPy restatement of the SIMPLE step against the reference's fixtures (g14, and
g15 at odd sizes, Lx != Ly and lid_velocity != 1), its pressure solve against a long-double one, the C ABI of
include/ldc_fv.h without a device, the plugin class, the configuration and the linear Ghia metric."""
import ctypes as C
import json
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"
sys.path.insert(0, str(Path(__file__).resolve().parent))
import fv_numpy  # noqa: E402
from fv_numpy import FVState  # noqa: E402

from conftest import PKG  # noqa: E402


def _state(m, **kw):
    return FVState(m["nx"], m["ny"], m["Re"], corner_treatment=m.get("lid", "none"), alpha_uv=m["alpha_uv"],
                   alpha_p=m["alpha_p"], linear_solver_tol=m["linear_solver_tol"],
                   convection_scheme=m["convection_scheme"], Lx=m.get("Lx", 1.0), Ly=m.get("Ly", 1.0),
                   lid_velocity=m.get("lid_velocity", 1.0), **kw)


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


@pytest.mark.parametrize("tag", ["N16", "12x20"])
def test_restatement_step_matches_reference_intermediates(tag):
    g = np.load(GOLD / "g14_fv_step.npz")
    m = json.loads((GOLD / "g14_fv_step.json").read_text())[tag]
    s = _state(m)
    s.set_state(g[f"{tag}_u0"], g[f"{tag}_v0"], g[f"{tag}_p0"], g[f"{tag}_mdot0"])
    cap = {}
    s.step(cap)
    for k, v in cap.items():
        assert _rel(v, g[f"{tag}_{k}"]) <= 1e-10, k
    for k in ("u", "v", "p"):
        assert _rel(getattr(s, k).ravel(), g[f"{tag}_{k}"]) <= 1e-10, k


def test_restatement_trajectories_match_reference():
    g = np.load(GOLD / "g14_fv_traj.npz")
    meta = json.loads((GOLD / "g14_fv_traj.json").read_text())
    assert len(meta) == 7 and any(m["nx"] != m["ny"] for m in meta.values())
    for tag, m in meta.items():
        if m["nx"] * m["ny"] > 32 * 32:
            continue                            # the N = 48 runs are checked on the GPU
        s = _state(m)
        rec = s.run(m["K"])
        ref = g[f"{tag}_rec"]
        assert rec.shape == ref.shape
        assert np.max(np.abs(rec[:, :7] - ref[:, :7]) / np.abs(ref[:, :7])) <= 1e-9, tag
        for k in ("u", "v", "p"):
            assert _rel(getattr(s, k).ravel(), g[f"{tag}_{k}"]) <= 1e-9, (tag, k)
        assert _rel(np.concatenate([s.fx.ravel(), s.fy.ravel()]), g[f"{tag}_mdot"]) <= 1e-9, tag


def test_pressure_correction_solves_the_pinned_system():
    """x = y - y_0 with y = L^+ c satisfies the reference's matrix (row and column 0 replaced by the identity)."""
    nx, ny = 12, 9
    s = FVState(nx, ny, 100.0, Lx=1.0, Ly=0.7)
    rng = np.random.default_rng(3)
    b = rng.normal(size=(ny, nx))
    b.flat[0] = 0.0
    x = s.pressure_solve(b)
    ax, ay = s.dy / s.dx, s.dx / s.dy
    A = np.zeros((nx * ny, nx * ny))
    for j in range(ny):
        for i in range(nx):
            c = j * nx + i
            for di, dj, g in ((1, 0, ax), (0, 1, ay)):
                if i + di < nx and j + dj < ny:
                    o = (j + dj) * nx + i + di
                    A[c, c] += g; A[o, o] += g; A[c, o] -= g; A[o, c] -= g
    A[0, :] = 0.0
    A[:, 0] = 0.0
    A[0, 0] = 1.0
    assert np.max(np.abs(A @ x.ravel() - b.ravel())) < 1e-11 * np.max(np.abs(b))


# ------------------------------------------------------------------------------------------- g15: odd sizes
@pytest.mark.parametrize("tag", ["13x17", "37x50"])
def test_restatement_step_matches_reference_at_odd_sizes(tag):
    """13 x 17 and 37 x 50 cells on a 2 x 0.5 cavity with lid speed 2 (g15_fv_step), bounds of the g14 test."""
    g = np.load(GOLD / "g15_fv_step.npz")
    m = json.loads((GOLD / "g15_fv_step.json").read_text())[tag]
    s = _state(m)
    s.set_state(g[f"{tag}_u0"], g[f"{tag}_v0"], g[f"{tag}_p0"], g[f"{tag}_mdot0"])
    cap = {}
    s.step(cap)
    for k, v in cap.items():
        assert _rel(v, g[f"{tag}_{k}"]) <= 1e-10, k
    for k in ("u", "v", "p"):
        assert _rel(getattr(s, k).ravel(), g[f"{tag}_{k}"]) <= 1e-10, k


def test_restatement_trajectories_match_reference_at_odd_sizes():
    g = np.load(GOLD / "g15_fv_traj.npz")
    meta = json.loads((GOLD / "g15_fv_traj.json").read_text())
    assert sorted((m["nx"], m["ny"], m["K"]) for m in meta.values()) == \
        [(8, 67, 30), (9, 30, 30), (13, 17, 40), (37, 50, 25)]
    wide = [m for m in meta.values() if m["nx"] == 37][0]
    assert (wide["Lx"], wide["Ly"], wide["lid_velocity"], wide["lid"]) == (2.0, 0.5, 2.0, "smoothing")
    for tag, m in meta.items():
        s = _state(m)
        rec = s.run(m["K"])
        ref = g[f"{tag}_rec"]
        assert rec.shape == ref.shape
        assert np.max(np.abs(rec[:, :7] - ref[:, :7]) / np.abs(ref[:, :7])) <= 1e-9, tag
        for k in ("u", "v", "p"):
            assert _rel(getattr(s, k).ravel(), g[f"{tag}_{k}"]) <= 1e-9, (tag, k)
        assert _rel(np.concatenate([s.fx.ravel(), s.fy.ravel()]), g[f"{tag}_mdot"]) <= 1e-9, tag
        assert "cap" not in s.exits and len(s.exits) == len(s.iters) == 2 * m["K"]


def test_restatement_stops_where_the_reference_stops():
    """The reference's own solve() at 13 x 17, Re 100, tolerance 1e-4 (g15_fv_converged): the same iteration count.
    rel at the stop and at the iteration before are 9.5e-4 and 7.7e-3 (relative) away from the tolerance, the
    restatement follows the reference to 1e-9, so rounding cannot move the count."""
    meta = json.loads((GOLD / "g15_fv_converged.json").read_text())
    g = np.load(GOLD / "g15_fv_converged.npz")
    assert min(meta["margins"].values()) >= 1e-4
    s = _state(meta)
    rec = s.run(5000, tol=meta["tolerance"])
    assert len(rec) == meta["metrics"]["iterations"] == 280 and meta["metrics"]["converged"]
    assert _rel(rec[10:, 0], g["ts_rel_iter_residual"]) <= 1e-9
    for k in ("u", "v", "p"):
        assert _rel(getattr(s, k).ravel(), g[k]) <= 1e-9, k


@pytest.mark.parametrize("lid", ["none", "saad", "smoothing"])
def test_lid_profiles_match_the_reference_mesh(lid):
    """The reference mesh builder's lid-face velocities at nx = 13, Lx = 2, lid_velocity = 2 (g15_fv_lid)."""
    from solvers.fv.solver import lid_profile
    m = json.loads((GOLD / "g15_fv_lid.json").read_text())
    ref = np.load(GOLD / "g15_fv_lid.npz")[lid]
    assert ref.shape == (m["nx"],) and ref.max() <= m["lid_velocity"]
    if lid != "none":
        assert 0 < ref[0] < 0.5 * m["lid_velocity"] and np.unique(np.round(ref, 12)).size > 2       # a real profile
    for fn in (lid_profile, fv_numpy.lid_profile):
        got = fn(m["nx"], m["Lx"], m["lid_velocity"], lid, m["corner_smoothing"])
        assert np.max(np.abs(got - ref)) <= 1e-15, fn.__module__


# the pinned pressure correction in long double (also used by tests/test_gpu_fv_edges.py on the kernel's rhs_p)
LD = np.longdouble


def ld_pressure_solve(b, dx, dy):
    """The pinned 5-point Neumann system of ``FVState.pressure_solve`` solved in np.longdouble with the ANALYTIC
    eigenpairs of the 1-D Neumann second difference: q_k(j) ~ cos(pi k (j + 1/2) / n), lambda_k = 2 - 2 cos(pi k / n).
    ``b``: (ny, nx) with b[0, 0] = 0; returns x with x[0, 0] = 0."""
    ny, nx = b.shape
    pi = np.arccos(LD(-1))

    def basis(n):
        k = np.arange(n, dtype=LD)[None, :]
        j = np.arange(n, dtype=LD)[:, None] + LD(0.5)
        Q = np.cos(pi * k * j / LD(n))
        Q /= np.sqrt((Q * Q).sum(0))[None, :]
        return 2 - 2 * np.cos(pi * np.arange(n, dtype=LD) / LD(n)), Q
    lx, Qx = basis(nx)
    ly, Qy = basis(ny)
    c = b.astype(LD)
    c.flat[0] = -c.ravel()[1:].sum()
    ax, ay = LD(dy) / LD(dx), LD(dx) / LD(dy)
    den = ax * lx[None, :] + ay * ly[:, None]
    den[0, 0] = 1
    h = Qy.T @ c @ Qx / den
    h[0, 0] = 0
    y = Qy @ h @ Qx.T
    return y - y.flat[0]


def ld_pinned_residual(x, b, dx, dy):
    """max |A x - b| over the cells other than the pinned one, relative to max |b|, in long double (x_0 = 0)."""
    x = x.astype(LD)
    ax, ay = LD(dy) / LD(dx), LD(dx) / LD(dy)
    r = np.zeros_like(x)
    r[:, :-1] += ax * (x[:, :-1] - x[:, 1:])
    r[:, 1:] += ax * (x[:, 1:] - x[:, :-1])
    r[:-1, :] += ay * (x[:-1, :] - x[1:, :])
    r[1:, :] += ay * (x[1:, :] - x[:-1, :])
    return float(np.max(np.abs(r - b.astype(LD)).ravel()[1:]) / np.max(np.abs(b)))


PRESSURE_GRIDS = [(13, 17, {}), (37, 50, dict(Lx=2.0, Ly=0.5)), (9, 250, {}), (256, 8, {}), (255, 253, {})]


@pytest.mark.parametrize("nx,ny,kw", PRESSURE_GRIDS, ids=[f"{a}x{b}" for a, b, _ in PRESSURE_GRIDS])
def test_pressure_solve_against_long_double(nx, ny, kw):
    """``FVState.pressure_solve`` (numpy eigh eigenvectors, four fp64 products) against the long-double solve of the
    same right-hand side, a seeded normal field.  The long-double solution must itself satisfy the pinned 5-point
    system to 1e-14 of max |b| (measured: 3.3e-18, 3.3e-17, 2.3e-16, 1.3e-15, 8.8e-16 in the order of the grids).

    Bound on max |x64 - x_ld| / max |x_ld|: 4 eps kappa, kappa the ratio of the largest to the smallest non-zero
    eigenvalue ax lamx + ay lamy of the pinned operator -- the forward error of a backward-stable solve is c eps kappa,
    and each of the four products with an orthogonal factor (computed to about eps itself) may add one eps kappa after
    the division by the eigenvalues.  Measured: 9.3e-15, 1.8e-12, 7.0e-13, 8.1e-13, 5.7e-13, which is 0.23, 0.48,
    0.12, 0.14 and 0.05 of eps kappa (kappa = 1.8e2, 1.7e4, 2.6e4, 2.7e4, 5.2e4)."""
    assert np.finfo(LD).eps < 1.1e-19                     # x87 extended precision or better
    s = FVState(nx, ny, 400.0, **kw)
    b = np.random.default_rng(nx * 1000 + ny).normal(size=(ny, nx))
    b.flat[0] = 0.0
    x_ld = ld_pressure_solve(b, s.dx, s.dy)
    assert x_ld.flat[0] == 0
    res = ld_pinned_residual(x_ld, b, s.dx, s.dy)
    x64 = s.pressure_solve(b)
    dev = float(np.max(np.abs(x64 - x_ld)) / np.max(np.abs(x_ld)))
    print(f"{nx}x{ny} {kw}: long-double residual {res:.2e}, fp64 against long double {dev:.2e}")
    assert res < 1e-14
    den = (s.dy / s.dx) * s.lamx[None, :] + (s.dx / s.dy) * s.lamy[:, None]
    kappa = den.max() / np.sort(den.ravel())[1]
    assert dev <= 4 * np.finfo(float).eps * kappa


# ------------------------------------------------------------------------------------------- C ABI
@pytest.fixture(scope="module")
def fvlib():
    import __graft_entry__ as g
    g.build()
    from solvers.fv import ldc_fv_lib
    return ldc_fv_lib


def test_header_and_exports_agree(fvlib):
    hdr = (ROOT / "include" / "ldc_fv.h").read_text()
    declared = set(re.findall(r"\b(ldc_fv_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(fvlib.EXPORTS)
    L = fvlib.lib()
    for name in declared:
        assert hasattr(L, name), name
    assert L.ldc_fv_version() == fvlib.VERSION == int(re.search(r"#define LDC_FV_VERSION (\d+)", hdr).group(1))
    val = lambda name: int(re.search(rf"#define {name} \(?(-?\d+)", hdr).group(1))        # noqa: E731
    assert (val("LDC_FV_MIN_N"), val("LDC_FV_MAX_N")) == (fvlib.MIN_N, fvlib.MAX_N)
    assert (val("LDC_FV_REC_LEN"), val("LDC_FV_CTRL_LEN")) == (fvlib.REC_LEN, fvlib.CTRL_LEN)
    assert (val("LDC_FV_NWORK"), val("LDC_FV_DESC_DOUBLES")) == (fvlib.NWORK, fvlib.DESC_DOUBLES)
    assert (val("LDC_FV_LAUNCH_MAX"), val("LDC_FV_E_NAN"), val("LDC_FV_DBG_COUNT")) == \
        (fvlib.LAUNCH_MAX, fvlib.E_NAN, len(fvlib.DBG))
    # 6 int32 + 9 double + 12 pointers
    assert C.sizeof(fvlib.Problem) == 24 + 72 + 96


def test_argument_validation_needs_no_device(fvlib):
    L = fvlib.lib()
    h = C.c_void_p()
    assert L.ldc_fv_create(None, C.byref(h)) == -1
    fake = 8                                                     # never dereferenced: validation comes first
    good = dict(nx=16, ny=16, scheme=1, rec_cap=4, warmup=10, max_lin_iters=1000, dx=1 / 16, dy=1 / 16, rho=1.0,
                mu=0.01, alpha_uv=0.4, alpha_p=0.2, lin_tol=1e-9, tol=1e-6, lid_velocity=1.0,
                **{k: fake for k in ("ulid", "Qx", "lamx", "Qy", "lamy", "u", "v", "p", "mdot", "work", "rec", "ctrl")})
    bad = [dict(nx=7), dict(ny=257), dict(scheme=2), dict(rec_cap=0), dict(max_lin_iters=0), dict(dx=0.0),
           dict(mu=-1.0), dict(alpha_uv=0.0), dict(alpha_p=1.5), dict(lin_tol=0.0), dict(work=None), dict(ctrl=None)]
    for change in bad:
        pr = fvlib.Problem(**dict(good, **change))
        assert L.ldc_fv_create(C.byref(pr), C.byref(h)) == -1, change
        assert not h.value
    assert L.ldc_fv_create(C.byref(fvlib.Problem(**good)), None) == -1
    for rc in (L.ldc_fv_destroy(None), L.ldc_fv_enqueue(None, 1, None), L.ldc_fv_status(None),
               L.ldc_fv_step_debug(None, 0, None, None)):
        assert rc == -2
    assert L.ldc_fv_batch_enqueue(None, 1, 1, None) == -1
    arr = (C.c_void_p * 1)(None)
    assert L.ldc_fv_batch_enqueue(arr, 0, 1, None) == -1
    assert L.ldc_fv_batch_enqueue(arr, 1, 1, None) == -2


def test_solver_imports_and_refuses_to_run_without_a_gpu(monkeypatch):
    import torch
    from solvers.fv.solver import FVSolver
    from solvers.datastructures import FVParameters
    from solvers.spectral import ldc_lib
    assert FVSolver.Parameters is FVParameters
    p = FVParameters()
    assert (p.convection_scheme, p.limiter, p.alpha_uv, p.alpha_p, p.linear_solver_tol, p.method) == \
        ("Upwind", "MUSCL", 0.6, 0.4, 1e-6, "FV-SIMPLE")
    assert "device" not in p.to_mlflow() and "check_every" not in p.to_mlflow()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(ldc_lib.LdcError, match="no CPU fallback"):
        FVSolver(name="fv", Re=100.0, nx=16, ny=16)
    with pytest.raises(ValueError):
        FVSolver(name="fv", Re=100.0, nx=4, ny=16)
    with pytest.raises(TypeError):
        FVSolver(name="fv", Re=100.0, nx=16, ny=16, not_a_key=1)


def test_configs_compose_to_the_reference_node():
    from utilities.config import compose as Cmp
    comp = Cmp.Composer(PKG / "conf")
    ref = {"_target_": "solvers.fv.solver.FVSolver", "name": "fv", "Re": 1000, "lid_velocity": 1.0, "Lx": 1.0,
           "Ly": 1.0, "nx": 128, "ny": 128, "tolerance": 1e-6, "max_iterations": 10000000,
           "convection_scheme": "TVD", "limiter": "MUSCL", "alpha_uv": 0.4, "alpha_p": 0.2,
           "linear_solver_tol": 1e-9, "corner_treatment": "none", "corner_smoothing": 0.15}
    cfg = Cmp.resolve(Cmp.compose_job(comp, ["solver=fv", "N=128", "Re=1000"], []))
    assert cfg["solver"] == ref
    job = Cmp.resolve(Cmp.compose_job(comp, ["+experiment/validation/ghia=fv"], [("N", 128), ("Re", 1000)]))
    assert job["solver"] == ref and job["experiment_name"] == "LDC-GHIA-PLOTS"
    default = Cmp.resolve(Cmp.compose_job(comp, [], []))
    assert default["solver"]["_target_"] == "solvers.spectral.sg.SGSolver"


def test_linear_ghia_interpolation_on_an_analytic_field():
    from solvers import validation as V
    (yu, ug), (xv, vg) = V.load_ghia(100)
    n = 64
    xc = (np.arange(n) + 0.5) / n
    # fields linear in the interpolation direction are reproduced exactly inside the node range
    U = np.tile(0.3 + 0.5 * xc, (n, 1))            # [ix, iy]: u = 0.3 + 0.5 y
    Vf = np.tile((0.2 - 0.4 * xc)[:, None], (1, n))  # v = 0.2 - 0.4 x
    e = V.ghia_centerline_error(xc, xc, U, Vf, 100, interpolation="linear")
    inside_u = (yu >= xc[0]) & (yu <= xc[-1])
    eu = np.where(inside_u, 0.3 + 0.5 * yu, 0.3 + 0.5 * np.clip(yu, xc[0], xc[-1])) - ug
    ev = 0.2 - 0.4 * np.clip(xv, xc[0], xc[-1]) - vg
    assert e["u_rms"] == pytest.approx(np.sqrt(np.mean(eu**2)), rel=1e-12)
    assert e["v_max"] == pytest.approx(np.max(np.abs(ev)), rel=1e-12)
    assert e != V.ghia_centerline_error(xc, xc, U, Vf, 100)                  # the default stays Legendre
    with pytest.raises(ValueError):
        V.ghia_centerline_error(xc, xc, U, Vf, 100, interpolation="cubic")


def test_trial_cost_has_an_fv_branch():
    from utilities.sweep import farm
    a = farm.trial_cost(dict(N=64, Re=100), solver="solvers.fv.solver.FVSolver")
    b = farm.trial_cost(dict(N=128, Re=100), solver="solvers.fv.solver.FVSolver")
    assert 0 < a < b
    assert farm.trial_cost(dict(N=64, Re=100), solver="solvers.spectral.sg.SGSolver") == farm.trial_cost(dict(N=64, Re=100))
