"""What the three stretched-grid kernels of a one-CU finite-volume trial leave in their work vectors after ONE iteration, and
the cases of tests/test_fv_stretched_edges_cpu.py and tests/test_gpu_fv_stretched_edges.py (test helper, no test in it).

The kernels (csrc/ldc_fv_stretched.hip, csrc/ldc_fv_stretched_sep.hip, csrc/ldc_fv_stretched_phases.inc) have no debug
instantiation: ``ldc_fv_step_debug`` refuses a handle with tables.  But every intermediate of ``FVStretchedState.step(capture)``
survives the iteration in a work vector of its own, so ``intermediates(solver, kernel)`` reads ``solver.t["work"]`` after
``solver._advance(1)``.  ``VEC`` follows ``enum FvVec`` (csrc/ldc_fv_common.inc), the ``PCG_*`` aliases
(csrc/ldc_fv_pressure_cells.inc) and ``SEP_S`` (csrc/ldc_fv_stretched_sep.hip); tests/test_fv_stretched_edges_cpu.py pins it
against those three files.

The restatement runs that the GPU tests compare against are made here, once per case (``functools.lru_cache``), and never
changed by a caller: the CPU file asserts their preconditions, the GPU file compares with them.
"""
from __future__ import annotations

import functools
import json
from pathlib import Path

import numpy as np

from fv_separable_numpy import FVSeparableState
from fv_stretched_numpy import FVStretchedState

GOLD = Path(__file__).resolve().parent / "golden"

# ---------------------------------------------------------------------------------------------- the three kernels
KERNELS = ("reference", "laplacian", "separable")
REF = dict(grid="tanh", pressure_equation="reference")
LAP = dict(grid="tanh", pressure_equation="consistent_cu", pressure_preconditioner="laplacian")      # test_gpu_fv_separable.py
SEP = dict(grid="tanh", pressure_equation="consistent_cu", pressure_preconditioner="separable")
SOLVER_MODE = dict(reference=REF, laplacian=LAP, separable=SEP)

# work vectors, by the name of the enumerator that owns them
VEC = dict(grad_p=("FV_GPX", "FV_GPY"), diag=("FV_AP", "FV_AW", "FV_AE", "FV_AS", "FV_AN"), u_star=("FV_XU",),
           v_star=("FV_XV",), mdot_star=("PCG_MS",), cg_r=("PCG_R",), sep_s=("SEP_S",), rhs_p=("FV_C",), p_prime=("FV_Y",),
           u_prime=("FV_UP",), v_prime=("FV_VP",), omega=("FV_OMEGA",), b=("FV_BU", "FV_BV"))
INDEX = dict(FV_GPX=0, FV_GPY=1, FV_AP=2, FV_AW=3, FV_AE=4, FV_AS=5, FV_AN=6, FV_XU=7, FV_XV=8, PCG_MS=9, PCG_R=12, SEP_S=15,
             FV_C=23, FV_Y=26, FV_UP=27, FV_VP=28, FV_OMEGA=29, FV_BU=30, FV_BV=31)
MS_VECTORS = 3                          # mdot* fills PCG_MS and the two vectors behind it (nx (ny + 1) + ny (nx + 1) <= 3 nx ny)

STEP_KEYS = ("grad_p", "diag", "b", "u_star", "v_star", "mdot_star", "rhs_p", "p_prime", "u_prime", "v_prime", "mdot")


def restatement(kernel, nx, ny, Re, **kw):
    """The NumPy restatement of ``kernel``'s trial (tests/fv_stretched_numpy.py, tests/fv_separable_numpy.py)."""
    if kernel == "reference":
        return FVStretchedState(nx, ny, Re, pressure_equation="reference", **kw)
    cls = FVSeparableState if kernel == "separable" else FVStretchedState
    return cls(nx, ny, Re, pressure_equation="consistent", **kw)


def mdot_of(o):
    return np.concatenate([o.fx.ravel(), o.fy.ravel()])


def state_of(o):
    return dict(u=o.u.ravel().copy(), v=o.v.ravel().copy(), p=o.p.ravel().copy(), mdot=mdot_of(o))


def intermediates(solver, kernel):
    """The keys of ``FVStretchedState.step(capture)`` plus ``omega``, read from the work vectors after ``_advance(1)``.

    ``mdot_star`` only with a consistent kernel (the reference kernel updates mdot in place; the vectors hold BiCGSTAB
    leftovers).  ``rhs_p``: entry 0 is 0.0 as a consistent kernel leaves it; the reference kernel keeps b00 there, which comes
    back as ``b00`` with entry 0 of ``rhs_p`` set to 0.0.  ``p_prime`` is y - y[0]; ``y`` is the iterate itself.  The separable
    kernel adds ``sep_s`` (the scaling s) and ``cg_r`` (the last CG residual), the laplacian one ``cg_r``."""
    if kernel not in KERNELS:
        raise ValueError(kernel)
    nx, ny = solver.nx, solver.ny
    n, nf = nx * ny, ny * (nx + 1) + (ny + 1) * nx
    w = solver.t["work"].cpu().numpy()

    def vec(name, count=1):
        k = INDEX[name]
        return w[k * n: (k + count) * n].copy()

    out = {key: np.concatenate([vec(name) for name in VEC[key]]) for key in ("grad_p", "diag", "b", "u_star", "v_star",
                                                                               "u_prime", "v_prime", "omega")}
    rhs = vec("FV_C")
    if kernel == "reference":
        out["b00"] = float(rhs[0])
        rhs[0] = 0.0
    else:
        out["mdot_star"] = vec("PCG_MS", MS_VECTORS)[:nf]
        out["cg_r"] = vec("PCG_R")
    if kernel == "separable":
        out["sep_s"] = vec("SEP_S")
    y = vec("FV_Y")
    out.update(rhs_p=rhs, y=y, p_prime=y - y[0], mdot=solver.t["mdot"].cpu().numpy().copy(),
               row=solver.t["rec"][0].cpu().numpy().copy())
    return out


# ---------------------------------------------------------------------------------------------- a. phases from a seed
PHASE_TAGS = ("13x17", "37x50")
PHASE_TOL = dict(linear_solver_tol=1e-12, pressure_tol=1e-13)
PHASE_MORE = 10                          # iterations after the one that is taken apart


def phase_case(tag):
    """(settings of g17's step fixture ``tag`` with TVD, its seeded state u0, v0, p0, mdot0)."""
    m = dict(json.loads((GOLD / "g17_fv_stretched.json").read_text())[tag], convection_scheme="TVD")
    g = np.load(GOLD / "g17_fv_stretched.npz")
    return m, [g[f"{tag}_{k}0"] for k in ("u", "v", "p", "mdot")]


def phase_geometry(m):
    return dict(Lx=m.get("Lx", 1.0), Ly=m.get("Ly", 1.0), lid_velocity=m.get("lid_velocity", 1.0))


def phase_solver_kwargs(m, kernel):
    return dict(name="fv", Re=m["Re"], nx=m["nx"], ny=m["ny"], corner_treatment=m["lid"], alpha_uv=m["alpha_uv"],
                alpha_p=m["alpha_p"], convection_scheme=m["convection_scheme"], grid_stretch=m["beta"], tolerance=1e-30,
                max_iterations=10**6, check_every=16, **PHASE_TOL, **phase_geometry(m), **SOLVER_MODE[kernel])


@functools.lru_cache(maxsize=None)
def phase_reference(tag, consistent):
    """One ``step(capture)`` of the restatement with the dense pressure solve from the seeded state, then PHASE_MORE more.
    Both consistent kernels solve the same equation, so they share this run (an ``FVSeparableState``: it has ``scaling``).
    A dict: cap, omega, row, state (after the one step), exits, and with ``consistent``: A's smallest positive eigenvalue
    ``lam1``, A itself, b, x* (``xs``), wx, wy, the scaling ``s``; then rows and state_after of the further iterations."""
    m, seed = phase_case(tag)
    o = restatement("separable" if consistent else "reference", m["nx"], m["ny"], m["Re"], corner_treatment=m["lid"],
                    alpha_uv=m["alpha_uv"], alpha_p=m["alpha_p"], linear_solver_tol=PHASE_TOL["linear_solver_tol"],
                    convection_scheme="TVD", grid_stretch=m["beta"], pressure_solver="direct", **phase_geometry(m))
    o.set_state(*seed)
    cap = {}
    row = o.step(cap)
    out = dict(cap=cap, omega=o.vorticity().ravel(), row=row, state=state_of(o))
    if consistent:
        A = o.dense(o.last["wx"], o.last["wy"])
        lam = np.linalg.eigvalsh(A)
        assert abs(lam[0]) <= 1e-12 * lam[-1] and lam[1] > 1e-9 * lam[-1]        # one zero mode: the constants
        D = o.V / (cap["diag"][: o.nx * o.ny].reshape(o.ny, o.nx) + 1e-14)       # D of this step: a_P is diag's first block
        out.update(A=A, lam1=float(lam[1]), b=o.last["b"].copy(), xs=o.last["x"].copy(), wx=o.last["wx"].copy(),
                   wy=o.last["wy"].copy(), s=o.scaling(D).ravel())
    out["rows"] = o.run(PHASE_MORE)
    out["state_after"] = state_of(o)
    out["exits"] = tuple(o.exits)
    return out


# ---------------------------------------------------------------------------------------------- b. edge shapes
# (nx, ny, beta, geometry, K): TVD from rest, Re 400, both tolerances tight, the CG pressure solver
SHAPES = [(37, 50, 1.0, (("Lx", 2.0), ("Ly", 0.5), ("lid_velocity", 2.0)), 12),
          (131, 77, 1.5, (), 6),
          (8, 256, 1.5, (), 6),
          (256, 8, 1.5, (), 6),
          (24, 40, 2.5, (), 12),
          (255, 253, 1.5, (), 3),
          (256, 256, 1.5, (), 3)]
SHAPE_IDS = [f"{nx}x{ny}-beta{beta}" for nx, ny, beta, _, _ in SHAPES]
SHAPE_TOL = dict(linear_solver_tol=1e-12, pressure_tol=1e-13, pressure_max_iters=2000)
SHAPE_RE = 400.0


def shape_solver_kwargs(nx, ny, beta, geo, K, kernel):
    return dict(name="fv", Re=SHAPE_RE, nx=nx, ny=ny, convection_scheme="TVD", alpha_uv=0.4, alpha_p=0.2, grid_stretch=beta,
                tolerance=1e-30, max_iterations=K, check_every=16, **SHAPE_TOL, **dict(geo), **SOLVER_MODE[kernel])


def _trajectory(kernel, nx, ny, Re, K, **kw):
    """(rows, state, exits, cg_iters, cg_caps) of K iterations of the restatement from rest."""
    o = restatement(kernel, nx, ny, Re, **kw)
    rows = o.run(K)
    return dict(rows=rows, state=state_of(o), exits=tuple(o.exits), iters=tuple(o.iters), cg_iters=tuple(o.cg_iters),
                cg_caps=int(o.cg_caps))


@functools.lru_cache(maxsize=None)
def shape_reference(nx, ny, beta, geo, K, kernel):
    """The restatement with the kernel's own pressure solve (CG with the same preconditioner; the exact solve in reference
    mode), once per shape and kernel."""
    return _trajectory(kernel, nx, ny, SHAPE_RE, K, convection_scheme="TVD", grid_stretch=beta, pressure_solver="cg",
                       linear_solver_tol=SHAPE_TOL["linear_solver_tol"], pressure_tol=SHAPE_TOL["pressure_tol"],
                       pressure_max_iters=SHAPE_TOL["pressure_max_iters"], **dict(geo))


# ---------------------------------------------------------------------------------------------- c. CG counts at an edge
# the 24 x 40, beta 2.5 case of the list above, one iteration per launch: about 28 CG iterations per solve with the separable
# preconditioner, 410 to 470 with the laplacian one
COUNTS = SHAPES[4]


def counts_reference(kernel):
    return shape_reference(*COUNTS, kernel)


def counts_solver_kwargs(kernel):
    return shape_solver_kwargs(*COUNTS, kernel)


# How far the restatement's OWN per-solve counts move when its linear_solver_tol goes from 1e-12 to 1e-13: nothing with the
# separable preconditioner (28 iterations), up to 2 with the laplacian one, whose 460 iterations lose conjugacy to rounding long
# before they end (tests/test_fv_stretched_edges_cpu.py measures both).  The card is allowed one (a stop test at the threshold)
# or ten times this figure, whichever is larger.
COUNT_SENSITIVITY = dict(separable=0, laplacian=2)


def count_bound(kernel):
    return max(1, 10 * COUNT_SENSITIVITY[kernel])


@functools.lru_cache(maxsize=None)
def counts_sensitivity(kernel):
    """max over the solves of |count at linear_solver_tol 1e-13 - count at 1e-12| of the restatement."""
    nx, ny, beta, geo, K = COUNTS
    tight = _trajectory(kernel, nx, ny, SHAPE_RE, K, convection_scheme="TVD", grid_stretch=beta, pressure_solver="cg",
                        linear_solver_tol=1e-13, pressure_tol=SHAPE_TOL["pressure_tol"],
                        pressure_max_iters=SHAPE_TOL["pressure_max_iters"], **dict(geo))
    assert tight["cg_caps"] == 0 and "cap" not in tight["exits"]
    return max(abs(a - b) for a, b in zip(tight["cg_iters"], counts_reference(kernel)["cg_iters"]))


# ---------------------------------------------------------------------------------------------- d, e. the exits
SMALL = dict(nx=13, ny=17, beta=1.5, Re=100.0, K=30)
CAPPED_CG = dict(pressure_tol=1e-10, pressure_max_iters=3, linear_solver_tol=1e-12)
CAPPED_LINEAR = dict(max_lin_iters=3, linear_solver_tol=1e-12, pressure_tol=1e-12)
LOOSE = dict(nx=30, ny=21, beta=1.0, Re=400.0, K=40, linear_solver_tol=1e-6, pressure_tol=1e-12)


def small_solver_kwargs(kernel, case=SMALL, **kw):
    return dict(dict(name="fv", Re=case["Re"], nx=case["nx"], ny=case["ny"], convection_scheme="TVD", alpha_uv=0.4, alpha_p=0.2,
                     grid_stretch=case["beta"], tolerance=1e-30, max_iterations=case["K"], check_every=16,
                     **SOLVER_MODE[kernel]), **kw)


@functools.lru_cache(maxsize=None)
def capped_cg_reference(kernel):
    s = SMALL
    return _trajectory(kernel, s["nx"], s["ny"], s["Re"], s["K"], convection_scheme="TVD", grid_stretch=s["beta"],
                       pressure_solver="cg", **CAPPED_CG)


@functools.lru_cache(maxsize=None)
def capped_linear_reference(kernel):
    s = SMALL
    return _trajectory(kernel, s["nx"], s["ny"], s["Re"], s["K"], convection_scheme="TVD", grid_stretch=s["beta"],
                       pressure_solver="cg", **CAPPED_LINEAR)


@functools.lru_cache(maxsize=None)
def loose_reference(kernel):
    s = LOOSE
    return _trajectory(kernel, s["nx"], s["ny"], s["Re"], s["K"], convection_scheme="TVD", grid_stretch=s["beta"],
                       pressure_solver="cg", linear_solver_tol=s["linear_solver_tol"], pressure_tol=s["pressure_tol"])


# ---------------------------------------------------------------------------------------------- f. the NaN latch
NAN_CASE = dict(nx=16, ny=16, beta=1.5, Re=1000.0, alpha_uv=1.0, alpha_p=1.0, linear_solver_tol=1e-9)
NAN_AT = dict(reference=11, laplacian=10, separable=10)        # the restatement's first non-finite record row (from 0)


def nan_solver_kwargs(kernel, **kw):
    c = NAN_CASE
    return dict(dict(name="fv", nx=c["nx"], ny=c["ny"], Re=c["Re"], convection_scheme="TVD", alpha_uv=c["alpha_uv"],
                     alpha_p=c["alpha_p"], linear_solver_tol=c["linear_solver_tol"], grid_stretch=c["beta"], tolerance=1e-5,
                     max_iterations=2000, check_every=256, **SOLVER_MODE[kernel]), **kw)


@functools.lru_cache(maxsize=None)
def nan_reference(kernel):
    """The iteration, counted from 0, whose record row is the restatement's first non-finite one (None within 40)."""
    c = NAN_CASE
    o = restatement(kernel, c["nx"], c["ny"], c["Re"], alpha_uv=c["alpha_uv"], alpha_p=c["alpha_p"], convection_scheme="TVD",
                    grid_stretch=c["beta"], linear_solver_tol=c["linear_solver_tol"], pressure_solver="cg")
    with np.errstate(all="ignore"):
        for k in range(40):
            if not np.all(np.isfinite(o.step())):
                return k
    return None


# ---------------------------------------------------------------------------------------------- g. more than one launch
LAUNCH_MAX = 256                         # LDC_FV_LAUNCH_MAX (include/ldc_fv.h)
LAUNCH_N, LAUNCH_K = LAUNCH_MAX + 2, 20  # handles per kind, iterations
LAUNCH_CHECKED = (0, LAUNCH_MAX - 1, LAUNCH_MAX, LAUNCH_N - 1)


def launch_re(q):
    """Re spread over 100 ... 1000, as tests/test_gpu_fv_batched.py::test_more_trials_than_one_launch_takes spreads it."""
    return 100.0 + 900.0 * q / (LAUNCH_N - 1)


def launch_solver_kwargs(kernel, q):
    return dict(name="fv", nx=8, ny=8, Re=launch_re(q), convection_scheme="TVD", alpha_uv=0.05, alpha_p=0.05,
                linear_solver_tol=1e-9, grid_stretch=1.5, tolerance=1e-30, max_iterations=LAUNCH_K, check_every=32,
                **SOLVER_MODE[kernel])


@functools.lru_cache(maxsize=None)
def launch_reference(kernel, q):
    return _trajectory(kernel, 8, 8, launch_re(q), LAUNCH_K, alpha_uv=0.05, alpha_p=0.05, convection_scheme="TVD",
                       grid_stretch=1.5, linear_solver_tol=1e-9, pressure_solver="cg")


# ---------------------------------------------------------------------------------------------- h. more than one stride
STRIDES = dict(nx=37, ny=50, Re=400.0, grid_stretch=1.0, Lx=2.0, Ly=0.5, lid_velocity=2.0)      # 1850 cells: four strides
STRIDES_KERNELS = ("separable", "reference")


def strides_solver_kwargs(kernel, **kw):
    return dict(dict(name="fv", convection_scheme="TVD", alpha_uv=0.4, alpha_p=0.2, linear_solver_tol=1e-9, tolerance=1e-30,
                     check_every=32, **STRIDES, **SOLVER_MODE[kernel]), **kw)
