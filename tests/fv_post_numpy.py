"""NumPy statements of the finite-volume post-processing (include/ldc_fv.h, ldc_fv_post_enqueue), shared by
tests/test_fv_post_cpu.py and tests/test_gpu_fv_post.py: the sine fast-diagonalisation solve of the streamfunction in
fp64 and in long double, the extrema rule, the host code path of ``FVSolver`` on bare arrays, and the seeded states and
error bounds of the GPU tests."""
from types import SimpleNamespace

import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)

# (nx, ny, Lx, Ly): the shapes of the issue's accuracy table ...
TABLE_SHAPES = [(8, 8, 1.0, 1.0), (13, 17, 1.0, 1.0), (37, 50, 2.0, 0.5), (9, 250, 1.0, 1.0), (256, 8, 1.0, 1.0),
                (131, 77, 1.0, 1.0), (255, 253, 1.0, 1.0), (256, 256, 1.0, 1.0)]
# ... and of the GPU field tests: 8 x 8 is one partial tile with K no multiple of 4, 18 x 18 exactly one tile,
# 19 x 19 one tile + 1
GPU_SHAPES = [(8, 8, 1.0, 1.0), (18, 18, 1.0, 1.0), (19, 19, 1.0, 1.0), (13, 17, 1.0, 1.0), (37, 50, 2.0, 0.5),
              (9, 250, 1.0, 1.0), (256, 8, 1.0, 1.0), (131, 77, 1.0, 1.0), (256, 256, 1.0, 1.0)]


def shape_id(s):
    return f"{s[0]}x{s[1]}"


def sine_basis(m, dtype=np.float64):
    """(lam, S) of tridiag(-1, 2, -1), m x m: S[k, j] = sqrt(2/(m+1)) sin(pi (k+1)(j+1)/(m+1))."""
    pi = np.arccos(dtype(-1))
    k = np.arange(1, m + 1).astype(dtype)
    S = np.sqrt(dtype(2) / dtype(m + 1)) * np.sin(pi * np.outer(k, k) / dtype(m + 1))
    return dtype(2) - dtype(2) * np.cos(pi * k / dtype(m + 1)), S


def psi_solve(omega, dx, dy, dtype=np.float64):
    """psi (ny, nx), zero on the boundary ring, from (cx Tx + cy Ty) psi = omega on the interior cells by fast
    diagonalisation: psi = Sy ((Sy^T F Sx) / (cy lamy[a] + cx lamx[b])) Sx^T.  ``dtype=LD``: the long-double yardstick."""
    ny, nx = omega.shape
    lx, Sx = sine_basis(nx - 2, dtype)
    ly, Sy = sine_basis(ny - 2, dtype)
    cx, cy = dtype(1) / (dtype(dx) * dtype(dx)), dtype(1) / (dtype(dy) * dtype(dy))
    F = omega[1:-1, 1:-1].astype(dtype)
    h = (Sy.T @ F @ Sx) / (cy * ly[:, None] + cx * lx[None, :])
    psi = np.zeros((ny, nx), dtype=dtype)
    psi[1:-1, 1:-1] = Sy @ h @ Sx.T
    return psi


def kappa(nx, ny, dx, dy):
    """Condition number of the interior 5-point Dirichlet operator: largest over smallest cy lamy + cx lamx."""
    lx, _ = sine_basis(nx - 2)
    ly, _ = sine_basis(ny - 2)
    cx, cy = 1.0 / (dx * dx), 1.0 / (dy * dy)
    return float((cy * ly[-1] + cx * lx[-1]) / (cy * ly[0] + cx * lx[0]))


def cell_centres(nx, ny, Lx, Ly):
    return (np.arange(nx) + 0.5) * (Lx / nx), (np.arange(ny) + 0.5) * (Ly / ny)


def mask_bounds(xs, ys):
    """(ix_lt, ix_gt, jy_lt, jy_gt): xs < 0.5 is i < ix_lt, xs > 0.5 is i >= ix_gt; likewise ys."""
    return (int(np.count_nonzero(xs < 0.5)), int(xs.size - np.count_nonzero(xs > 0.5)),
            int(np.count_nonzero(ys < 0.5)), int(ys.size - np.count_nonzero(ys > 0.5)))


def _first_best(values, cells):
    """(value, cell) of the largest entry of values[cells] scanning the cells in increasing order with a strict
    comparison; (-inf, -1) when there is none."""
    best, at = -np.inf, -1
    flat = values.ravel()
    for c in cells:
        if flat[c] > best:
            best, at = flat[c], int(c)
    return best, at


def extrema(psi, omega, bounds, xs, ys):
    """The vortex-metrics dict by the device's rule: five (value, lowest cell) extrema, the corner regions from index
    bounds, a corner that is not > 0 reported as zeros; x, y from xs, ys by index."""
    ny, nx = psi.shape
    ix_lt, ix_gt, jy_lt, jy_gt = bounds
    cells = np.arange(nx * ny)
    i, j = cells % nx, cells // nx
    _, cmin = _first_best(-psi, cells)
    _, cmax = _first_best(np.abs(omega), cells)
    out = dict(psi_min=float(psi.ravel()[cmin]), psi_min_x=float(xs[cmin % nx]), psi_min_y=float(ys[cmin // nx]),
               omega_center=float(omega.ravel()[cmin]), omega_max=float(omega.ravel()[cmax]),
               omega_max_x=float(xs[cmax % nx]), omega_max_y=float(ys[cmax // nx]))
    regions = {"BR": (i >= ix_gt) & (j < jy_lt), "BL": (i < ix_lt) & (j < jy_lt), "TL": (i < ix_lt) & (j >= jy_gt)}
    for name, mask in regions.items():
        val, c = _first_best(psi, cells[mask])
        if val > 0:
            out.update({f"psi_{name}": float(val), f"psi_{name}_x": float(xs[c % nx]), f"psi_{name}_y": float(ys[c // nx])})
        else:
            out.update({f"psi_{name}": 0.0, f"psi_{name}_x": 0.0, f"psi_{name}_y": 0.0})
    return out


def host_namespace(nx, ny, Lx=1.0, Ly=1.0, lid=1.0, u=None, v=None):
    """What the host methods of ``FVSolver`` read, without a device: call them unbound on this."""
    xs, ys = cell_centres(nx, ny, Lx, Ly)
    X, Y = np.meshgrid(xs, ys)
    ns = SimpleNamespace(nx=nx, ny=ny, shape_full=(ny, nx), dx_min=Lx / nx, dy_min=Ly / ny,
                         params=SimpleNamespace(lid_velocity=lid, vortex_metrics="host"),
                         fields=SimpleNamespace(x=X.ravel(), y=Y.ravel(), u=u, v=v))
    return ns


def host_fields(ns):
    """(omega, psi) by the solver's host code (ghost-cell vorticity, SciPy sparse solve)."""
    from solvers.fv.solver import FVSolver
    ns._ghost_gradient = lambda f2, bc: FVSolver._ghost_gradient(ns, f2, bc)
    omega = FVSolver._vorticity(ns)
    return omega, FVSolver._streamfunction(ns, omega)


def host_metrics(ns, omega, psi):
    """The host branch of ``FVSolver.compute_vortex_metrics`` on given arrays."""
    from solvers.fv.solver import FVSolver
    ns._vorticity = lambda: omega
    ns._streamfunction = lambda w: psi
    return FVSolver.compute_vortex_metrics(ns)


def random_state(nx, ny, seed=None):
    """u, v of the GPU field tests: seeded normal values per cell."""
    rng = np.random.default_rng(1000 * nx + ny if seed is None else seed)
    return rng.normal(size=nx * ny), rng.normal(size=nx * ny)


def omega_bound(u, v, lid, dx, dy):
    """4 eps max(|u|, |v|, lid) (1/dx + 1/dy): two differences and a division per term."""
    return 4 * EPS * max(float(np.max(np.abs(u))), float(np.max(np.abs(v))), abs(lid)) * (1 / dx + 1 / dy)


def psi_bound(psi_ld, nx, ny, dx, dy):
    """4 eps kappa max|psi|."""
    return 4 * EPS * kappa(nx, ny, dx, dy) * float(np.max(np.abs(psi_ld)))


def runner_up_gaps(psi, omega, bounds):
    """Per extremum, best minus second-best candidate (of -psi, |omega|, psi inside BR, BL, TL); inf with < 2 cells."""
    ny, nx = psi.shape
    ix_lt, ix_gt, jy_lt, jy_gt = bounds
    cells = np.arange(nx * ny)
    i, j = cells % nx, cells // nx

    def gap(values):
        top = np.sort(values)[-2:]
        return float(top[1] - top[0]) if top.size == 2 else np.inf
    return dict(psi_min=gap(-psi.ravel()), omega_max=gap(np.abs(omega).ravel()),
                psi_BR=gap(psi.ravel()[(i >= ix_gt) & (j < jy_lt)]), psi_BL=gap(psi.ravel()[(i < ix_lt) & (j < jy_lt)]),
                psi_TL=gap(psi.ravel()[(i < ix_lt) & (j >= jy_gt)]))
