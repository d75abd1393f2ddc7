"""Finite-volume SIMPLE solver of the lid-driven cavity on MI355X (the reference's ``solvers.fv.solver.FVSolver``).

Contract: reference src/solvers/fv/solver.py (the iteration, :170-257), base.py:202-330 (the loop and its record),
:359-450 (E, Z, P), :569-760 (streamfunction and vortex extrema).  Every SIMPLE iteration runs in the HIP kernel of
include/ldc_fv.h -- one work-group per trial, ``check_every`` iterations per launch -- and the host only reads the
record rows and the latch.  ``acceleration="anderson"`` mixes the iterates on the device after every iteration
(``ldc_fv_anderson_enqueue``: one launch per iteration and a mixing launch after it, still one wait per chunk);
``acceleration="anderson_chip"`` is the same mixing for ``mapping="chip"`` and ``"shared"`` trials, three launches over
the whole chip behind every iteration (``ldc_fv_wide_set_anderson``).  The host computes, once per trial, the eigenvectors of the 1-D Neumann Laplacians that the
kernel's exact pressure-correction solve uses, and, once per solve, the vortex metrics: on the host with SciPy's sparse
solve (``vortex_metrics="host"``, the default) or on the device (``"device"``: ``ldc_fv_post_enqueue``, one work-group
per trial, the same quantities by the same rules; ``"chip"``: ``ldc_fv_wide_post_enqueue``, the whole chip per trial, for
``mapping="chip"`` and ``"shared"`` trials of up to 1024 cells per axis, the same bits as ``"device"`` where both exist).
``streamfunction="wall"`` reads the vortices by a second-order rule instead of the reference's (psi = 0 on the wall faces,
the lid profile in omega's ghost row; ``vortex_refine="quadratic"``: sub-cell centres), always on the device and for every
mapping and size (``ldc_fv_wall_post_enqueue``: the wall trials of a call share seven launches per 24 of them).
``grid="tanh"`` clusters the cells of a ``mapping="cu"`` trial at the walls (``ldc_fv_set_grid``: the same iteration with the
geometry read from per-axis tables, either pressure equation); its vortex metrics are computed on the host by the
reference's rule, or with ``streamfunction="wall_stretched"`` on the device by the wall rule on the stretched mesh
(``ldc_fv_wall_stretched_post_enqueue``: the Dirichlet generalised eigenpairs of each axis, the quadratic fit with unequal
spacing; such trials of a call share seven launches per 32 of them).  With ``mapping="chip"`` and ``chip_grid="tables"`` a
lone such trial of 8 ... 1024 cells per axis runs on the whole chip (``ldc_fv_wide_set_grid``: the chip chain with stretched
twins of the phases that read the geometry, ``pressure_equation`` ``"reference"`` or ``"consistent"``; with
``chip_preconditioner="separable"`` the CG of the consistent equation takes the separable scaled preconditioner of the one-CU
kernel, ``ldc_fv_wide_set_preconditioner``).
``transfer="tables"`` on the FINE trial of a pair lets ``prolong`` / ``start_from`` read both grids from per-axis tables
(``ldc_fv_prolong_tables_enqueue``: one work-group per pair, 23 pairs per launch), so stretched trials are sequenced, continued
in Re and started from uniform ones; the default ``"uniform"`` is the equal-spacing transfer of before.
``chip_transfer="tables"`` is the same for a lone ``mapping="chip"`` trial on either grid
(``ldc_fv_wide_prolong_tables_enqueue``: the same arithmetic, two launches over the whole chip per pair, 8 ... 1024 cells per
axis on both sides, a source of any mapping and grid), so a stretched chip trial is sequenced up to 1024 cells.
"""
from __future__ import annotations

import ctypes as C
import logging

import numpy as np

from .. import validation as _val
from ..base import LidDrivenCavitySolver
from ..datastructures import FVParameters
from . import ldc_fv_lib as F

log = logging.getLogger(__name__)

SCHEMES = {"Upwind": 0, "TVD": 1}
VORTEX_METRICS = ("host", "device", "chip")
ACCELERATIONS = ("none", "anderson", "anderson_chip")
MAPPINGS = ("cu", "chip", "shared")
# "consistent": the chain of launches over the whole chip (mapping "chip" / "shared"); "consistent_cu": the same equation
# inside the work-group of a one-CU trial (mapping "cu"); both are LDC_FV_PRESSURE_CONSISTENT to the library
PRESSURE_EQUATIONS = ("reference", "consistent", "consistent_cu")
STREAMFUNCTIONS = ("reference", "wall", "wall_stretched")
WALL_RULES = ("wall", "wall_stretched")      # the wall rule on equal spacing, and on the tables of grid="tanh"
VORTEX_REFINES = ("none", "quadratic")
GRIDS = ("uniform", "tanh")
# what the phase kernels of a mapping "chip" trial read the geometry from: "uniform" (dx, dy) or "tables" (the per-axis tables
# of grid="tanh": ldc_fv_wide_set_grid, a lone chip trial of 8 ... 1024 cells per axis)
CHIP_GRIDS = ("uniform", "tables")
# what preconditions the CG of such a trial with pressure_equation "consistent": "laplacian" (the operator with D left out) or
# "separable" (the tables of pressure_preconditioner "separable" on the chip chain: ldc_fv_wide_set_preconditioner)
CHIP_PRECONDITIONERS = ("laplacian", "separable")
PRESSURE_PRECONDITIONERS = ("laplacian", "separable")
# what prolong / start_from / the levels of solver=fv/fsg read the geometry from: "uniform" (dx, dy: the equal-spacing kernels)
# or "tables" (per-axis tables of centres, widths and face weights: ldc_fv_prolong_tables_enqueue, either grid, mapping "cu")
TRANSFERS = ("uniform", "tables")
# the same choice for a lone mapping "chip" trial as the fine one of a pair: "uniform" (the routes of `transfer`) or "tables"
# (ldc_fv_wide_prolong_tables_enqueue: both grids from per-axis tables, two launches over the chip, 8 ... 1024 cells per axis)
CHIP_TRANSFERS = ("uniform", "tables")
LINEAR_MAX_ITERATIONS = 1000        # scipy_solver.py:15


def lid_profile(nx, Lx=1.0, lid_velocity=1.0, corner_treatment="none", corner_smoothing=0.15) -> np.ndarray:
    """u on the lid faces, evaluated as the reference's mesh builder does (simple_structured.py:244-262)."""
    x = np.linspace(0, Lx, nx + 1)
    xf = 0.5 * (x[:-1] + x[1:])
    xi = xf / Lx
    if corner_treatment in ("polynomial", "saad"):
        return 16.0 * xi**2 * (1.0 - xi) ** 2 * lid_velocity
    u = np.full(nx, float(lid_velocity))
    if corner_treatment == "smoothing":
        d = corner_smoothing * Lx
        for i, x_face in enumerate(xf):
            if x_face < d:
                u[i] = 0.5 * (1 - np.cos(np.pi * x_face / d)) * lid_velocity
            elif x_face > (Lx - d):
                u[i] = 0.5 * (1 - np.cos(np.pi * (Lx - x_face) / d)) * lid_velocity
    return u


def tanh_vertices(n: int, L: float, beta: float) -> np.ndarray:
    """The n + 1 vertices of one axis of the wall-clustered grid: L s(k / n), s(xi) = (1 + tanh(beta (2 xi - 1)) / tanh(beta)) / 2,
    s(xi) = xi at beta = 0."""
    xi = np.arange(n + 1) / n
    if beta == 0:
        return L * xi
    return L * (0.5 * (1.0 + np.tanh(beta * (2.0 * xi - 1.0)) / np.tanh(beta)))


def axis_tables(xv):
    """(centres, h, d, g) of one axis with the vertices ``xv``: widths h (n); per face k = 0 .. n the distance d between the
    centres it separates (walls: h / 2) and the weight g of the cell behind it, (xv[k] - xc[k-1]) / d (walls: 0, not read).
    ``np.concatenate([h, d, g])`` is the table of ``ldc_fv_set_grid``."""
    xv = np.asarray(xv, dtype=np.float64)
    n = xv.size - 1
    xc = 0.5 * (xv[:-1] + xv[1:])
    h = xv[1:] - xv[:-1]
    d, g = np.zeros(n + 1), np.zeros(n + 1)
    d[0], d[n] = 0.5 * h[0], 0.5 * h[-1]
    d[1:n] = xc[1:] - xc[:-1]
    g[1:n] = (xv[1:n] - xc[:-1]) / d[1:n]
    return xc, h, d, g


def generalised_eig_host(h, d, rho=1.0):
    """(eigenvalues ascending, eigenvectors as columns) of K q = lam H q with Q^T H Q = I: K the 1-D Neumann stiffness with the
    weights rho / d of the inner faces, H = diag(h); index 0 = zero mode.  With them the operator Hy (x) Kx + Ky (x) Hx of the
    pressure correction on a tensor grid is solved by the four products of the uniform case, divisor lamy[a] + lamx[b]."""
    from scipy.linalg import eigh
    n = h.size
    w = rho / d[1:n]
    K = np.zeros((n, n))
    i = np.arange(n - 1)
    K[i, i] += w
    K[i + 1, i + 1] += w
    K[i, i + 1] -= w
    K[i + 1, i] -= w
    lam, Q = eigh(K, np.diag(h))
    # (the first mode above zero stays near rho (pi / L)^2 whatever n is, while lam[-1] grows like 1 / h_min^2: on the grids of
    # the chip mapping, up to 1024 cells, lam[1] / lam[-1] falls below 1e-6, so lam[1] is held against the former)
    assert abs(lam[0]) < 1e-9 * lam[-1] and lam[1] > 0.5 * rho * (np.pi / h.sum()) ** 2, "Neumann stiffness: one zero mode, first"
    return lam, Q


_grid_cache = {}


def grid_axis(n: int, L: float, beta: float, device, rho=1.0):
    """The device tensors of one axis of a tanh grid, cached per (n, L, beta, rho, device) like ``sine_eig``: (table
    [h | d | g], lam, Q).  Trials of equal axes share one upload and one eigen-decomposition."""
    import torch
    device = torch.device(device)
    key = (int(n), float(L), float(beta), float(rho), device.type,
           torch.cuda.current_device() if device.index is None else device.index)
    if key not in _grid_cache:
        _, h, d, g = axis_tables(tanh_vertices(n, L, beta))
        lam, Q = generalised_eig_host(h, d, rho)
        f64 = dict(dtype=torch.float64, device=device)
        _grid_cache[key] = (torch.tensor(np.concatenate([h, d, g]), **f64), torch.tensor(lam, **f64),
                            torch.tensor(Q, **f64).contiguous())
    return _grid_cache[key]


_transfer_cache = {}


def transfer_axis(n: int, L: float, beta: float, device):
    """The device tensor of one axis of ``ldc_fv_prolong_tables_enqueue``, [xc (n) | h (n) | d (n + 1) | g (n + 1)], cached per
    (n, L, beta, device) like ``grid_axis``: the cell centres, then the geometry table of ``ldc_fv_set_grid``.  ``beta`` = 0 is
    an equally spaced axis (a uniform trial): the same table of its vertices k L / n, and no eigen-decomposition either way."""
    import torch
    device = torch.device(device)
    key = (int(n), float(L), float(beta), device.type, torch.cuda.current_device() if device.index is None else device.index)
    if key not in _transfer_cache:
        xc, h, d, g = axis_tables(tanh_vertices(n, L, beta))
        _transfer_cache[key] = torch.tensor(np.concatenate([xc, h, d, g]), dtype=torch.float64, device=device)
    return _transfer_cache[key]


def dirichlet_eig_host(h, d):
    """(eigenvalues ascending, eigenvectors as columns) of K q = lam H q with Q^T H Q = I: K the 1-D stiffness with the
    weights 1 / d on ALL n + 1 faces (the walls carry 1 / (h / 2): zero on the wall FACE), H = diag(h).  Every lam > 0.  With
    them (Hy (x) Kx + Ky (x) Hx) psi = V . omega, the wall rule's problem on a tensor grid, is solved by the four products of
    the uniform case, divisor lamy[a] + lamx[b]."""
    from scipy.linalg import eigh
    n = h.size
    w = 1.0 / d
    K = np.diag(w[:-1] + w[1:]) - np.diag(w[1:n], 1) - np.diag(w[1:n], -1)
    lam, Q = eigh(K, np.diag(h))
    assert lam[0] > 0, "Dirichlet stiffness: no zero mode"
    return lam, Q


_wall_stretched_cache = {}


def wall_stretched_axis(n: int, L: float, beta: float, device):
    """The device tensor of one axis' post table of ``ldc_fv_wall_stretched_post_enqueue``, [xc | lam | Q (row-major)],
    cached per (n, L, beta, device) like ``grid_axis``: one eigen-decomposition and one upload per axis and mesh."""
    import torch
    device = torch.device(device)
    key = (int(n), float(L), float(beta), device.type, torch.cuda.current_device() if device.index is None else device.index)
    if key not in _wall_stretched_cache:
        xc, h, d, _ = axis_tables(tanh_vertices(n, L, beta))
        lam, Q = dirichlet_eig_host(h, d)
        _wall_stretched_cache[key] = torch.tensor(np.concatenate([xc, lam, np.ascontiguousarray(Q).ravel()]),
                                                  dtype=torch.float64, device=device)
    return _wall_stretched_cache[key]


def separable_fit(hx, dxf, hy, dyf):
    """(a (nx), b (ny)) with a_i b_j ~ G_ij = hx_i hy_j / (hy_j ax_i + hx_i ay_j), ax_i = 1 / dx[i] + 1 / dx[i+1] (ay likewise):
    G is V / a_P of pure diffusion with mu left out (a constant factor in a preconditioner does not change CG), the fit the
    least-squares one of log G by a sum: a_i = exp(mean_j l_ij - m / 2), b_j = exp(mean_i l_ij - m / 2), m = mean(l)."""
    ax = 1.0 / dxf[:-1] + 1.0 / dxf[1:]
    ay = 1.0 / dyf[:-1] + 1.0 / dyf[1:]
    G = (hy[:, None] * hx[None, :]) / (hy[:, None] * ax[None, :] + hx[None, :] * ay[:, None])
    l = np.log(G)
    m = l.mean()
    return np.exp(l.mean(axis=0) - 0.5 * m), np.exp(l.mean(axis=1) - 0.5 * m)


def separable_axis_host(h, d, g, a, rho=1.0):
    """(eigenvalues ascending, eigenvectors as columns) of K q = lam M q with Q^T M Q = I: K the 1-D Neumann stiffness with the
    weights rho a_f / d of the inner faces, a_f[k] = g[k] a[k] + (1 - g[k]) a[k-1] (the rule that takes D to a face),
    M = diag(h a); index 0 = zero mode."""
    from scipy.linalg import eigh
    n = h.size
    af = g[1:n] * a[1:] + (1.0 - g[1:n]) * a[:-1]
    w = rho * af / d[1:n]
    K = np.zeros((n, n))
    i = np.arange(n - 1)
    K[i, i] += w
    K[i + 1, i + 1] += w
    K[i, i + 1] -= w
    K[i + 1, i] -= w
    lam, Q = eigh(K, np.diag(h * a))
    # (lam[1] / lam[-1] falls below 1e-6 from about 600 cells per axis on, and at 256 with beta = 2.5; lam[1] itself stays put)
    assert abs(lam[0]) < 1e-9 * lam[-1] and lam[1] > 0.5 * rho * (np.pi / h.sum()) ** 2, "Neumann stiffness: one zero mode, first"
    return lam, Q


def separable_tables_host(nx, ny, Lx, Ly, beta, rho=1.0):
    """The two tables of ``ldc_fv_set_preconditioner`` for a tanh grid, [a | lam | Q (row-major)] per axis (y: b for a)."""
    _, hx, dxf, gxf = axis_tables(tanh_vertices(nx, Lx, beta))
    _, hy, dyf, gyf = axis_tables(tanh_vertices(ny, Ly, beta))
    a, b = separable_fit(hx, dxf, hy, dyf)
    lamx, Qx = separable_axis_host(hx, dxf, gxf, a, rho)
    lamy, Qy = separable_axis_host(hy, dyf, gyf, b, rho)
    return (np.concatenate([a, lamx, np.ascontiguousarray(Qx).ravel()]),
            np.concatenate([b, lamy, np.ascontiguousarray(Qy).ravel()]))


_separable_cache = {}


def separable_tables(nx: int, ny: int, Lx: float, Ly: float, beta: float, device, rho=1.0):
    """The device tensors of ``separable_tables_host``, cached per (nx, ny, Lx, Ly, beta, rho, device) like ``grid_axis``: the
    fit couples the axes, so the key names both.  Trials of equal meshes share one upload and two eigen-decompositions."""
    import torch
    device = torch.device(device)
    key = (int(nx), int(ny), float(Lx), float(Ly), float(beta), float(rho), device.type,
           torch.cuda.current_device() if device.index is None else device.index)
    if key not in _separable_cache:
        tx, ty = separable_tables_host(nx, ny, Lx, Ly, beta, rho)
        f64 = dict(dtype=torch.float64, device=device)
        _separable_cache[key] = (torch.tensor(tx, **f64), torch.tensor(ty, **f64))
    return _separable_cache[key]


def lid_profile_at(xf, Lx=1.0, lid_velocity=1.0, corner_treatment="none", corner_smoothing=0.15) -> np.ndarray:
    """``lid_profile`` at the face centres ``xf`` of any mesh (the reference's builder evaluates the lid at the face centre)."""
    xf = np.asarray(xf, dtype=np.float64)
    xi = xf / Lx
    if corner_treatment in ("polynomial", "saad"):
        return 16.0 * xi**2 * (1.0 - xi) ** 2 * lid_velocity
    u = np.full(xf.size, float(lid_velocity))
    if corner_treatment == "smoothing":
        d = corner_smoothing * Lx
        for i, x_face in enumerate(xf):
            if x_face < d:
                u[i] = 0.5 * (1 - np.cos(np.pi * x_face / d)) * lid_velocity
            elif x_face > (Lx - d):
                u[i] = 0.5 * (1 - np.cos(np.pi * (Lx - x_face) / d)) * lid_velocity
    return u


def stretched_streamfunction_matrix(dxf, dyf):
    """The non-uniform 5-point operator on the interior cells, rows in the order j (outer), i (inner), sparse: per axis
    (2 / (d_w + d_e)) ((psi_E - psi_P) / d_e - (psi_P - psi_W) / d_w) with the distances between cell centres; the ring of
    boundary cells is 0 as in the uniform rule."""
    from scipy.sparse import diags, identity, kron

    def axis(d):                              # cells 1 .. n - 2; d[k] is the face between cells k - 1 and k
        dw, de = d[1:-2], d[2:-1]
        s = 2.0 / (dw + de)
        return diags([(s / dw)[1:], -s * (1.0 / de + 1.0 / dw), (s / de)[:-1]], [-1, 0, 1], format="csr")
    nx, ny = dxf.size - 1, dyf.size - 1
    return (kron(identity(ny - 2), axis(dxf)) + kron(axis(dyf), identity(nx - 2))).tocsr()


def neumann_eig(n: int):
    """(eigenvalues ascending, eigenvectors as columns) of the 1-D Neumann second difference; index 0 = zero mode."""
    T = 2 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1)
    T[0, 0] = T[-1, -1] = 1.0
    lam, Q = np.linalg.eigh(T)
    assert abs(lam[0]) < 1e-10 and lam[1] > 1e-6, "Neumann Laplacian: one zero mode, first"
    return lam, Q


_sine_cache = {}


def sine_eig_host(m: int):
    """(eigenvalues ascending, eigenvectors as columns) of the m x m Dirichlet second difference tridiag(-1, 2, -1),
    analytic: S[k, j] = sqrt(2 / (m + 1)) sin(pi (k + 1)(j + 1) / (m + 1)), lam[k] = 2 - 2 cos(pi (k + 1) / (m + 1))."""
    k = np.arange(1, m + 1, dtype=np.float64)
    S = np.sqrt(2.0 / (m + 1)) * np.sin(np.pi * np.outer(k, k) / (m + 1))
    return 2.0 - 2.0 * np.cos(np.pi * k / (m + 1)), S


def sine_eig(m: int, device=None):
    """``sine_eig_host(m)``; with a ``device`` as float64 tensors there, cached per (m, device): trials of equal size
    share one upload."""
    if device is None:
        return sine_eig_host(m)
    import torch
    device = torch.device(device)
    key = (int(m), device.type, torch.cuda.current_device() if device.index is None else device.index)
    if key not in _sine_cache:
        lam, S = sine_eig_host(m)
        _sine_cache[key] = (torch.tensor(lam, dtype=torch.float64, device=device),
                            torch.tensor(S, dtype=torch.float64, device=device).contiguous())
    return _sine_cache[key]


_wall_cache = {}


def wall_eig_host(n: int):
    """(eigenvalues ascending, eigenvectors as columns) of the n x n second difference tridiag(-1, 2, -1) with 3 in both
    corners (the ghost cell is minus its neighbour: zero on the wall FACE), analytic: C[j, k] = sqrt(2 / n)
    sin(pi (k + 1)(j + 1/2) / n), the last column divided by sqrt(2); lam[k] = 2 - 2 cos(pi (k + 1) / n).  Not symmetric."""
    k = np.arange(1, n + 1, dtype=np.float64)
    j = np.arange(n, dtype=np.float64) + 0.5
    Cm = np.sqrt(2.0 / n) * np.sin(np.pi * np.outer(j, k) / n)
    Cm[:, -1] /= np.sqrt(2.0)
    return 2.0 - 2.0 * np.cos(np.pi * k / n), Cm


def wall_eig(n: int, device=None):
    """``wall_eig_host(n)``; with a ``device`` as float64 tensors there, cached per (n, device), as ``sine_eig``."""
    if device is None:
        return wall_eig_host(n)
    import torch
    device = torch.device(device)
    key = (int(n), device.type, torch.cuda.current_device() if device.index is None else device.index)
    if key not in _wall_cache:
        lam, Cm = wall_eig_host(n)
        _wall_cache[key] = (torch.tensor(lam, dtype=torch.float64, device=device),
                            torch.tensor(Cm, dtype=torch.float64, device=device).contiguous())
    return _wall_cache[key]


def mask_bounds(xs, ys):
    """The corner regions of ``compute_vortex_metrics`` as index bounds on the sorted cell-centre coordinates:
    xs < 0.5 is i < ix_lt, xs > 0.5 is i >= ix_gt, likewise ys (absolute coordinates, as the reference's masks)."""
    return (int(np.count_nonzero(xs < 0.5)), int(xs.size - np.count_nonzero(xs > 0.5)),
            int(np.count_nonzero(ys < 0.5)), int(ys.size - np.count_nonzero(ys > 0.5)))


def post_route(vortex_metrics: str, has_cu_handle: bool, streamfunction: str = "reference") -> str:
    """The entry that post-processes a trial: ``"wall"`` (``ldc_fv_wall_post_enqueue``, launches shared by the wall trials
    of the call) for a ``streamfunction="wall"`` trial, whatever ``vortex_metrics`` says and for every mapping and size,
    ``"wall_stretched"`` (``ldc_fv_wall_stretched_post_enqueue``, likewise) for a ``streamfunction="wall_stretched"`` one;
    else ``"chip"`` (``ldc_fv_wide_post_enqueue``, a chain of launches over the
    whole chip for this trial alone) when the trial asks for it or has no one-CU handle, else ``"cu"``
    (``ldc_fv_post_enqueue``, one work-group, beside the other such trials of the call)."""
    if streamfunction in WALL_RULES:
        return streamfunction
    return "chip" if vortex_metrics == "chip" or not has_cu_handle else "cu"


def prolong_route(coarse_has_cu: bool, fine_has_cu: bool, coarse_chip: bool, fine_chip: bool, fine_tables: bool = False) -> str:
    """The entry that prolongs a (coarse, fine) pair: ``"tables"`` (``ldc_fv_prolong_tables_enqueue``: the geometry of both
    from per-axis tables) when the FINE trial has ``transfer="tables"``, whatever the coarse one's grid and option; else
    ``"cu"`` (``ldc_fv_prolong_enqueue``) when both trials have a one-CU
    handle; else ``"chip"`` (``ldc_fv_wide_prolong_enqueue``), which takes the whole-chip handles of both: a trial without
    one is a ``ValueError``."""
    if fine_tables:
        if not (coarse_has_cu and fine_has_cu):
            raise ValueError(f"prolong: transfer='tables' takes trials of at most {F.MAX_N} cells per axis on both sides")
        return "tables"
    if coarse_has_cu and fine_has_cu:
        return "cu"
    if coarse_chip and fine_chip:
        return "chip"
    raise ValueError(f"prolong: a trial above {F.MAX_N} cells per axis is prolonged through the whole-chip handles of both "
                     f"trials, and one of them has none: give the coarse trial mapping='chip' (or 'shared')")


def _same_extent(a: float, b: float) -> bool:
    """One domain length, to the rounding the equal-spacing kernels allow (1e-12 relative)."""
    return abs(float(a) - float(b)) <= 1e-12 * max(abs(float(a)), abs(float(b)))


def postprocess(trials):
    """omega, psi and the vortex extrema of ``trials`` (FVSolvers on one device, none in flight) on the device: one
    launch per 256 trials of the one-CU route, one chain of launches per trial of the chip route, one chain per 24
    trials of the wall route and one per 32 of the stretched wall route (``post_route``), then ONE copy of all result blocks (rows of ``WALL_RESULT_LEN`` doubles when
    the call has a wall trial: the ``POST_*`` slots come first either way).  ``psi`` and ``omega`` stay on the device as ``t["psi"]``, ``t["omega"]``; every
    trial keeps its row of the result blocks for ``compute_vortex_metrics``."""
    import torch
    from solvers.spectral import ldc_lib
    if not trials:
        return
    for s in trials:
        if s.stretched and not getattr(s, "stretched_wall", False):
            raise ValueError("postprocess: grid='tanh' trials with streamfunction='reference' are post-processed on the host "
                             "(those device kernels assume equal spacing); give the trial vortex_metrics='host', or "
                             "streamfunction='wall_stretched'")
    routes = [post_route(s.params.vortex_metrics, s._has_cu_handle, s.params.streamfunction) for s in trials]
    for s, route in zip(trials, routes):
        if route == "cu":
            s._require_cu_handle("postprocess")
        elif route == "chip" and s._wide is None:
            raise ValueError(f"postprocess: a trial of {s.nx} x {s.ny} cells with mapping={s.params.mapping!r} has no "
                             f"whole-chip handle")
    dev = trials[0].device
    index = torch.cuda.current_device() if dev.index is None else dev.index
    with torch.cuda.device(dev):
        width = F.WALL_RESULT_LEN if "wall" in routes or "wall_stretched" in routes else F.POST_RESULT_LEN
        results = torch.zeros((len(trials), width), dtype=torch.float64, device=dev)
        posts, jobs, stretched_jobs = [], [], []
        for q, s in enumerate(trials):
            if (torch.cuda.current_device() if s.device.index is None else s.device.index) != index:
                raise ValueError("postprocess: all trials must be on one device")
            if routes[q] == "wall":
                posts.append(None)
                jobs.append(s._wall_job(results[q].data_ptr()))
                continue
            if routes[q] == "wall_stretched":
                posts.append(None)
                stretched_jobs.append(s._wall_stretched_job(results[q].data_ptr()))
                continue
            lamx, Sx = sine_eig(s.nx - 2, dev)
            lamy, Sy = sine_eig(s.ny - 2, dev)
            for name in ("psi", "omega"):
                if name not in s.t:
                    s.t[name] = torch.zeros(s.n_cells, dtype=torch.float64, device=dev)
            ix_lt, ix_gt, jy_lt, jy_gt = s._mask_bounds
            posts.append(F.Post(Sx=Sx.data_ptr(), lamx=lamx.data_ptr(), Sy=Sy.data_ptr(), lamy=lamy.data_ptr(),
                                ix_lt=ix_lt, ix_gt=ix_gt, jy_lt=jy_lt, jy_gt=jy_gt, psi=s.t["psi"].data_ptr(),
                                omega=s.t["omega"].data_ptr(), result=results[q].data_ptr()))
        cu = [q for q, route in enumerate(routes) if route == "cu"]
        chip = [q for q, route in enumerate(routes) if route == "chip"]
        for q in chip:
            if "post_scratch" not in trials[q].t:
                trials[q].t["post_scratch"] = torch.zeros(F.wide_post_scratch_len(trials[q].nx, trials[q].ny),
                                                          dtype=torch.float64, device=dev)
        with ldc_lib.resident_lock(index):
            stream = torch.cuda.current_stream(dev).cuda_stream
            for lo in range(0, len(cu), F.LAUNCH_MAX):
                part = cu[lo: lo + F.LAUNCH_MAX]
                F.post_enqueue([trials[q].handle for q in part], [posts[q] for q in part], stream)
            for q in chip:
                scratch = trials[q].t["post_scratch"]
                F.wide_post_enqueue(trials[q]._wide, posts[q], scratch.data_ptr(), scratch.numel(), stream)
            if jobs:
                F.wall_post_enqueue(jobs, stream)
            if stretched_jobs:
                F.wall_stretched_post_enqueue(stretched_jobs, stream)
            rows = results.cpu().numpy()          # (synchronises the stream)
    for s, row in zip(trials, rows):
        s._post = row.copy()


def prolong(pairs):
    """Start every fine trial from the state of its coarse one: ``pairs`` of (coarse, fine) FVSolvers on one device, of
    any sizes and parameters but one domain (Lx, Ly), none in flight (``ldc_fv_prolong_enqueue``: bilinear in u, v, p from the coarse cell
    centres and the boundary values, p pinned at cell 0, mdot from the new u and v).  One call of the library for all pairs, which it checks together and
    launches ``PROLONG_LAUNCH_MAX`` (128) at a time, one work-group each; the fine trials' control words, records and work vectors are left alone (a ``solve()`` zeroes the
    control words itself), and so are the coarse trials.  A fine trial must not be the coarse or the fine trial of
    another pair of the same call: chain levels with one call per level.

    A pair with a trial above 256 cells per axis (no one-CU handle) goes through ``ldc_fv_wide_prolong_enqueue`` instead,
    two launches over the whole chip per pair, the same arithmetic; both its trials must then be ``mapping="chip"`` or
    ``"shared"`` trials (``prolong_route``).

    A pair whose FINE trial has ``transfer="tables"`` goes through ``ldc_fv_prolong_tables_enqueue``: the same transfer with
    the geometry of both trials read from per-axis tables, so either may be a ``grid="tanh"`` trial (the coarse one with any
    ``transfer``); all such pairs of a call are one call of the library, 23 per launch, one work-group each.  A pair with a
    stretched trial whose fine trial lacks the option is refused.

    A pair whose FINE trial has ``chip_transfer="tables"`` (a lone ``mapping="chip"`` trial on either grid) goes through
    ``ldc_fv_wide_prolong_tables_enqueue``: the same arithmetic, two launches over the whole chip per pair, 8 ... 1024 cells per
    axis on both sides; the coarse trial may be of any mapping and grid.  All routes may stand in one call."""
    import torch
    from solvers.spectral import ldc_lib
    pairs = list(pairs)
    if not pairs:
        return
    # (getattr: a trial built before the option, or a stand-in that has only `stretched`, is a transfer="uniform" trial)
    by_tables = [bool(getattr(f, "transfer_tables", False)) for _, f in pairs]
    by_chip_tables = [bool(getattr(f, "chip_transfer_tables", False)) for _, f in pairs]
    for (c, f), tables, chip_tables in zip(pairs, by_tables, by_chip_tables):
        if (c.stretched or f.stretched) and not (tables or chip_tables):
            raise ValueError("prolong / start_from with grid='tanh': the prolongation kernel assumes equal spacing on both "
                             "trials; give the FINE trial transfer='tables' (the transfer that reads both grids from tables)")
    dev = pairs[0][1].device
    index = torch.cuda.current_device() if dev.index is None else dev.index
    # (a fine trial with chip_transfer="tables" takes raw pointers of both trials: no handle of a particular kind is needed)
    routes = ["chip_tables" if chip_tables else prolong_route(c._has_cu_handle, f._has_cu_handle, c.chip, f.chip, tables)
              for (c, f), tables, chip_tables in zip(pairs, by_tables, by_chip_tables)]
    for (c, f), route in zip(pairs, routes):
        for s in (c, f):
            if route in ("cu", "tables"):
                s._require_cu_handle("prolong")
            elif route == "chip" and s._wide is None:
                raise ValueError(f"prolong: a trial of {s.nx} x {s.ny} cells has no whole-chip handle")
            if (torch.cuda.current_device() if s.device.index is None else s.device.index) != index:
                raise ValueError("prolong: all trials must be on one device")
        if route in ("tables", "chip_tables") and not (_same_extent(c.params.Lx, f.params.Lx) and _same_extent(c.params.Ly, f.params.Ly)):
            raise ValueError(f"prolong: the trials of a pair cover one domain, got Lx, Ly = {c.params.Lx}, {c.params.Ly} and "
                             f"{f.params.Lx}, {f.params.Ly}")
    cu = [pair for pair, route in zip(pairs, routes) if route == "cu"]
    chip = [pair for pair, route in zip(pairs, routes) if route == "chip"]
    tables = [pair for pair, route in zip(pairs, routes) if route == "tables"]
    chip_tables = [pair for pair, route in zip(pairs, routes) if route == "chip_tables"]
    if chip or tables or chip_tables:  # (the library checks the pairs of ONE of its calls together; with others beside them the rule is kept here)
        for q, (_, f) in enumerate(pairs):
            if any(f is c2 or (r != q and f is f2) for r, (c2, f2) in enumerate(pairs)):
                raise ValueError("prolong: a fine trial is the coarse or the fine trial of another pair of the call")
    with torch.cuda.device(dev):
        jobs = [f._prolong_tables_job(c) for c, f in tables]
        chip_jobs = [f._prolong_tables_job(c) for c, f in chip_tables]
        with ldc_lib.resident_lock(index):
            stream = torch.cuda.current_stream(dev).cuda_stream
            if cu:
                F.prolong_enqueue([c.handle for c, _ in cu], [f.handle for _, f in cu], stream)
            for c, f in chip:
                F.wide_prolong_enqueue(c._wide, f._wide, stream)
            if jobs:
                F.prolong_tables_enqueue(jobs, stream)
            if chip_jobs:
                F.wide_prolong_tables_enqueue(chip_jobs, stream)
            torch.cuda.current_stream(dev).synchronize()      # (the lock goes back with the CUs free)
    for _, f in pairs:
        f._post = None


def advance(trials, k):
    """One chunk for lone trials and batches alike: ``k`` iterations (at most every trial's record ring) for each of
    ``trials`` (FVSolvers on one device) in ONE launch, one work-group each, then ONE copy of their ctrl words and ONE of
    the first ``k`` rows of their record rings (the slices stack whatever the rings' own lengths); per trial (rows of the
    new iterations, latch, nan, iteration count).

    With ``acceleration="anderson"`` on any of the trials the chunk is ``k`` launches of ONE iteration with the mixing
    kernel after each (``ldc_fv_anderson_enqueue``), all enqueued before the one wait; without, the launch of before.

    A work-group holds its CU for the whole chunk, so launch and wait hold the device's resident lock: not beside a
    launch whose work-groups must all be resident (a lone trial in the launcher's pool of streams, next to spectral
    batches; solvers.fv.batched)."""
    import torch
    from solvers.spectral import ldc_lib
    from solvers.spectral.chunks import _words
    dev = trials[0].device
    index = torch.cuda.current_device() if dev.index is None else dev.index
    accelerated = any(s.accelerated for s in trials)
    with torch.cuda.device(dev):
        starts = _words([s.t["ctrl"] for s in trials])[:, F.CTRL_ITER]
        with ldc_lib.resident_lock(index):
            if accelerated:     # k launches of one iteration, a mixing launch after each; plain trials ride at depth 0
                F.anderson_enqueue([s.handle for s in trials], [s._anderson_block() for s in trials], k,
                                   torch.cuda.current_stream(dev).cuda_stream)
            else:
                F.batch_enqueue([s.handle for s in trials], k, torch.cuda.current_stream(dev).cuda_stream)
            ctrl = _words([s.t["ctrl"] for s in trials])        # (synchronises the stream)
        rings = _words([s.t["rec"][:k] for s in trials])
    return [(ring[: int(c[F.CTRL_ITER] - start)].copy(), int(c[F.CTRL_DONE]), int(c[F.CTRL_NAN]), int(c[F.CTRL_ITER]))
            for start, c, ring in zip(starts, ctrl, rings)]


def advance_with_budget(step, start, k, budget, max_lin_iters):
    """``k`` iterations of a ``"chip"`` trial that stands at iteration ``start``, whatever BiCGSTAB budget they need.

    ``step(m, budget)`` enqueues up to ``m`` iterations with ``budget`` BiCGSTAB iterations each, waits, and returns
    (rows of the iterations it completed, latch, nan, iteration count, overflow).  An overflow means: the iteration after
    the last completed one needs more than ``budget`` and has changed nothing; the rest is enqueued again with twice the
    budget, at most ``max_lin_iters`` (where the kernel accepts a solve that has not converged, so it cannot overflow).
    Returns (rows, latch, nan, iteration count, budget now, retries): no iteration is lost or counted twice."""
    import numpy as np
    blocks, total, retries = [], int(start), 0
    latch = nan = 0
    while total - start < k:
        rows, latch, nan, new_total, overflow = step(k - (total - start), budget)
        if len(rows) != new_total - total:
            raise RuntimeError(f"{len(rows)} record rows for iterations {total} ... {new_total}")
        blocks.append(rows)
        total = int(new_total)
        if latch or nan:
            break
        if overflow:
            if budget >= max_lin_iters:
                raise RuntimeError(f"linear budget {budget} >= max_lin_iters {max_lin_iters} reported an overflow")
            budget = min(2 * budget, int(max_lin_iters))
            retries += 1
        elif total - start < k:
            raise RuntimeError("device loop made no progress")
    rows = np.concatenate(blocks, axis=0) if blocks else np.zeros((0, F.REC_LEN))
    return rows, int(latch), int(nan), total, budget, retries


def advance_batch_with_budget(step, starts, ks, budgets, max_lin_iters):
    """``advance_with_budget`` for trials that share their launches (``mapping="shared"``): trial q stands at iteration
    ``starts[q]`` and is to do ``ks[q]`` more (0: it is left alone), whatever BiCGSTAB budget they need.

    ``step(quotas, budget)`` enqueues up to ``quotas[q]`` iterations of every trial in the same launches with ``budget``
    BiCGSTAB iterations each, waits, and returns per trial (rows of the iterations it completed, latch, nan, iteration
    count, overflow).  The first call carries every trial with ``ks[q] > 0`` at the largest of their budgets.  A trial
    that overflowed has learnt that the call's budget is not enough: its own budget becomes twice that, at most
    ``max_lin_iters``, and it is enqueued again with what is left of its count, beside the others that overflowed and
    with quota 0 for everyone else; and so on until nobody overflows.  A trial that needed no more keeps its budget.
    Returns per trial (rows, latch, nan, iteration count, budget now, retries): no iteration is lost or counted twice."""
    import numpy as np
    n = len(starts)
    starts = [int(x) for x in starts]
    totals, budgets, retries = list(starts), [int(b) for b in budgets], [0] * n
    blocks, flags = [[] for _ in range(n)], [(0, 0)] * n
    todo = [q for q in range(n) if ks[q] > 0]
    while todo:
        quotas = [0] * n
        for q in todo:
            quotas[q] = int(ks[q]) - (totals[q] - starts[q])
        budget = max(budgets[q] for q in todo)
        out = step(list(quotas), budget)
        if len(out) != n:
            raise RuntimeError("one result per trial expected")
        again = []
        for q, (rows, latch, nan, new_total, overflow) in enumerate(out):
            if len(rows) != new_total - totals[q]:
                raise RuntimeError(f"trial {q}: {len(rows)} record rows for iterations {totals[q]} ... {new_total}")
            if quotas[q] == 0:
                if new_total != totals[q]:
                    raise RuntimeError(f"trial {q} had quota 0 and went from iteration {totals[q]} to {new_total}")
                continue
            blocks[q].append(rows)
            totals[q] = int(new_total)
            flags[q] = (int(latch), int(nan))
            if latch or nan:
                continue
            if overflow:
                if budget >= max_lin_iters:
                    raise RuntimeError(f"trial {q}: linear budget {budget} >= max_lin_iters {max_lin_iters} reported "
                                       f"an overflow")
                budgets[q] = min(2 * budget, int(max_lin_iters))
                retries[q] += 1
                again.append(q)
            elif totals[q] - starts[q] < ks[q]:
                raise RuntimeError(f"trial {q}: device loop made no progress")
        todo = again
    return [(np.concatenate(b, axis=0) if b else np.zeros((0, F.REC_LEN)), latch, nan, total, budget, r)
            for b, (latch, nan), total, budget, r in zip(blocks, flags, totals, budgets, retries)]


def advance_with_budgets(step, start, k, budgets, caps):
    """``advance_with_budget`` for a trial with the consistent pressure equation, whose iterations carry two fixed numbers
    of launches: ``budgets`` = (BiCGSTAB iterations, CG iterations of the pressure solve) per SIMPLE iteration, ``caps`` =
    (max_lin_iters, pressure_max_iters).

    ``step(m, linear_budget, pressure_budget)`` enqueues up to ``m`` iterations, waits, and returns (rows of the iterations
    it completed, latch, nan, iteration count, overflow): overflow ``OVERFLOW_LINEAR`` (1) when a momentum solve of the next
    iteration needs more than its budget, ``OVERFLOW_PRESSURE`` (2) when its pressure solve does; either way that iteration
    has changed nothing, and the rest is enqueued again with twice THAT budget, at most its cap.  Returns (rows, latch, nan,
    iteration count, budgets now, retries per budget)."""
    import numpy as np
    budgets, retries = [int(b) for b in budgets], [0, 0]
    blocks, total = [], int(start)
    latch = nan = 0
    while total - start < k:
        rows, latch, nan, new_total, overflow = step(k - (total - start), budgets[0], budgets[1])
        if len(rows) != new_total - total:
            raise RuntimeError(f"{len(rows)} record rows for iterations {total} ... {new_total}")
        blocks.append(rows)
        total = int(new_total)
        if latch or nan:
            break
        if overflow:
            if overflow not in (F.OVERFLOW_LINEAR, F.OVERFLOW_PRESSURE):
                raise RuntimeError(f"overflow word {overflow}")
            which = overflow - 1
            if budgets[which] >= caps[which]:
                raise RuntimeError(f"{('linear', 'pressure')[which]} budget {budgets[which]} >= its cap {caps[which]} "
                                   f"reported an overflow")
            budgets[which] = min(2 * budgets[which], int(caps[which]))
            retries[which] += 1
        elif total - start < k:
            raise RuntimeError("device loop made no progress")
    rows = np.concatenate(blocks, axis=0) if blocks else np.zeros((0, F.REC_LEN))
    return rows, int(latch), int(nan), total, tuple(budgets), tuple(retries)


def advance_batch_with_budgets(step, starts, ks, budgets, caps):
    """``advance_batch_with_budget`` with the two budgets of ``advance_with_budgets``: ``budgets[q]`` = (BiCGSTAB, CG) of trial
    q, ``caps`` = (max_lin_iters, pressure_max_iters).  ``step(quotas, linear_budget, pressure_budget)`` returns per trial
    (rows, latch, nan, iteration count, overflow code).  A call carries the largest budget of either kind among its trials; a
    trial that overflowed takes twice the CALL's budget of the kind it ran out of and is enqueued again beside the others
    that overflowed, quota 0 for everyone else.  Returns per trial (rows, latch, nan, iteration count, budgets now, retries
    per budget)."""
    import numpy as np
    n = len(starts)
    starts = [int(x) for x in starts]
    totals, budgets, retries = list(starts), [[int(b) for b in bq] for bq in budgets], [[0, 0] for _ in range(n)]
    blocks, flags = [[] for _ in range(n)], [(0, 0)] * n
    todo = [q for q in range(n) if ks[q] > 0]
    while todo:
        quotas = [0] * n
        for q in todo:
            quotas[q] = int(ks[q]) - (totals[q] - starts[q])
        call = [max(budgets[q][w] for q in todo) for w in range(2)]
        out = step(list(quotas), call[0], call[1])
        if len(out) != n:
            raise RuntimeError("one result per trial expected")
        again = []
        for q, (rows, latch, nan, new_total, overflow) in enumerate(out):
            if len(rows) != new_total - totals[q]:
                raise RuntimeError(f"trial {q}: {len(rows)} record rows for iterations {totals[q]} ... {new_total}")
            if quotas[q] == 0:
                if new_total != totals[q]:
                    raise RuntimeError(f"trial {q} had quota 0 and went from iteration {totals[q]} to {new_total}")
                continue
            blocks[q].append(rows)
            totals[q] = int(new_total)
            flags[q] = (int(latch), int(nan))
            if latch or nan:
                continue
            if overflow:
                if overflow not in (F.OVERFLOW_LINEAR, F.OVERFLOW_PRESSURE):
                    raise RuntimeError(f"trial {q}: overflow word {overflow}")
                which = overflow - 1
                if call[which] >= caps[which]:
                    raise RuntimeError(f"trial {q}: {('linear', 'pressure')[which]} budget {call[which]} >= its cap "
                                       f"{caps[which]} reported an overflow")
                budgets[q][which] = min(2 * call[which], int(caps[which]))
                retries[q][which] += 1
                again.append(q)
            elif totals[q] - starts[q] < ks[q]:
                raise RuntimeError(f"trial {q}: device loop made no progress")
        todo = again
    return [(np.concatenate(b, axis=0) if b else np.zeros((0, F.REC_LEN)), latch, nan, total, tuple(bq), tuple(r))
            for b, (latch, nan), total, bq, r in zip(blocks, flags, totals, budgets, retries)]


class SharedBatch:
    """``solvers`` (FVSolvers with ``mapping="shared"`` on one device, at most ``WIDE_BATCH_MAX``) as ONE batch object of
    the library (``ldc_fv_wide_batch_*``): every phase launch carries the work-groups of all of them, and an enqueue gives
    every trial its own quota of iterations.  The table the kernels look their work-group up in lives in a tensor of this
    object.  A lone shared trial is a batch of one."""

    def __init__(self, solvers, graph=None):
        import torch
        self.solvers = list(solvers)
        if not 1 <= len(self.solvers) <= F.WIDE_BATCH_MAX:
            raise ValueError(f"{len(self.solvers)} trials in one shared batch: 1 ... {F.WIDE_BATCH_MAX}")
        self.device = self.solvers[0].device
        self._wides = [s._wide.value for s in self.solvers]
        self.handle = None
        with torch.cuda.device(self.device):
            self.table = torch.empty(F.wide_batch_table_len([(s.nx, s.ny) for s in self.solvers]), dtype=torch.uint8,
                                     device=self.device)
            torch.cuda.current_stream(self.device).synchronize()      # (create copies the table on the library's stream)
            self.handle = F.wide_batch_create(self._wides, self.table.data_ptr(), self.table.numel())
        if graph is not None:
            self.set_graph(graph)

    def set_graph(self, on: bool):
        F.check(F.lib().ldc_fv_wide_batch_set_graph(self.handle, int(bool(on))), "ldc_fv_wide_batch_set_graph")

    def close(self):
        if self.handle is not None:
            F.lib().ldc_fv_wide_batch_destroy(self.handle)
            self.handle = None

    def _step(self, quotas, budget, pressure_budget=None):
        """ONE enqueue and ONE wait, then one copy each of the control words, the overflow words and the new record rows
        (``advance_batch_with_budget``'s step; with a ``pressure_budget``, ``advance_batch_with_budgets``'s)."""
        import torch
        from solvers.spectral import ldc_lib
        from solvers.spectral.chunks import _words
        dev, ss = self.device, self.solvers
        index = torch.cuda.current_device() if dev.index is None else dev.index
        with torch.cuda.device(dev):
            if pressure_budget is not None:
                F.check(F.lib().ldc_fv_wide_batch_set_pressure_budget(self.handle, int(pressure_budget)),
                        "ldc_fv_wide_batch_set_pressure_budget")
            with ldc_lib.resident_lock(index):
                F.wide_batch_enqueue(self.handle, quotas, budget, torch.cuda.current_stream(dev).cuda_stream)
                ctrl = _words([s.t["ctrl"] for s in ss])          # (synchronises the stream)
            overflow = _words([s.t["scratch"][:1].view(torch.int64) for s in ss])[:, 0]
            new = [int(c[F.CTRL_ITER]) - t for c, t in zip(ctrl, self._totals)]
            got = [s.t["rec"][:m] for s, m in zip(ss, new) if m > 0]
            rows = torch.cat(got).cpu().numpy() if got else np.zeros((0, F.REC_LEN))
        out, lo = [], 0
        for q, (c, m) in enumerate(zip(ctrl, new)):
            out.append((rows[lo: lo + m].copy(), int(c[F.CTRL_DONE]), int(c[F.CTRL_NAN]), int(c[F.CTRL_ITER]),
                        int(overflow[q])))
            lo += max(m, 0)
            self._totals[q] = int(c[F.CTRL_ITER])
        return out

    def advance(self, ks):
        """``ks[q]`` iterations of trial q (0: left alone; at most its record ring), all in the same launches, whatever
        budgets they need; per trial (rows of the new iterations, latch, nan, iteration count).  Every trial's
        ``linear_budget`` and ``linear_budget_retries`` go on as a lone trial's do."""
        import torch
        from solvers.spectral.chunks import _words
        ss = self.solvers
        if [s._wide.value if s._wide is not None else None for s in ss] != self._wides:
            raise RuntimeError("a trial of a shared batch has a new device handle: the batch's table is out of date")
        with torch.cuda.device(self.device):
            self._totals = [int(t) for t in _words([s.t["ctrl"] for s in ss])[:, F.CTRL_ITER]]
        consistent = [s for s in ss if s.consistent]
        if consistent:      # (ldc_fv_wide_batch_create has seen to it that they share pressure_max_iters)
            out = advance_batch_with_budgets(self._step, list(self._totals), [int(k) for k in ks],
                                             [(s.linear_budget, s.pressure_budget) for s in ss],
                                             (LINEAR_MAX_ITERATIONS, int(consistent[0].params.pressure_max_iters)))
            for s, (_, _, _, _, budgets, retries) in zip(ss, out):
                s.linear_budget, s.pressure_budget = budgets
                s.linear_budget_retries += retries[0]
                s.pressure_budget_retries += retries[1]
            return [(rows, latch, nan, total) for rows, latch, nan, total, _, _ in out]
        out = advance_batch_with_budget(self._step, list(self._totals), [int(k) for k in ks],
                                        [s.linear_budget for s in ss], LINEAR_MAX_ITERATIONS)
        for s, (_, _, _, _, budget, retries) in zip(ss, out):
            s.linear_budget = budget
            s.linear_budget_retries += retries
        return [(rows, latch, nan, total) for rows, latch, nan, total, _, _ in out]


class FVSolver(LidDrivenCavitySolver):
    """Collocated finite-volume SIMPLE solver; ``nx`` x ``ny`` cells (8 ... 256 each with ``mapping="cu"``, one
    work-group per trial; 8 ... 1024 with ``mapping="chip"``, one launch per phase over the whole chip, and with
    ``mapping="shared"``, the same launches shared by all trials of a batch).  ``streamfunction()``, ``vorticity()``,
    ``vortex_metrics="chip"``, ``prolong`` and ``start_from`` take a chip or shared trial of any of these sizes; a chip trial
    on a stretched mesh (``chip_grid="tables"``) starts from another trial with ``chip_transfer="tables"``."""

    Parameters = FVParameters
    rho = 1.0
    _needs_cu_handle = None                   # (a subclass that cannot do without the one-CU handle names itself here)

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        p = self.params
        if p.convection_scheme not in SCHEMES:
            raise ValueError(f"convection_scheme={p.convection_scheme!r}: 'Upwind' or 'TVD'")
        if p.convection_scheme == "TVD" and p.limiter != "MUSCL":
            raise ValueError(f"limiter={p.limiter!r}: the TVD scheme of the reference is MUSCL")
        if p.vortex_metrics not in VORTEX_METRICS:
            raise ValueError(f"vortex_metrics={p.vortex_metrics!r}: 'host', 'device' or 'chip'")
        if p.streamfunction not in STREAMFUNCTIONS:
            raise ValueError(f"streamfunction={p.streamfunction!r}: 'reference', 'wall' or 'wall_stretched'")
        if p.vortex_refine not in VORTEX_REFINES:
            raise ValueError(f"vortex_refine={p.vortex_refine!r}: 'none' or 'quadratic'")
        if p.vortex_refine == "quadratic" and p.streamfunction not in WALL_RULES:
            raise ValueError("vortex_refine='quadratic' with streamfunction='reference': the ring rule's O(h) error in psi "
                             "makes sub-cell centres moot, give the trial streamfunction='wall'")
        self.vortex_refine_status = None         # per (primary, BR, BL, TL) after a refined compute_vortex_metrics()
        if p.acceleration not in ACCELERATIONS:
            raise ValueError(f"acceleration={p.acceleration!r}: 'none', 'anderson' or 'anderson_chip'")
        if not 1 <= int(p.anderson_depth) <= F.ANDERSON_MAX_DEPTH:
            raise ValueError(f"anderson_depth={p.anderson_depth}: 1 ... {F.ANDERSON_MAX_DEPTH} columns")
        if int(p.anderson_start) < 1:
            raise ValueError(f"anderson_start={p.anderson_start}: an iteration count, at least 1")
        self.accelerated = p.acceleration == "anderson"      # the one-CU mixing path: advance() routes on it
        self.mixed_chip = p.acceleration == "anderson_chip"  # the mixing chain of the chip mapping, attached to the handle
        if p.mapping not in MAPPINGS:
            raise ValueError(f"mapping={p.mapping!r}: 'cu', 'chip' or 'shared'")
        if int(p.linear_budget) < 1:
            raise ValueError(f"linear_budget={p.linear_budget}: BiCGSTAB iterations per SIMPLE iteration, at least 1")
        if p.pressure_equation not in PRESSURE_EQUATIONS:
            raise ValueError(f"pressure_equation={p.pressure_equation!r}: 'reference', 'consistent' or 'consistent_cu'")
        self.consistent = p.pressure_equation == "consistent"          # the chip chain, with its budget protocol
        self.consistent_cu = p.pressure_equation == "consistent_cu"    # the one-CU kernel: no budget, no retries
        if self.consistent_cu and p.mapping != "cu":
            raise ValueError(f"pressure_equation='consistent_cu' with mapping={p.mapping!r}: the one-CU kernel of the "
                             f"consistent pressure equation takes mapping='cu' trials (a chip or shared trial takes "
                             f"pressure_equation='consistent')")
        if self.consistent and p.mapping == "cu":
            raise ValueError("pressure_equation='consistent' with mapping='cu': the consistent pressure equation is solved "
                             "by launches over the whole chip, give the trial mapping=chip (or mapping=shared)")
        if not 0.0 < float(p.pressure_tol) < 1.0:
            raise ValueError(f"pressure_tol={p.pressure_tol}: a relative residual, between 0 and 1")
        if int(p.pressure_max_iters) < 1:
            raise ValueError(f"pressure_max_iters={p.pressure_max_iters}: CG iterations per pressure solve, at least 1")
        if int(p.pressure_budget) < 1:
            raise ValueError(f"pressure_budget={p.pressure_budget}: CG iterations per SIMPLE iteration, at least 1")
        if p.transfer not in TRANSFERS:
            raise ValueError(f"transfer={p.transfer!r}: 'uniform' or 'tables'")
        self.transfer_tables = p.transfer == "tables"       # prolong() routes the pairs this trial is the FINE one of on it
        if p.chip_transfer not in CHIP_TRANSFERS:
            raise ValueError(f"chip_transfer={p.chip_transfer!r}: 'uniform' or 'tables'")
        self.chip_transfer_tables = p.chip_transfer == "tables"     # likewise, through ldc_fv_wide_prolong_tables_enqueue
        if self.chip_transfer_tables:
            if p.mapping != "chip":
                raise ValueError(f"chip_transfer='tables' with mapping={p.mapping!r}: the transfer over the whole chip that "
                                 f"reads the grids from tables starts a lone mapping='chip' trial (a one-CU trial takes "
                                 f"transfer='tables')")
            if self.transfer_tables:
                raise ValueError("chip_transfer='tables' beside transfer='tables': one transfer per trial, and transfer="
                                 "'tables' is the one-CU kernel's (mapping='cu')")
            if p.grid == "tanh" and p.chip_grid != "tables":
                raise ValueError(f"chip_transfer='tables' with grid='tanh' and chip_grid={p.chip_grid!r}: a stretched chip "
                                 f"trial takes chip_grid='tables'")
        if self.transfer_tables and p.mapping != "cu":
            raise ValueError(f"transfer='tables' with mapping={p.mapping!r}: the transfer that reads the grids from tables "
                             f"takes mapping='cu' trials")
        if p.grid not in GRIDS:
            raise ValueError(f"grid={p.grid!r}: 'uniform' or 'tanh'")
        self.stretched = p.grid == "tanh"         # geometry tables on the handle: fv_stretched_kernel advances the trial
        if p.chip_grid not in CHIP_GRIDS:
            raise ValueError(f"chip_grid={p.chip_grid!r}: 'uniform' or 'tables'")
        self.chip_tables = p.chip_grid == "tables"          # ... or, on the wide handle, the stretched twins of the chip chain
        if self.chip_tables and not self.stretched:
            raise ValueError(f"chip_grid='tables' with grid={p.grid!r}: the tables are those of a wall-clustered mesh, give the "
                             f"trial grid='tanh' (or chip_grid='uniform')")
        if self.chip_tables and p.mapping != "chip":
            raise ValueError(f"chip_grid='tables' with mapping={p.mapping!r}: the stretched phase kernels advance a lone "
                             f"mapping='chip' trial (a shared batch has no room for the tables in its table entry; a one-CU "
                             f"trial reads them without the option)")
        if self.stretched:
            if not float(p.grid_stretch) >= 0.0 or not np.isfinite(float(p.grid_stretch)):
                raise ValueError(f"grid_stretch={p.grid_stretch}: the tanh clustering parameter, a finite number >= 0")
            if p.mapping != "cu" and not self.chip_tables:
                raise ValueError(f"grid='tanh' with mapping={p.mapping!r}: stretched grids run on the one-CU kernel only "
                                 f"(mapping='cu')")
            if p.acceleration != "none":
                raise ValueError(f"grid='tanh' with acceleration={p.acceleration!r}: Anderson mixing has not been tested "
                                 f"on stretched grids, give the trial acceleration='none'")
            if self._needs_cu_handle and not (self.transfer_tables or self.chip_transfer_tables):
                raise ValueError("grid='tanh' with solver=fv/fsg: the prolongation between the levels assumes equal "
                                 "spacing, run the trial with solver=fv (or give it transfer='tables', the transfer that "
                                 "reads the grids of both levels from tables)")
            # (streamfunction="wall_stretched" is served on the device by ldc_fv_wall_stretched_post_enqueue and does not
            # consult vortex_metrics, as "wall" does not for uniform trials)
            if p.vortex_metrics != "host" and p.streamfunction != "wall_stretched":
                raise ValueError(f"grid='tanh' with vortex_metrics={p.vortex_metrics!r}: the post-processing kernels of the "
                                 f"reference's rule assume equal spacing, give the trial vortex_metrics='host' (or "
                                 f"streamfunction='wall_stretched')")
            if p.streamfunction == "wall":
                raise ValueError("grid='tanh' with streamfunction='wall': that kernel assumes equal spacing, give the trial "
                                 "streamfunction='wall_stretched' (the wall rule on the stretched mesh)")
        elif p.streamfunction == "wall_stretched":
            raise ValueError(f"streamfunction='wall_stretched' with grid={p.grid!r}: it reads the tables of a stretched mesh, "
                             f"give the trial grid='tanh' (or streamfunction='wall')")
        self.stretched_wall = p.streamfunction == "wall_stretched"      # postprocess() routes on it
        if p.pressure_preconditioner not in PRESSURE_PRECONDITIONERS:
            raise ValueError(f"pressure_preconditioner={p.pressure_preconditioner!r}: 'laplacian' or 'separable'")
        self.separable = p.pressure_preconditioner == "separable"     # tables on the handle: fv_stretched_sep_kernel
        if self.separable and not (self.stretched and self.consistent_cu):
            raise ValueError(f"pressure_preconditioner='separable' with grid={p.grid!r}, pressure_equation="
                             f"{p.pressure_equation!r}: it preconditions the CG of a stretched one-CU trial, give the trial "
                             f"grid='tanh' and pressure_equation='consistent_cu'")
        if p.chip_preconditioner not in CHIP_PRECONDITIONERS:
            raise ValueError(f"chip_preconditioner={p.chip_preconditioner!r}: 'laplacian' or 'separable'")
        self.chip_separable = p.chip_preconditioner == "separable"    # tables on the wide handle: the twins of the CG launches
        if self.chip_separable and not (self.chip_tables and self.consistent):
            raise ValueError(f"chip_preconditioner='separable' with mapping={p.mapping!r}, grid={p.grid!r}, chip_grid="
                             f"{p.chip_grid!r}, pressure_equation={p.pressure_equation!r}: it preconditions the CG of a lone "
                             f"stretched chip trial, give the trial mapping='chip', grid='tanh', chip_grid='tables' and "
                             f"pressure_equation='consistent' (a one-CU trial takes pressure_preconditioner='separable')")
        self.shared =p.mapping == "shared"       # the phase kernels of csrc/ldc_fv_wide.hip: a launch of its own per
        self.chip = p.mapping == "chip" or self.shared        # phase ("chip") or one for all trials of a batch ("shared")
        nx, ny = int(p.nx), int(p.ny)
        max_n = F.WIDE_MAX_N if self.chip else F.MAX_N
        if not (F.MIN_N <= nx <= max_n and F.MIN_N <= ny <= max_n):
            raise ValueError(f"nx, ny = {nx}, {ny}: the FV kernel takes {F.MIN_N} ... {max_n} cells per axis "
                             f"with mapping={p.mapping!r}")
        if self.chip and self.accelerated:
            raise ValueError(f"acceleration='anderson' with mapping={p.mapping!r}: the mixing kernel follows the one-CU "
                             f"kernel's launches only (a chip or shared trial takes acceleration='anderson_chip')")
        if self.mixed_chip and not self.chip:
            raise ValueError(f"acceleration='anderson_chip' with mapping={p.mapping!r}: the mixing chain over the whole "
                             f"chip takes mapping='chip' or 'shared' trials (a one-CU trial takes acceleration='anderson')")
        # the one-CU handle beside the wide one wherever it exists: postprocess, prolong and start_from use it
        if p.vortex_metrics == "chip" and not self.chip:
            raise ValueError(f"vortex_metrics='chip' with mapping={p.mapping!r}: the post-processing chain over the whole "
                             f"chip takes mapping='chip' or 'shared' trials")
        self._has_cu_handle = not self.chip or max(nx, ny) <= F.MAX_N
        # (with chip_transfer="tables" the levels are prolonged over the whole chip: no level needs the one-CU handle)
        if self._needs_cu_handle and not self._has_cu_handle and not self.chip_transfer_tables:
            raise ValueError(f"{self._needs_cu_handle} of {nx} x {ny} cells: the prolongation takes at most {F.MAX_N} "
                             f"cells per axis")
        if p.vortex_metrics == "device" and not self._has_cu_handle:
            raise ValueError(f"vortex_metrics='device' at {nx} x {ny}: device post-processing takes at most {F.MAX_N} "
                             f"cells per axis")
        self.nx, self.ny, self.n_cells = nx, ny, nx * ny
        self.dx_min, self.dy_min = p.Lx / nx, p.Ly / ny
        self.shape_full = (ny, nx)               # as the reference's FV solver: cells c = j*nx + i
        self.mu = self.rho * p.lid_velocity * p.Lx / p.Re
        xc, yc = (np.arange(nx) + 0.5) * self.dx_min, (np.arange(ny) + 0.5) * self.dy_min
        if self.stretched:                       # (dx_min, dy_min stay the mean widths: the kernel does not read them)
            beta = float(p.grid_stretch)
            self._xv, self._yv = tanh_vertices(nx, p.Lx, beta), tanh_vertices(ny, p.Ly, beta)
            xc, self._hx, self._dxf, self._gxf = axis_tables(self._xv)
            yc, self._hy, self._dyf, self._gyf = axis_tables(self._yv)
        X, Y = np.meshgrid(xc, yc)
        self._init_fields(x=X.ravel(), y=Y.ravel())
        self._mask_bounds = mask_bounds(np.sort(np.unique(self.fields.x)), np.sort(np.unique(self.fields.y)))
        self._post = None                        # the trial's result block of the last postprocess()

        import torch
        from solvers.spectral import ldc_lib
        self.device = torch.device(p.device)
        ldc_lib.require_device(self.device)      # no GPU / not gfx950 -> LdcError: there is no CPU fallback
        L = F.lib()
        if L.ldc_fv_version() != F.VERSION:
            raise ldc_lib.LdcError(f"ldc_fv ABI {L.ldc_fv_version()} != {F.VERSION}: rebuild the library")
        f64 = dict(dtype=torch.float64, device=self.device)
        self.rec_cap = max(1, int(p.check_every))
        if self.stretched:                       # shared per (n, L, beta, device); the lid at the stretched face centres
            gridx, lamx, Qx = grid_axis(nx, p.Lx, float(p.grid_stretch), self.device, self.rho)
            gridy, lamy, Qy = grid_axis(ny, p.Ly, float(p.grid_stretch), self.device, self.rho)
            ulid = lid_profile_at(xc, p.Lx, p.lid_velocity, p.corner_treatment, p.corner_smoothing)
            ops = dict(Qx=Qx, lamx=lamx, Qy=Qy, lamy=lamy, gridx=gridx, gridy=gridy)
            if self.separable or self.chip_separable:     # shared per (nx, ny, Lx, Ly, beta, rho, device): the fit couples the axes
                ops["precx"], ops["precy"] = separable_tables(nx, ny, p.Lx, p.Ly, float(p.grid_stretch), self.device,
                                                              self.rho)
        else:
            lamx, Qx = neumann_eig(nx)
            lamy, Qy = neumann_eig(ny)
            ulid = lid_profile(nx, p.Lx, p.lid_velocity, p.corner_treatment, p.corner_smoothing)
            ops = dict(Qx=torch.tensor(Qx, **f64).contiguous(), lamx=torch.tensor(lamx, **f64),
                       Qy=torch.tensor(Qy, **f64).contiguous(), lamy=torch.tensor(lamy, **f64))
        self._ulid_host = np.asarray(ulid, dtype=np.float64)
        self.t = dict(
            ulid=torch.tensor(ulid, **f64), **ops,
            u=torch.zeros(nx * ny, **f64), v=torch.zeros(nx * ny, **f64), p=torch.zeros(nx * ny, **f64),
            mdot=torch.zeros(F.faces(nx, ny), **f64), work=torch.zeros(F.work_len(nx, ny), **f64),
            rec=torch.zeros((self.rec_cap, F.REC_LEN), **f64),
            ctrl=torch.zeros(F.CTRL_LEN, dtype=torch.int64, device=self.device),
            # the mixing kernel's words: every trial has them (a plain trial rides in an accelerated call at depth 0)
            astate=torch.zeros(F.ANDERSON_STATE_LEN, dtype=torch.int64, device=self.device))
        if self.accelerated or self.mixed_chip:
            self.t["hist"] = torch.zeros(F.anderson_hist_len(nx, ny, int(p.anderson_depth)), **f64)
        if self.mixed_chip:
            self.t["mix_scratch"] = torch.zeros(F.wide_anderson_scratch_len(nx, ny, int(p.anderson_depth)), **f64)
        if self.chip:
            self.t["scratch"] = torch.zeros(F.wide_scratch_len(nx, ny), **f64)
        if self.consistent:                       # CG iterations, solves, cap hits, the last solve's count (pfinish)
            self.t["pstats"] = torch.zeros(F.WIDE_PRESSURE_SCRATCH_LEN, dtype=torch.int64, device=self.device)
        if self.consistent_cu:                    # the same four words, added to by the one-CU kernel with ctrl
            self.t["pstats"] = torch.zeros(F.PRESSURE_STATS_LEN, dtype=torch.int64, device=self.device)
        self.linear_budget = int(p.linear_budget)        # grows when a solve overflows it (advance_with_budget)
        self.linear_budget_retries = 0
        self.pressure_budget = int(p.pressure_budget)    # likewise (advance_with_budgets)
        self.pressure_budget_retries = 0
        self._handle = None
        self._wide = None
        self._batch1 = None                      # a "shared" trial alone: the batch object of one it is advanced through
        self.wide_graph = None                   # None: the library's default; set_wide_graph() chooses
        self._handle_tol = None
        self._make_handle(p.tolerance)

    # ---- device handle ----------------------------------------------------------------------------
    def _problem(self, tolerance: float) -> F.Problem:
        p, t = self.params, self.t
        pr = F.Problem(nx=self.nx, ny=self.ny, scheme=SCHEMES[p.convection_scheme], rec_cap=self.rec_cap, warmup=10,
                       max_lin_iters=LINEAR_MAX_ITERATIONS, dx=self.dx_min, dy=self.dy_min, rho=self.rho, mu=self.mu,
                       alpha_uv=float(p.alpha_uv), alpha_p=float(p.alpha_p), lin_tol=float(p.linear_solver_tol),
                       tol=float(tolerance), lid_velocity=float(p.lid_velocity))
        for name in ("ulid", "Qx", "lamx", "Qy", "lamy", "u", "v", "p", "mdot", "work", "rec", "ctrl"):
            setattr(pr, name, t[name].data_ptr())
        return pr

    def _make_handle(self, tolerance: float):
        import torch
        if (self._handle is not None or self._wide is not None) and self._handle_tol == tolerance:
            return
        self._destroy_handle()
        pr = self._problem(tolerance)
        with torch.cuda.device(self.device):
            torch.cuda.current_stream(self.device).synchronize()
            if self._has_cu_handle:
                h = C.c_void_p()
                F.check(F.lib().ldc_fv_create(C.byref(pr), C.byref(h)), "ldc_fv_create")
                self._handle = h
                if self.consistent_cu:
                    F.set_pressure(h, "consistent", float(self.params.pressure_tol), int(self.params.pressure_max_iters),
                                   self.t["pstats"].data_ptr(), self.t["pstats"].numel())
                if self.stretched:
                    F.set_grid(h, self.t["gridx"].data_ptr(), self.t["gridx"].numel(), self.t["gridy"].data_ptr(),
                               self.t["gridy"].numel())
                if self.separable:                # (after the grid: the call refuses a handle without geometry tables)
                    F.set_preconditioner(h, self.t["precx"].data_ptr(), self.t["precx"].numel(),
                                         self.t["precy"].data_ptr(), self.t["precy"].numel())
            if self.chip:
                h = C.c_void_p()
                F.check(F.lib().ldc_fv_wide_create(C.byref(pr), self.t["scratch"].data_ptr(),
                                                   self.t["scratch"].numel(), C.byref(h)), "ldc_fv_wide_create")
                self._wide = h
                if self.wide_graph is not None:
                    F.check(F.lib().ldc_fv_wide_set_graph(h, int(self.wide_graph)), "ldc_fv_wide_set_graph")
                if self.consistent:               # (likewise before the batch of one)
                    F.wide_set_pressure(h, "consistent", float(self.params.pressure_tol),
                                        int(self.params.pressure_max_iters), self.t["pstats"].data_ptr(),
                                        self.t["pstats"].numel())
                if self.chip_tables:              # (the tables of grid_axis; Qx, lamx, Qy, lamy are its eigenpairs already)
                    F.wide_set_grid(h, self.t["gridx"].data_ptr(), self.t["gridx"].numel(), self.t["gridy"].data_ptr(),
                                    self.t["gridy"].numel())
                if self.chip_separable:           # (after the grid: the call refuses a handle without geometry tables)
                    F.wide_set_preconditioner(h, self.t["precx"].data_ptr(), self.t["precx"].numel(),
                                              self.t["precy"].data_ptr(), self.t["precy"].numel())
                if self.mixed_chip:              # (before the batch of one below: a batch copies the block)
                    F.wide_set_anderson(h, self._anderson_block(), self.t["mix_scratch"].data_ptr(),
                                        self.t["mix_scratch"].numel())
                if self.shared:
                    self._batch1 = SharedBatch([self], self.wide_graph)
        self._handle_tol = tolerance

    def _destroy_handle(self):
        if getattr(self, "_batch1", None) is not None:
            self._batch1.close()
            self._batch1 = None
        if self._handle is not None:
            F.lib().ldc_fv_destroy(self._handle)
            self._handle = None
        if getattr(self, "_wide", None) is not None:
            F.lib().ldc_fv_wide_destroy(self._wide)
            self._wide = None
        self._handle_tol = None

    def set_wide_graph(self, on: bool):
        """A ``"chip"`` trial's launches: one replayed hipGraph per iteration (True) or every kernel on its own (False).
        The same kernels in the same order either way (tools/fv_wide_perf.py measures both).  A ``"shared"`` trial
        alone: the same for its batch of one (a batch of several has ``BatchedFVSolver.set_wide_graph``)."""
        if not self.chip:
            raise ValueError("set_wide_graph: only a mapping='chip' trial has launches to capture")
        self.wide_graph = bool(on)
        F.check(F.lib().ldc_fv_wide_set_graph(self._wide, int(self.wide_graph)), "ldc_fv_wide_set_graph")
        if self._batch1 is not None:
            self._batch1.set_graph(self.wide_graph)

    def _require_cu_handle(self, what: str):
        if self._handle is None:
            raise ValueError(f"{what}: a trial of {self.nx} x {self.ny} cells has no one-CU handle "
                             f"(at most {F.MAX_N} cells per axis)")

    def _anderson_block(self) -> F.Anderson:
        """This trial's block of an ``anderson_enqueue`` call (or of ``wide_set_anderson``): its depth and history, depth
        0 for a plain trial."""
        p = self.params
        if not (self.accelerated or self.mixed_chip):
            return F.Anderson(depth=0, start=1, hist=None, hist_len=0, astate=self.t["astate"].data_ptr())
        return F.Anderson(depth=int(p.anderson_depth), start=int(p.anderson_start), hist=self.t["hist"].data_ptr(),
                          hist_len=self.t["hist"].numel(), astate=self.t["astate"].data_ptr())

    def close(self):
        """Release the device handle (the torch tensors go with the object)."""
        self._destroy_handle()

    def __del__(self):
        try:
            self._destroy_handle()
        except Exception:
            pass

    @property
    def handle(self):
        return self._handle

    def _stream(self):
        import torch
        return torch.cuda.current_stream(self.device).cuda_stream

    def start_from(self, other: "FVSolver"):
        """This trial's state from ``other``'s (any FV trial of the same device and the same domain Lx, Ly; its grid and
        its other parameters may differ) by one prolongation (``prolong``): a coarser trial to start from, or a trial of
        this size at another Re to continue from."""
        prolong([(other, self)])

    def _transfer_axes(self):
        """(x, y) tensors [xc | h | d | g] of this trial's mesh (``transfer_axis``: shared per axis, mesh and device); a
        uniform trial is the mesh at beta = 0."""
        p = self.params
        beta = float(p.grid_stretch) if self.stretched else 0.0
        return transfer_axis(self.nx, p.Lx, beta, self.device), transfer_axis(self.ny, p.Ly, beta, self.device)

    def _prolong_tables_job(self, coarse: "FVSolver") -> F.ProlongTablesJob:
        """The job of a ``prolong_tables_enqueue`` call that starts THIS trial from ``coarse``: the coarse state, lid profile
        and centres, this trial's state, geometry tables and centres, the domain and this trial's rho."""
        t, c = self.t, coarse.t
        fx, fy = self._transfer_axes()
        cx, cy = coarse._transfer_axes()
        return F.ProlongTablesJob(
            coarse_u=c["u"].data_ptr(), coarse_v=c["v"].data_ptr(), coarse_p=c["p"].data_ptr(),
            coarse_ulid=c["ulid"].data_ptr(), coarse_xc=cx.data_ptr(), coarse_yc=cy.data_ptr(),
            fine_u=t["u"].data_ptr(), fine_v=t["v"].data_ptr(), fine_p=t["p"].data_ptr(), fine_mdot=t["mdot"].data_ptr(),
            fine_x_grid=fx[self.nx:].data_ptr(), fine_y_grid=fy[self.ny:].data_ptr(), fine_xc=fx.data_ptr(),
            fine_yc=fy.data_ptr(), Lx=float(self.params.Lx), Ly=float(self.params.Ly), rho=float(self.rho),
            coarse_nx=coarse.nx, coarse_ny=coarse.ny, fine_nx=self.nx, fine_ny=self.ny)

    # ---- state access (tests, tools) -------------------------------------------------------------------
    def set_state(self, u, v, p, mdot):
        """Overwrite the device state: u, v, p per cell (c = j*nx + i), mdot in the [fx | fy] face layout."""
        import torch
        for name, val in (("u", u), ("v", v), ("p", p), ("mdot", mdot)):
            self.t[name].copy_(torch.as_tensor(np.asarray(val, dtype=np.float64).ravel()))
        self.t["ctrl"].zero_()
        self.t["astate"].zero_()
        self._reset_budgets()
        self._post = None

    def _reset_budgets(self):
        """The budgets of a new solve, and the statistics words of its pressure solves at zero."""
        p = self.params
        self.linear_budget, self.linear_budget_retries = int(p.linear_budget), 0
        self.pressure_budget, self.pressure_budget_retries = int(p.pressure_budget), 0
        if self.consistent or self.consistent_cu:
            self.t["pstats"].zero_()

    def state(self) -> dict:
        return {k: self.t[k].cpu().numpy().copy() for k in ("u", "v", "p", "mdot")}

    def counters(self) -> dict:
        c = self.t["ctrl"].cpu().numpy()
        a = self.t["astate"].cpu().numpy()
        out = dict(done=int(c[F.CTRL_DONE]), iterations=int(c[F.CTRL_ITER]), nan=int(c[F.CTRL_NAN]),
                   linear_giveups=int(c[F.CTRL_GIVEUP]), linear_iterations=int(c[F.CTRL_LIN_ITERS]),
                   momentum_solves=int(c[F.CTRL_SOLVES]), anderson_fallbacks=int(a[F.ASTATE_FALLBACKS]),
                   linear_budget_retries=int(self.linear_budget_retries))
        if self.consistent:
            ps = self.t["pstats"].cpu().numpy()
            out.update(pressure_iterations=int(ps[F.PSTAT_ITERS]), pressure_solves=int(ps[F.PSTAT_SOLVES]),
                       pressure_caps=int(ps[F.PSTAT_CAPS]), pressure_last=int(ps[F.PSTAT_LAST]),
                       pressure_budget_retries=int(self.pressure_budget_retries))
        if self.consistent_cu:                    # (no budget on this mapping: no retries to report)
            ps = self.t["pstats"].cpu().numpy()
            out.update(pressure_iterations=int(ps[F.PSTAT_ITERS]), pressure_solves=int(ps[F.PSTAT_SOLVES]),
                       pressure_caps=int(ps[F.PSTAT_CAPS]), pressure_last=int(ps[F.PSTAT_LAST]))
        return out

    def step_debug(self, which=F.DBG) -> dict:
        """One iteration through ldc_fv_step_debug; returns the named intermediates (include/ldc_fv.h)."""
        import torch
        n, nf = self.n_cells, F.faces(self.nx, self.ny)
        size = dict(grad_p=2 * n, diag=5 * n, b=2 * n, mdot_star=nf, mdot=nf)
        bufs = {k: torch.full((size.get(k, n),), float("nan"), dtype=torch.float64, device=self.device) for k in which}
        ptrs = (C.c_void_p * len(F.DBG))(*[bufs[k].data_ptr() if k in bufs else None for k in F.DBG])
        mask = sum(1 << F.DBG.index(k) for k in which)
        with torch.cuda.device(self.device):
            F.check(F.lib().ldc_fv_step_debug(self._handle, mask, ptrs, C.c_void_p(self._stream())), "ldc_fv_step_debug")
            torch.cuda.current_stream(self.device).synchronize()
        return {k: b.cpu().numpy() for k, b in bufs.items()}

    # ---- LidDrivenCavitySolver hooks --------------------------------------------------------------------
    def _begin(self, tolerance: float):
        """A new solve: the trial's control words start at zero (latch, iteration count, NaN flag, the linear-solver
        counters), the fields stay.  Like the reference's loop (base.py:243) and the spectral solvers, every
        ``solve()`` counts from 0 on the current state, with its own warm-up, history and iteration count."""
        self._make_handle(tolerance)
        self.t["ctrl"].zero_()
        self.t["astate"].zero_()                 # (the mixing history starts over with the count: include/ldc_fv.h)
        self._reset_budgets()
        self._post = None

    def _wide_step(self, m: int, budget: int, pressure_budget: int = None):
        """One wide enqueue of up to ``m`` iterations at ``budget`` and ONE wait (``advance_with_budget``'s step; with a
        ``pressure_budget``, ``advance_with_budgets``'s: the overflow word then tells which budget was too small)."""
        import torch
        from solvers.spectral import ldc_lib
        index = torch.cuda.current_device() if self.device.index is None else self.device.index
        with torch.cuda.device(self.device):
            start = int(self.t["ctrl"][F.CTRL_ITER].item())
            if pressure_budget is not None:
                F.check(F.lib().ldc_fv_wide_set_pressure_budget(self._wide, int(pressure_budget)),
                        "ldc_fv_wide_set_pressure_budget")
            with ldc_lib.resident_lock(index):
                F.check(F.lib().ldc_fv_wide_enqueue(self._wide, int(m), int(budget), C.c_void_p(self._stream())),
                        "ldc_fv_wide_enqueue")
                c = self.t["ctrl"].cpu().numpy()          # (synchronises the stream)
            total = int(c[F.CTRL_ITER])
            rows = self.t["rec"][: total - start].cpu().numpy().copy()
            overflow = int(self.t["scratch"][:1].view(torch.int64).item())
        return rows, int(c[F.CTRL_DONE]), int(c[F.CTRL_NAN]), total, overflow

    def _advance(self, n_iters: int):
        n_iters = max(1, min(int(n_iters), self.rec_cap))
        if self.shared:
            rows, done, nan, total = self._batch1.advance([n_iters])[0]
            if nan:
                F.check(F.lib().ldc_fv_wide_status(self._wide), f"FV trial at iteration {total}")
            return rows, done, total
        if self.chip:
            start = int(self.t["ctrl"][F.CTRL_ITER].item())
            if self.consistent:
                rows, done, nan, total, budgets, both = advance_with_budgets(
                    self._wide_step, start, n_iters, (self.linear_budget, self.pressure_budget),
                    (LINEAR_MAX_ITERATIONS, int(self.params.pressure_max_iters)))
                self.linear_budget, self.pressure_budget = budgets
                retries, more = both
                self.pressure_budget_retries += more
            else:
                rows, done, nan, total, self.linear_budget, retries = advance_with_budget(
                    self._wide_step, start, n_iters, self.linear_budget, LINEAR_MAX_ITERATIONS)
            self.linear_budget_retries += retries
            if nan:
                F.check(F.lib().ldc_fv_wide_status(self._wide), f"FV trial at iteration {total}")
            return rows, done, total
        rows, done, nan, total = advance([self], n_iters)[0]
        if nan:
            F.check(F.lib().ldc_fv_status(self._handle), f"FV trial at iteration {total}")
        return rows, done, total

    def _finalize_fields(self):
        st = self.state()
        self.fields.u, self.fields.v, self.fields.p = st["u"], st["v"], st["p"]

    # ---- vortex metrics (reference base.py:569-760), on the host once per solve ----------------------------
    def _ghost_gradient(self, f2, bc_lid):
        g = np.zeros((self.ny + 2, self.nx + 2))
        g[1:-1, 1:-1] = f2
        g[0, 1:-1] = -f2[0, :]
        g[-1, 1:-1] = 2 * bc_lid - f2[-1, :]
        g[1:-1, 0] = -f2[:, 0]
        g[1:-1, -1] = -f2[:, -1]
        return ((g[1:-1, 2:] - g[1:-1, :-2]) / (2 * self.dx_min), (g[2:, 1:-1] - g[:-2, 1:-1]) / (2 * self.dy_min))

    def _gauss_gradient(self, f2, lid):
        """(d f / dx, d f / dy) on the stretched grid: (f_e - f_w) / hx with g-weighted face values, 0 on the walls and
        ``lid`` (nx values) on the lid: the rule of the kernel's record (include/ldc_fv.h)."""
        ny, nx = self.shape_full
        gx, gy = self._gxf[1:-1][None, :], self._gyf[1:-1][:, None]
        fx, fy = np.zeros((ny, nx + 1)), np.zeros((ny + 1, nx))
        fx[:, 1:-1] = gx * f2[:, 1:] + (1.0 - gx) * f2[:, :-1]
        fy[1:-1, :] = gy * f2[1:, :] + (1.0 - gy) * f2[:-1, :]
        fy[-1, :] = lid
        return (fx[:, 1:] - fx[:, :-1]) / self._hx[None, :], (fy[1:, :] - fy[:-1, :]) / self._hy[:, None]

    def _vorticity(self) -> np.ndarray:
        U, V = self.fields.u.reshape(self.shape_full), self.fields.v.reshape(self.shape_full)
        if getattr(self, "stretched", False):
            dvdx, _ = self._gauss_gradient(V, 0.0)
            _, dudy = self._gauss_gradient(U, self._ulid_host)
            return dvdx - dudy
        dvdx, _ = self._ghost_gradient(V, 0.0)
        _, dudy = self._ghost_gradient(U, float(getattr(self.params, "lid_velocity", 1.0)))
        return dvdx - dudy

    def _streamfunction(self, omega):
        """psi from the 5-point Dirichlet Poisson problem on the interior cells (base.py:569-630)."""
        from scipy.sparse import diags
        from scipy.sparse.linalg import spsolve
        ny, nx = self.shape_full
        if getattr(self, "stretched", False):
            A = stretched_streamfunction_matrix(self._dxf, self._dyf)
            psi = np.zeros((ny, nx))
            psi[1:-1, 1:-1] = spsolve(A, -omega[1:-1, 1:-1].ravel()).reshape(ny - 2, nx - 2)
            return psi
        dx, dy = self.dx_min, self.dy_min
        ni = (ny - 2) * (nx - 2)
        cx, cy = 1.0 / (dx * dx), 1.0 / (dy * dy)
        dmain = np.full(ni, -2.0 * (cx + cy))
        dxo = np.full(ni - 1, cx)
        dyo = np.full(ni - (nx - 2), cy)
        for i in range(1, ny - 2):
            idx = i * (nx - 2) - 1
            if idx < len(dxo):
                dxo[idx] = 0.0
        A = diags([dyo, dxo, dmain, dxo, dyo], [-(nx - 2), -1, 0, 1, (nx - 2)], format="csr")
        psi = np.zeros((ny, nx))
        psi[1:-1, 1:-1] = spsolve(A, -omega[1:-1, 1:-1].ravel()).reshape(ny - 2, nx - 2)
        return psi

    def compute_vortex_metrics(self) -> dict:
        # (getattr: tests/fv_post_numpy.py calls this method on a bare namespace that has only the host branch's parameters)
        if getattr(self.params, "streamfunction", "reference") in WALL_RULES:
            return self._wall_vortex_metrics()
        if self.params.vortex_metrics in ("device", "chip"):
            return self._device_vortex_metrics()
        omega = self._vorticity()
        psi = self._streamfunction(omega)
        xs, ys = np.sort(np.unique(self.fields.x)), np.sort(np.unique(self.fields.y))
        imin = np.unravel_index(np.argmin(psi), psi.shape)
        imax = np.unravel_index(np.argmax(np.abs(omega)), omega.shape)
        out = dict(psi_min=float(psi[imin]), psi_min_x=float(xs[imin[1]]), psi_min_y=float(ys[imin[0]]),
                   omega_center=float(omega[imin]), omega_max=float(omega[imax]),
                   omega_max_x=float(xs[imax[1]]), omega_max_y=float(ys[imax[0]]))
        X, Y = np.meshgrid(xs, ys)
        regions = {"BR": (X > 0.5) & (Y < 0.5), "BL": (X < 0.5) & (Y < 0.5), "TL": (X < 0.5) & (Y > 0.5)}
        for name, mask in regions.items():
            k = np.unravel_index(np.argmax(np.where(mask, psi, -np.inf)), psi.shape)
            if psi[k] > 0:
                out.update({f"psi_{name}": float(psi[k]), f"psi_{name}_x": float(xs[k[1]]),
                            f"psi_{name}_y": float(ys[k[0]])})
            else:
                out.update({f"psi_{name}": 0.0, f"psi_{name}_x": 0.0, f"psi_{name}_y": 0.0})
        return out

    # ---- the same on the device (ldc_fv_post_enqueue, ldc_fv_wide_post_enqueue) ------------------------------
    def _device_vortex_metrics(self) -> dict:
        """The host branch's dict from the trial's result block: the block ``postprocess`` left (a batch post-processes
        its trials together), or one of a launch of its own."""
        if self._post is None:
            postprocess([self])
        r, self._post = self._post, None
        if r[F.POST_NONFINITE] != 0:
            raise FloatingPointError("vortex metrics: omega or psi is not finite")
        xs, ys = np.sort(np.unique(self.fields.x)), np.sort(np.unique(self.fields.y))
        xy = lambda c: (float(xs[int(c) % self.nx]), float(ys[int(c) // self.nx]))        # noqa: E731
        (x0, y0), (x1, y1) = xy(r[F.POST_PSI_MIN_CELL]), xy(r[F.POST_OMEGA_MAX_CELL])
        out = dict(psi_min=float(r[F.POST_PSI_MIN]), psi_min_x=x0, psi_min_y=y0,
                   omega_center=float(r[F.POST_OMEGA_CENTER]), omega_max=float(r[F.POST_OMEGA_MAX]),
                   omega_max_x=x1, omega_max_y=y1)
        for q, name in enumerate(("BR", "BL", "TL")):
            val, cell = float(r[F.POST_PSI_BR + q]), r[F.POST_PSI_BR_CELL + q]
            if val > 0:
                x, y = xy(cell)
                out.update({f"psi_{name}": val, f"psi_{name}_x": x, f"psi_{name}_y": y})
            else:
                out.update({f"psi_{name}": 0.0, f"psi_{name}_x": 0.0, f"psi_{name}_y": 0.0})
        return out

    # ---- the wall rule (ldc_fv_wall_post_enqueue) ---------------------------------------------------------------
    def _wall_job(self, result_ptr: int) -> F.WallJob:
        """This trial's job of a ``wall_post_enqueue`` call: the state, the tables of its sizes (shared per device), its own
        psi, omega and scratch, and the row of the call's result tensor."""
        import torch
        dev, t = self.device, self.t
        lamx, Cx = wall_eig(self.nx, dev)
        lamy, Cy = wall_eig(self.ny, dev)
        for name, size in (("psi", self.n_cells), ("omega", self.n_cells),
                           ("wall_scratch", F.wall_scratch_len(self.nx, self.ny))):
            if name not in t:
                t[name] = torch.zeros(size, dtype=torch.float64, device=dev)
        ix_lt, ix_gt, jy_lt, jy_gt = self._mask_bounds
        return F.WallJob(u=t["u"].data_ptr(), v=t["v"].data_ptr(), ulid=t["ulid"].data_ptr(), Cx=Cx.data_ptr(),
                         lamx=lamx.data_ptr(), Cy=Cy.data_ptr(), lamy=lamy.data_ptr(), psi=t["psi"].data_ptr(),
                         omega=t["omega"].data_ptr(), scratch=t["wall_scratch"].data_ptr(), result=result_ptr,
                         dx=self.dx_min, dy=self.dy_min, nx=self.nx, ny=self.ny, ix_lt=ix_lt, ix_gt=ix_gt, jy_lt=jy_lt,
                         jy_gt=jy_gt, refine=int(self.params.vortex_refine == "quadratic"), pad=0)

    def _wall_stretched_job(self, result_ptr: int) -> F.WallStretchedJob:
        """This trial's job of a ``wall_stretched_post_enqueue`` call: the state, the geometry tables its handle reads, the
        post tables of its axes (shared per mesh and device), its own psi, omega and scratch, and the row of the call's
        result tensor."""
        import torch
        dev, t, p = self.device, self.t, self.params
        postx = wall_stretched_axis(self.nx, p.Lx, float(p.grid_stretch), dev)
        posty = wall_stretched_axis(self.ny, p.Ly, float(p.grid_stretch), dev)
        for name, size in (("psi", self.n_cells), ("omega", self.n_cells),
                           ("wall_scratch", F.wall_scratch_len(self.nx, self.ny))):
            if name not in t:
                t[name] = torch.zeros(size, dtype=torch.float64, device=dev)
        ix_lt, ix_gt, jy_lt, jy_gt = self._mask_bounds
        return F.WallStretchedJob(u=t["u"].data_ptr(), v=t["v"].data_ptr(), ulid=t["ulid"].data_ptr(),
                                  x_grid=t["gridx"].data_ptr(), y_grid=t["gridy"].data_ptr(), x_post=postx.data_ptr(),
                                  y_post=posty.data_ptr(), psi=t["psi"].data_ptr(), omega=t["omega"].data_ptr(),
                                  scratch=t["wall_scratch"].data_ptr(), result=result_ptr, nx=self.nx, ny=self.ny,
                                  ix_lt=ix_lt, ix_gt=ix_gt, jy_lt=jy_lt, jy_gt=jy_gt,
                                  refine=int(p.vortex_refine == "quadratic"), pad=0)

    def _wall_vortex_metrics(self) -> dict:
        """The metrics dict of a wall trial from its result block: the primary minimum and the corners from the groups
        (refined, or the cell's own values), under the existing rule that a corner counts when its grid value is > 0;
        ``omega_max`` stays on the grid.  ``omega_BR`` / ``omega_BL`` / ``omega_TL`` are filled."""
        if self._post is None or len(self._post) < F.WALL_RESULT_LEN:
            postprocess([self])
        r, self._post = self._post, None
        if r[F.POST_NONFINITE] != 0:
            raise FloatingPointError("vortex metrics: omega or psi is not finite")
        groups = r[F.POST_RESULT_LEN: F.WALL_RESULT_LEN].reshape(4, F.WALL_GROUP_LEN)
        refined = self.params.vortex_refine == "quadratic"
        self.vortex_refine_status = tuple(int(g[F.WALL_STATUS]) for g in groups) if refined else None
        cmax = int(r[F.POST_OMEGA_MAX_CELL])
        xs, ys = np.sort(np.unique(self.fields.x)), np.sort(np.unique(self.fields.y))      # (as the other two routes)
        g = groups[0]
        out = dict(psi_min=float(g[F.WALL_PSI]), psi_min_x=float(g[F.WALL_X]), psi_min_y=float(g[F.WALL_Y]),
                   omega_center=float(g[F.WALL_OMEGA]), omega_max=float(r[F.POST_OMEGA_MAX]),
                   omega_max_x=float(xs[cmax % self.nx]), omega_max_y=float(ys[cmax // self.nx]))
        for q, name in enumerate(("BR", "BL", "TL")):
            g = groups[1 + q]
            keep = float(r[F.POST_PSI_BR + q]) > 0
            vals = (g[F.WALL_PSI], g[F.WALL_OMEGA], g[F.WALL_X], g[F.WALL_Y]) if keep else (0.0, 0.0, 0.0, 0.0)
            out.update({f"psi_{name}": float(vals[0]), f"omega_{name}": float(vals[1]), f"psi_{name}_x": float(vals[2]),
                        f"psi_{name}_y": float(vals[3])})
        return out

    def _post_field(self, name) -> np.ndarray:
        if self.stretched and not self.stretched_wall:      # the reference's rule: on the host, from the current device state
            self._finalize_fields()
            omega = self._vorticity()
            return omega if name == "omega" else self._streamfunction(omega)
        postprocess([self])
        self._post = None
        return self.t[name].cpu().numpy().reshape(self.shape_full).copy()

    def streamfunction(self) -> np.ndarray:
        """psi (ny, nx) of the current device state, computed on the device."""
        return self._post_field("psi")

    def vorticity(self) -> np.ndarray:
        """omega (ny, nx) of the current device state, computed on the device."""
        return self._post_field("omega")

    # ---- Ghia centrelines: linear interpolation, as the reference plots FV fields ----------------------------
    def ghia_error(self) -> dict:
        ny, nx = self.shape_full
        x, y = self.fields.x.reshape(ny, nx)[0, :], self.fields.y.reshape(ny, nx)[:, 0]
        U, V = self.fields.u.reshape(ny, nx).T, self.fields.v.reshape(ny, nx).T        # -> [ix, iy]
        return _val.ghia_centerline_error(x, y, U, V, int(self.params.Re), interpolation="linear")
