"""Host tables of the finite-volume solver and their one device cache.

What the kernels read beside a trial's own state is computed here, on the host, once per mesh: the lid profile at the face
centres, the vertices and per-axis geometry tables of ``grid="tanh"`` (``ldc_fv_set_grid``, ``ldc_fv_wide_set_grid``), the
eigenpairs of the 1-D operators behind every exact solve (the Neumann Laplacian of the pressure correction, uniform and
generalised; the Dirichlet ones of the two streamfunction rules and of the wall rule on a stretched mesh), the fit and the
tables of the separable preconditioner (``ldc_fv_set_preconditioner``, ``ldc_fv_wide_set_preconditioner``) and the tables of
the transfers that read both grids (``ldc_fv_prolong_tables_enqueue`` and its chip twin).  The ``*_host`` builders return
NumPy arrays; the getters below them return float64 tensors on a device through ``cached_tables``, so trials of equal axes
share one decomposition and one upload."""
from __future__ import annotations

import numpy as np


# ---- the device cache ---------------------------------------------------------------------------------------------
_tables = {}


def device_index(device) -> int:
    """The ordinal of a torch device: its own, or the current one of a bare "cuda" (0 where the type has no ordinals)."""
    import torch
    if device.index is not None:
        return device.index
    return torch.cuda.current_device() if device.type == "cuda" else 0


def cached_tables(key, device, build):
    """The arrays of ``build()`` as contiguous float64 tensors on ``device``, built and uploaded once per ``key`` (which
    names the table and its arguments) and device: the key gets (device.type, device_index(device)) appended."""
    import torch
    device = torch.device(device)
    key = tuple(key) + (device.type, device_index(device))
    if key not in _tables:
        _tables[key] = tuple(torch.tensor(a, dtype=torch.float64, device=device).contiguous() for a in build())
    return _tables[key]


# ---- the lid ------------------------------------------------------------------------------------------------------
def lid_profile_at(xf, Lx=1.0, lid_velocity=1.0, corner_treatment="none", corner_smoothing=0.15) -> np.ndarray:
    """u on the lid faces with the centres ``xf`` of any mesh, evaluated as the reference's mesh builder does
    (simple_structured.py:244-262: it evaluates the lid at the face centre)."""
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


def lid_profile(nx, Lx=1.0, lid_velocity=1.0, corner_treatment="none", corner_smoothing=0.15) -> np.ndarray:
    """``lid_profile_at`` the face centres of ``nx`` equal cells."""
    x = np.linspace(0, Lx, nx + 1)
    return lid_profile_at(0.5 * (x[:-1] + x[1:]), Lx, lid_velocity, corner_treatment, corner_smoothing)


# ---- meshes and their geometry tables -----------------------------------------------------------------------------
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


def mask_bounds(xs, ys):
    """The corner regions of ``compute_vortex_metrics`` as index bounds on the sorted cell-centre coordinates:
    xs < 0.5 is i < ix_lt, xs > 0.5 is i >= ix_gt, likewise ys (absolute coordinates, as the reference's masks)."""
    return (int(np.count_nonzero(xs < 0.5)), int(xs.size - np.count_nonzero(xs > 0.5)),
            int(np.count_nonzero(ys < 0.5)), int(ys.size - np.count_nonzero(ys > 0.5)))


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


# ---- eigenpairs of the 1-D operators ------------------------------------------------------------------------------
def neumann_eig(n: int):
    """(eigenvalues ascending, eigenvectors as columns) of the 1-D Neumann second difference; index 0 = zero mode."""
    T = 2 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1)
    T[0, 0] = T[-1, -1] = 1.0
    lam, Q = np.linalg.eigh(T)
    assert abs(lam[0]) < 1e-10 and lam[1] > 1e-6, "Neumann Laplacian: one zero mode, first"
    return lam, Q


def _neumann_eigh(w, m, rho, L):
    """(eigenvalues ascending, eigenvectors as columns) of K q = lam M q with Q^T M Q = I: K the 1-D Neumann stiffness of
    n cells with the weights ``w`` of the n - 1 inner faces, M = diag(m); index 0 = zero mode."""
    from scipy.linalg import eigh
    n = m.size
    K = np.zeros((n, n))
    i = np.arange(n - 1)
    K[i, i] += w
    K[i + 1, i + 1] += w
    K[i, i + 1] -= w
    K[i + 1, i] -= w
    lam, Q = eigh(K, np.diag(m))
    # (the first mode above zero stays near rho (pi / L)^2 whatever n is, while lam[-1] grows like 1 / h_min^2: lam[1] /
    # lam[-1] falls below 1e-6 from about 600 cells per axis on, and at 256 with beta = 2.5, so lam[1] is held against the
    # former)
    assert abs(lam[0]) < 1e-9 * lam[-1] and lam[1] > 0.5 * rho * (np.pi / L) ** 2, "Neumann stiffness: one zero mode, first"
    return lam, Q


def generalised_eig_host(h, d, rho=1.0):
    """The eigenpairs of K q = lam H q, Q^T H Q = I: K the 1-D Neumann stiffness with the weights rho / d of the inner
    faces, H = diag(h).  With them the operator Hy (x) Kx + Ky (x) Hx of the pressure correction on a tensor grid is solved
    by the four products of the uniform case, divisor lamy[a] + lamx[b]."""
    return _neumann_eigh(rho / d[1:h.size], h, rho, h.sum())


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


def sine_eig_host(m: int):
    """(eigenvalues ascending, eigenvectors as columns) of the m x m Dirichlet second difference tridiag(-1, 2, -1),
    analytic: S[k, j] = sqrt(2 / (m + 1)) sin(pi (k + 1)(j + 1) / (m + 1)), lam[k] = 2 - 2 cos(pi (k + 1) / (m + 1))."""
    k = np.arange(1, m + 1, dtype=np.float64)
    S = np.sqrt(2.0 / (m + 1)) * np.sin(np.pi * np.outer(k, k) / (m + 1))
    return 2.0 - 2.0 * np.cos(np.pi * k / (m + 1)), S


def wall_eig_host(n: int):
    """(eigenvalues ascending, eigenvectors as columns) of the n x n second difference tridiag(-1, 2, -1) with 3 in both
    corners (the ghost cell is minus its neighbour: zero on the wall FACE), analytic: C[j, k] = sqrt(2 / n)
    sin(pi (k + 1)(j + 1/2) / n), the last column divided by sqrt(2); lam[k] = 2 - 2 cos(pi (k + 1) / n).  Not symmetric."""
    k = np.arange(1, n + 1, dtype=np.float64)
    j = np.arange(n, dtype=np.float64) + 0.5
    Cm = np.sqrt(2.0 / n) * np.sin(np.pi * np.outer(j, k) / n)
    Cm[:, -1] /= np.sqrt(2.0)
    return 2.0 - 2.0 * np.cos(np.pi * k / n), Cm


# ---- the separable preconditioner ---------------------------------------------------------------------------------
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
    """The eigenpairs of K q = lam M q, Q^T M Q = I: K the 1-D Neumann stiffness with the weights rho a_f / d of the inner
    faces, a_f[k] = g[k] a[k] + (1 - g[k]) a[k-1] (the rule that takes D to a face), M = diag(h a).  (Not
    ``generalised_eig_host`` at a = 1 in floating point: g + (1 - g) is not exactly 1.)"""
    n = h.size
    af = g[1:n] * a[1:] + (1.0 - g[1:n]) * a[:-1]
    return _neumann_eigh(rho * af / d[1:n], h * a, rho, h.sum())


def separable_tables_host(nx, ny, Lx, Ly, beta, rho=1.0):
    """The two tables of ``ldc_fv_set_preconditioner`` for a tanh grid, [a | lam | Q (row-major)] per axis (y: b for a)."""
    _, hx, dxf, gxf = axis_tables(tanh_vertices(nx, Lx, beta))
    _, hy, dyf, gyf = axis_tables(tanh_vertices(ny, Ly, beta))
    a, b = separable_fit(hx, dxf, hy, dyf)
    lamx, Qx = separable_axis_host(hx, dxf, gxf, a, rho)
    lamy, Qy = separable_axis_host(hy, dyf, gyf, b, rho)
    return (np.concatenate([a, lamx, np.ascontiguousarray(Qx).ravel()]),
            np.concatenate([b, lamy, np.ascontiguousarray(Qy).ravel()]))


# ---- the same on a device, shared by the trials of equal axes ------------------------------------------------------
def grid_axis(n: int, L: float, beta: float, device, rho=1.0):
    """The device tensors of one axis of a tanh grid, cached per (n, L, beta, rho, device): (table [h | d | g], lam, Q).
    Trials of equal axes share one upload and one eigen-decomposition."""
    def build():
        _, h, d, g = axis_tables(tanh_vertices(n, L, beta))
        return (np.concatenate([h, d, g]),) + generalised_eig_host(h, d, rho)
    return cached_tables(("grid_axis", int(n), float(L), float(beta), float(rho)), device, build)


def transfer_axis(n: int, L: float, beta: float, device):
    """The device tensor of one axis of ``ldc_fv_prolong_tables_enqueue``, [xc (n) | h (n) | d (n + 1) | g (n + 1)], cached per
    (n, L, beta, device): the cell centres, then the geometry table of ``ldc_fv_set_grid``.  ``beta`` = 0 is an equally
    spaced axis (a uniform trial): the same table of its vertices k L / n, and no eigen-decomposition either way."""
    return cached_tables(("transfer_axis", int(n), float(L), float(beta)), device,
                         lambda: (np.concatenate(axis_tables(tanh_vertices(n, L, beta))),))[0]


def wall_stretched_axis(n: int, L: float, beta: float, device):
    """The device tensor of one axis' post table of ``ldc_fv_wall_stretched_post_enqueue``, [xc | lam | Q (row-major)],
    cached per (n, L, beta, device): one eigen-decomposition and one upload per axis and mesh."""
    def build():
        xc, h, d, _ = axis_tables(tanh_vertices(n, L, beta))
        lam, Q = dirichlet_eig_host(h, d)
        return (np.concatenate([xc, lam, np.ascontiguousarray(Q).ravel()]),)
    return cached_tables(("wall_stretched_axis", int(n), float(L), float(beta)), device, build)[0]


def separable_tables(nx: int, ny: int, Lx: float, Ly: float, beta: float, device, rho=1.0):
    """The device tensors of ``separable_tables_host``, cached per (nx, ny, Lx, Ly, beta, rho, device): the fit couples the
    axes, so the key names both.  Trials of equal meshes share one upload and two eigen-decompositions."""
    return cached_tables(("separable_tables", int(nx), int(ny), float(Lx), float(Ly), float(beta), float(rho)), device,
                         lambda: separable_tables_host(nx, ny, Lx, Ly, beta, rho))


def sine_eig(m: int, device=None):
    """``sine_eig_host(m)``; with a ``device`` as float64 tensors there, cached per (m, device): trials of equal size
    share one upload."""
    if device is None:
        return sine_eig_host(m)
    return cached_tables(("sine_eig", int(m)), device, lambda: sine_eig_host(m))


def wall_eig(n: int, device=None):
    """``wall_eig_host(n)``; with a ``device`` as float64 tensors there, cached per (n, device), as ``sine_eig``."""
    if device is None:
        return wall_eig_host(n)
    return cached_tables(("wall_eig", int(n)), device, lambda: wall_eig_host(n))
