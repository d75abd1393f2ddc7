"""NumPy statement of the wall-anchored finite-volume post-processing on a stretched tensor grid (include/ldc_fv.h,
ldc_fv_wall_stretched_post_enqueue), shared by tests/test_fv_wall_stretched_cpu.py and tests/test_gpu_fv_wall_stretched.py:
the Dirichlet generalised eigenpairs, omega by the Gauss rule, psi with psi = 0 on the wall faces by fast diagonalisation
(fp64) and by a banded Cholesky factorisation of the same operator in long double, the extrema rule (that of
tests/fv_wall_post_numpy.py), the 3 x 3 quadratic refinement with unequal spacing, its floors and statuses, the result block
and the metrics read off it; and the manufactured fields, constructed states and error bounds of the tests.

An axis is the tuple ``(xc, h, d, g)`` of ``fv_stretched_numpy.axis_tables``: centres and widths (n), per face k = 0 .. n the
distance d between the centres it separates (walls: h / 2) and the weight g of the cell behind it."""
import numpy as np

import fv_wall_post_numpy as W
from fv_stretched_numpy import axis_tables, tanh_vertices

LD = np.longdouble
EPS, BIG = W.EPS, W.BIG
RESULT_LEN, POST_LEN, GROUP_LEN = W.RESULT_LEN, W.POST_LEN, W.GROUP_LEN
G_X, G_Y, G_PSI, G_OMEGA, G_STATUS, G_SX, G_SY = range(7)
GROUPS = W.GROUPS
LAUNCH_MAX = 32

# (nx, ny) of the GPU tests: the minimum; odd with GEMM edge fill; 37 x 50; tile remainders on either axis; above the one-CU
# limit with several work-groups per sweep; the maximum
GPU_SHAPES = [(8, 8), (13, 17), (37, 50), (64, 16), (16, 64), (257, 24), (1024, 9)]
BETAS = (0.0, 1.5, 2.5)


def axis(n, L=1.0, beta=1.5):
    return axis_tables(tanh_vertices(n, L, beta))


def grid_table(ax):
    """[h | d | g]: the table of ldc_fv_set_grid."""
    return np.concatenate([ax[1], ax[2], ax[3]])


# ---- tables -------------------------------------------------------------------------------------------------------
def dirichlet_stiffness(d, dtype=np.float64):
    """K^D (n x n): the 1-D stiffness with the weights 1 / d[k] on all n + 1 faces; the wall faces (d = h / 2) enter the
    diagonal only: psi = 0 on the wall face."""
    w = dtype(1) / np.asarray(d).astype(dtype)
    n = w.size - 1
    K = np.zeros((n, n), dtype=dtype)
    i = np.arange(n)
    K[i, i] = w[:-1] + w[1:]
    K[i[:-1], i[:-1] + 1] = -w[1:n]
    K[i[:-1] + 1, i[:-1]] = -w[1:n]
    return K


def dirichlet_eig(ax, tridiagonal=False):
    """(lam ascending, Q as columns) of K^D q = lam H q with Q^T H Q = I, H = diag(h).  Every lam > 0.  ``tridiagonal``: the
    same pairs from the symmetrised pencil, H^-1/2 K^D H^-1/2 = Y Lam Y^T and Q = H^-1/2 Y, in O(n^2): for the axes of the GPU
    tests that are longer than any the solver decomposes (it takes the dense route, up to 256 cells)."""
    from scipy.linalg import eigh, eigh_tridiagonal
    K = dirichlet_stiffness(ax[2])
    if tridiagonal:
        s = 1.0 / np.sqrt(ax[1])
        lam, Y = eigh_tridiagonal(np.diag(K) * s * s, np.diag(K, 1) * s[:-1] * s[1:])
        Q = s[:, None] * Y
    else:
        lam, Q = eigh(K, np.diag(ax[1]))
    assert lam[0] > 0
    return lam, Q


def post_table(ax, eig=None):
    """[xc | lam | Q (row-major, column k the k-th vector)]: one axis' post table."""
    lam, Q = dirichlet_eig(ax) if eig is None else eig
    return np.concatenate([ax[0], lam, np.ascontiguousarray(Q).ravel()])


# ---- fields -------------------------------------------------------------------------------------------------------
def omega(u, v, ulid, ax, ay):
    """omega (ny, nx) by the Gauss rule: (v_e - v_w) / hx - (u_n - u_s) / hy; inner faces g f_N + (1 - g) f_P, walls 0, the lid
    the profile ``ulid``."""
    U, V = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    ny, nx = U.shape
    gx, gy = ax[3][1:-1][None, :], ay[3][1:-1][:, None]
    vf = np.zeros((ny, nx + 1))
    vf[:, 1:-1] = gx * V[:, 1:] + (1.0 - gx) * V[:, :-1]
    uf = np.zeros((ny + 1, nx))
    uf[1:-1, :] = gy * U[1:, :] + (1.0 - gy) * U[:-1, :]
    uf[-1, :] = ulid
    return (vf[:, 1:] - vf[:, :-1]) / ax[1][None, :] - (uf[1:, :] - uf[:-1, :]) / ay[1][:, None]


def volume_rhs(om, ax, ay):
    """B = V . omega, V = hx_i hy_j."""
    return (ax[1][None, :] * ay[1][:, None]) * om


def psi_solve(om, ax, ay, eigs=None):
    """psi (ny, nx) from (Hy (x) Kx^D + Ky^D (x) Hx) psi = V . omega on all cells:
    Qy ((Qy^T B Qx) / (lamy[a] + lamx[b])) Qx^T.  ``eigs``: ((lamx, Qx), (lamy, Qy)) in place of ``dirichlet_eig``."""
    (lx, Qx), (ly, Qy) = (dirichlet_eig(ax), dirichlet_eig(ay)) if eigs is None else eigs
    h = (Qy.T @ volume_rhs(om, ax, ay) @ Qx) / (ly[:, None] + lx[None, :])
    return Qy @ h @ Qx.T


def apply_operator(psi, ax, ay, dtype=np.float64):
    """(Hy (x) Kx^D + Ky^D (x) Hx) psi, (ny, nx)."""
    P = np.asarray(psi).astype(dtype)
    hx, hy = ax[1].astype(dtype), ay[1].astype(dtype)
    return hy[:, None] * (P @ dirichlet_stiffness(ax[2], dtype)) + (dirichlet_stiffness(ay[2], dtype) @ P) * hx[None, :]


def psi_solve_ld(om, ax, ay):
    """The same problem solved directly in long double: a banded Cholesky factorisation of the operator (symmetric positive
    definite, half bandwidth = the shorter axis) and two banded substitutions, the operator built in long double from the
    fp64 tables.  (ny, nx), long double."""
    ny, nx = om.shape
    if nx > ny:                                  # order the unknowns along the shorter axis
        return psi_solve_ld(np.ascontiguousarray(np.asarray(om).T), ay, ax).T
    hx, hy = ax[1].astype(LD), ay[1].astype(LD)
    wx, wy = LD(1) / ax[2].astype(LD), LD(1) / ay[2].astype(LD)
    n, b = nx * ny, nx
    A = np.zeros((n, b + 1), dtype=LD)           # A[k, m] = entry (k + m, k) of the lower band
    A[:, 0] = (hy[:, None] * (wx[:-1] + wx[1:])[None, :] + (wy[:-1] + wy[1:])[:, None] * hx[None, :]).ravel()
    off_x = np.zeros((ny, nx), dtype=LD)
    off_x[:, :-1] = -hy[:, None] * wx[1:nx][None, :]
    A[:, 1] += off_x.ravel()                     # (b >= 8: the x and y neighbours are different bands)
    off_y = np.zeros((ny, nx), dtype=LD)
    off_y[:-1, :] = -wy[1:ny][:, None] * hx[None, :]
    A[:, b] += off_y.ravel()
    for k in range(n):
        A[k, 0] = np.sqrt(A[k, 0])
        A[k, 1:] /= A[k, 0]
        for m in range(1, min(b, n - 1 - k) + 1):
            if A[k, m] != 0:
                A[k + m, : b + 1 - m] -= A[k, m] * A[k, m:]
    x = ((hy[:, None] * hx[None, :]) * np.asarray(om).astype(LD)).ravel()
    for k in range(n):                           # L y = B
        x[k] /= A[k, 0]
        hi = min(b, n - 1 - k)
        x[k + 1: k + 1 + hi] -= A[k, 1: 1 + hi] * x[k]
    for k in range(n - 1, -1, -1):               # L^T psi = y
        hi = min(b, n - 1 - k)
        x[k] = (x[k] - A[k, 1: 1 + hi] @ x[k + 1: k + 1 + hi]) / A[k, 0]
    return x.reshape(ny, nx)


def kappa(ax, ay, eigs=None):
    """Condition number of the generalised problem: (lamy_max + lamx_max) / (lamy_min + lamx_min)."""
    (lx, _), (ly, _) = (dirichlet_eig(ax), dirichlet_eig(ay)) if eigs is None else eigs
    return float((ly[-1] + lx[-1]) / (ly[0] + lx[0]))


def omega_bound(u, v, ulid, ax, ay):
    """6 eps max(|u|, |v|, lid) (1 / min hx + 1 / min hy): per term two face values (a product, a complement and a sum each), a
    difference and a division."""
    top = max(float(np.max(np.abs(u))), float(np.max(np.abs(v))), float(np.max(np.abs(ulid))))
    return 6 * EPS * top * (1 / float(np.min(ax[1])) + 1 / float(np.min(ay[1])))


def psi_bound(psi_ld, ax, ay, eigs=None):
    """4 eps kappa max|psi|."""
    return 4 * EPS * kappa(ax, ay, eigs) * float(np.max(np.abs(psi_ld)))


def mask_bounds(ax, ay):
    return W.mask_bounds(ax[0], ay[0])


extrema = W.extrema
reflected = W.reflected


# ---- refinement ---------------------------------------------------------------------------------------------------
def stencil_distances(d, k):
    """(dw, de) of cell k: the distances to the neighbours' centres; the mirror cell beyond a wall lies at twice the wall's d."""
    n = d.size - 1
    return (d[k] if k > 0 else 2 * d[0]), (d[k + 1] if k < n - 1 else 2 * d[n])


def fit(Cc, Wv, E, S, N, SW, SE, NW, NE, dw, de, ds, dn):
    """(gx, gy, Hxx, Hyy, Hxy) of the six-term quadratic through a 3 x 3 stencil, in the order and grouping of the kernel."""
    gx = (((E - Cc) * dw) / de + ((Cc - Wv) * de) / dw) / (dw + de)
    gy = (((N - Cc) * ds) / dn + ((Cc - S) * dn) / ds) / (ds + dn)
    Hxx = (2 * ((E - Cc) / de - (Cc - Wv) / dw)) / (dw + de)
    Hyy = (2 * ((N - Cc) / dn - (Cc - S) / ds)) / (ds + dn)
    Hxy = (((NE - NW) - SE) + SW) / ((dw + de) * (ds + dn))
    return gx, gy, Hxx, Hyy, Hxy


def group(psi, om, cell, ax, ay, want_min, none=False, refine=1, dtype=np.float64):
    """One group of the result block, x, y, psi, omega, status, sx, sy, 0, for the extremum at ``cell`` (-1: none), every
    operation in the order and grouping of the kernel.  ``dtype=LD``: the same in long double (the floors stay fp64's)."""
    ny, nx = psi.shape
    r = np.zeros(GROUP_LEN, dtype=dtype)
    r[G_STATUS] = 1.0 if refine else -1.0
    if cell < 0:
        return r
    i, j = int(cell) % nx, int(cell) // nx
    f = dtype
    xc, yc = ax[0], ay[0]
    r[G_X], r[G_Y], r[G_PSI], r[G_OMEGA] = xc[i], yc[j], psi[j, i], om[j, i]
    if not refine or none:
        return r
    with np.errstate(all="ignore"):
        dw, de = (f(t) for t in stencil_distances(ax[2], i))
        ds, dn = (f(t) for t in stencil_distances(ay[2], j))
        at = lambda a, b: f(reflected(psi, i + a, j + b))        # noqa: E731
        Cc, Wv, E, S, N = at(0, 0), at(-1, 0), at(1, 0), at(0, -1), at(0, 1)
        SW, SE, NW, NE = at(-1, -1), at(1, -1), at(-1, 1), at(1, 1)
        gx, gy, Hxx, Hyy, Hxy = fit(Cc, Wv, E, S, N, SW, SE, NW, NE, dw, de, ds, dn)
        det = Hxx * Hyy - Hxy * Hxy
        eps = f(EPS)
        Fxx = (4 * eps) * ((2 * ((abs(E) + abs(Cc)) / de + (abs(Cc) + abs(Wv)) / dw)) / (dw + de))
        Fyy = (4 * eps) * ((2 * ((abs(N) + abs(Cc)) / dn + (abs(Cc) + abs(S)) / ds)) / (ds + dn))
        Fxy = (4 * eps) * ((((abs(NE) + abs(NW)) + abs(SE)) + abs(SW)) / ((dw + de) * (ds + dn)))
        definite = (abs(Hxx) > Fxx and abs(Hyy) > Fyy
                    and det > (Fxx * abs(Hyy) + Fyy * abs(Hxx)) + 2 * Fxy * abs(Hxy)
                    and (Hxx > 0 if want_min else Hxx < 0))
        if not definite:
            r[G_STATUS] = 2.0
            return r
        sx, sy = -(Hyy * gx - Hxy * gy) / det, -(Hxx * gy - Hxy * gx) / det
        x, y = f(xc[i]) + sx, f(yc[j]) + sy
        Lx, Ly = f(xc[nx - 1]) + f(ax[2][nx]), f(yc[ny - 1]) + f(ay[2][ny])
        if (not (-dw <= sx <= de) or not (-ds <= sy <= dn) or not (0.0 <= x <= Lx) or not (0.0 <= y <= Ly)):
            r[G_STATUS] = 3.0
            return r
        ps = Cc + f(0.5) * (gx * sx + gy * sy)
        w = f(om[j, i])
        if 0 < i < nx - 1 and 0 < j < ny - 1:
            o = lambda a, b: f(om[j + b, i + a])                 # noqa: E731
            wC = o(0, 0)
            ax_, ay_, Axx, Ayy, Axy = fit(wC, o(-1, 0), o(1, 0), o(0, -1), o(0, 1), o(-1, -1), o(1, -1), o(-1, 1), o(1, 1),
                                          dw, de, ds, dn)
            w = ((((wC + ax_ * sx) + ay_ * sy) + ((f(0.5) * Axx) * sx) * sx) + ((f(0.5) * Ayy) * sy) * sy) + (Axy * sx) * sy
        if not (abs(ps) <= BIG) or not (abs(w) <= BIG):
            r[G_STATUS] = 3.0
            return r
    r[:] = (x, y, ps, w, 0.0, sx / dw if sx < 0 else sx / de, sy / ds if sy < 0 else sy / dn, 0.0)
    return r


def result_block(psi, om, bounds, ax, ay, refine=1, dtype=np.float64):
    """The whole result block: the LDC_FV_POST_* slots, then the groups of the primary minimum, BR, BL and TL."""
    r = np.zeros(RESULT_LEN, dtype=dtype)
    r[:POST_LEN] = extrema(psi, om, bounds)
    flagged = r[W.NONFINITE] != 0
    r[POST_LEN: POST_LEN + GROUP_LEN] = group(psi, om, int(r[W.PSI_MIN_CELL]), ax, ay, True, flagged, refine, dtype)
    for q in range(3):
        none = flagged or not (r[W.PSI_BR + q] > 0)
        lo = POST_LEN + (1 + q) * GROUP_LEN
        r[lo: lo + GROUP_LEN] = group(psi, om, int(r[W.PSI_BR_CELL + q]), ax, ay, False, none, refine, dtype)
    return r


block_groups = W.block_groups


def statuses(r):
    return tuple(int(g[G_STATUS]) for g in block_groups(r).values())


def metrics(r, ax, ay):
    """The vortex-metrics dict a stretched wall trial reports, from a result block (``W.metrics`` with the stretched centres
    for omega_max)."""
    nx = ax[0].size
    out = W.metrics(r, nx, 1.0, 1.0)
    cmax = int(r[W.OMEGA_MAX_CELL])
    out.update(omega_max_x=float(ax[0][cmax % nx]), omega_max_y=float(ay[0][cmax // nx]))
    return out


# ---- states -------------------------------------------------------------------------------------------------------
def smooth_field(ax, ay):
    """psi = -sin(pi x) sin(pi y) exp(-((x - 0.53)^2 + (y - 0.57)^2)) on the unit square and omega = -lap psi, at the cell
    centres: (psi, omega), (ny, nx).  psi = 0 on the four walls."""
    def part(x, a):
        e, s, c = np.exp(-(x - a) ** 2), np.sin(np.pi * x), np.cos(np.pi * x)
        return s * e, e * ((4 * (x - a) ** 2 - 2 - np.pi**2) * s - 4 * np.pi * (x - a) * c)
    S, S2 = part(ax[0], 0.53)
    T, T2 = part(ay[0], 0.57)
    return -np.outer(T, S), np.outer(T, S2) + np.outer(T2, S)


def manufactured(ax, ay):
    """``W.manufactured``'s field at the stretched centres of the unit square: psi = -16 x^2 (1-x)^2 y^2 (1-y) e^{x/2},
    u = psi_y, v = -psi_x, ulid = u(x, 1): (u, v, ulid, psi_exact), fields (ny, nx)."""
    X, Y = np.meshgrid(ax[0], ay[0])
    a = lambda x: x**2 * (1 - x) ** 2 * np.exp(x / 2)                                            # noqa: E731
    da = lambda x: np.exp(x / 2) * (2 * x * (1 - x) ** 2 - 2 * x**2 * (1 - x) + 0.5 * x**2 * (1 - x) ** 2)  # noqa: E731
    b = lambda y: y**2 * (1 - y)                                                                 # noqa: E731
    db = lambda y: 2 * y - 3 * y**2                                                              # noqa: E731
    return -16 * a(X) * db(Y), 16 * da(X) * b(Y), -16 * a(ax[0]) * db(1.0), -16 * a(X) * b(Y)


def state_for_psi(target, ax, ay):
    """(u, v, ulid) whose omega satisfies V . omega = (Hy (x) Kx^D + Ky^D (x) Hx) target, so that the solve returns ``target``
    up to rounding: v = 0 and per column the face values of u upwards from 0 on the bottom wall, f_(j+1) = f_j - hy_j omega_j;
    u_0 = 0 and u_k from f_k = g_k u_k + (1 - g_k) u_(k-1); the lid profile is the top face."""
    ny, nx = target.shape
    om = apply_operator(target, ax, ay) / (ax[1][None, :] * ay[1][:, None])
    gy = ay[3]
    u = np.zeros((ny, nx))
    face = np.zeros(nx)
    for j in range(ny - 1):
        face = face - ay[1][j] * om[j]           # the face above row j
        u[j + 1] = (face - (1.0 - gy[j + 1]) * u[j]) / gy[j + 1]
    return u, np.zeros((ny, nx)), face - ay[1][-1] * om[-1]


def quadratic_field(ax, ay, x0, y0, a=1.3, b=0.8, c=0.4, level=-1.0):
    """level + a (x - x0)^2 + b (y - y0)^2 + c (x - x0)(y - y0) at the cell centres: the six-term quadratic the fit is exact for."""
    X, Y = np.meshgrid(ax[0] - x0, ay[0] - y0)
    return level + a * X**2 + b * Y**2 + c * X * Y


def short_side_field(ax, ay, i=3, j=4):
    """A field whose lowest cell is (i, j) of a mesh with dw < de there and whose fit steps west by more than dw and less
    than de: the status-3 case only unequal spacing has.  +1 everywhere but on the 3 x 3 stencil, which samples a narrow valley
    -1 + a X^2 + b Y^2 - c X Y (X, Y from the stationary point) running from the south-west to the north-east."""
    dw, de = stencil_distances(ax[2], i)
    ds, dn = stencil_distances(ay[2], j)
    assert 1.25 * dw < de
    tx, ty = 0.5 * (dw + de) if de < 2 * dw else 1.5 * dw, 0.6 * ds
    # the valley's axis passes through the cell: X / tx = Y / ty along it, steep across it
    psi = np.ones((ay[0].size, ax[0].size))
    for bb in (-1, 0, 1):
        for aa in (-1, 0, 1):
            X = tx + (ax[0][i + aa] - ax[0][i])
            Y = ty + (ay[0][j + bb] - ay[0][j])
            along, across = (X * tx + Y * ty) / np.hypot(tx, ty), (X * ty - Y * tx) / np.hypot(tx, ty)
            psi[j + bb, i + aa] = -1 + 0.02 * along**2 / (tx * tx + ty * ty) + 40.0 * across**2 / (dw * dw + ds * ds)
    return psi


def status_fields(ax, ay):
    """Target psi fields that reach every status code through the whole chain on a mesh of at least 12 x 10 cells, with the
    statuses (primary, BR, BL, TL) the statement gives on the exact field (None: whatever the corners of this field give):
    all zero; a vortex in the ring cells of the west wall and no corner; the same with a BR vortex; a narrow valley whose fit
    leaves the stencil on its short side; a lowest cell with an indefinite fit; a positive ramp, whose lowest cell has a
    definite fit of the wrong sign."""
    ny, nx = ay[0].size, ax[0].size
    X, Y = np.meshgrid(ax[0], ay[0])
    s = ax[1][0]
    wall = -(X / s) * np.exp(-2 * X / s) * np.exp(-((Y - 0.45) ** 2) / 0.05)
    corner = wall + 0.3 * np.exp(-((X - 0.8) ** 2 + (Y - 0.2) ** 2) / 0.01)
    I, J = np.meshgrid(np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64))
    saddle = -1 + 0.1 * (I - 5) ** 2 + 0.001 * (J - 4) ** 2
    for a, b in ((1, 1), (-1, -1), (1, -1), (-1, 1)):
        saddle[4 + b, 5 + a] += 0.05 * a * b
    ramp = 1 + 0.1 * I + 0.1 * J
    return dict(zero=(np.zeros((ny, nx)), (2, 1, 1, 1)), ring=(wall, (0, 1, 1, 1)), corner=(corner, (0, 0, None, None)),
                short_side=(short_side_field(ax, ay), (3, None, None, None)),
                saddle=(saddle, (2, None, None, None)), ramp=(ramp, (2, None, None, None)))
