"""NumPy statement of the wall-anchored finite-volume post-processing (include/ldc_fv.h, ldc_fv_wall_post_enqueue),
shared by tests/test_fv_wall_post_cpu.py and tests/test_gpu_fv_wall_post.py: the half-sample sine tables, omega with the
lid profile in its ghost row, psi with psi = 0 on the wall faces by fast diagonalisation (fp64 and long double), the
extrema rule, the 3 x 3 quadratic refinement with its floors and statuses, the result block and the metrics read off it;
and the manufactured field, seeded states and error bounds of the tests."""
import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
BIG = float(np.finfo(np.float64).max)

RESULT_LEN, POST_LEN, GROUP_LEN = 48, 16, 8
(PSI_MIN, OMEGA_CENTER, OMEGA_MAX, PSI_BR, PSI_BL, PSI_TL, PSI_MIN_CELL, OMEGA_MAX_CELL, PSI_BR_CELL, PSI_BL_CELL,
 PSI_TL_CELL, NONFINITE) = range(12)
G_X, G_Y, G_PSI, G_OMEGA, G_STATUS, G_SX, G_SY = range(7)
GROUPS = ("min", "BR", "BL", "TL")

# (nx, ny, Lx, Ly) of the GPU tests: the minimum; odd with GEMM edge fill; a stretched domain; 33 x 20; above the one-CU
# limit with several work-groups per sweep; the maximum either way
GPU_SHAPES = [(8, 8, 1.0, 1.0), (13, 17, 1.0, 1.0), (24, 16, 2.0, 0.5), (33, 20, 1.0, 1.0), (260, 9, 1.0, 1.0),
              (1024, 8, 1.0, 1.0), (8, 1024, 1.0, 1.0)]
EXACT_CENTRE = (0.531129, 0.666667)          # of the manufactured field below


def shape_id(s):
    return f"{s[0]}x{s[1]}"


# ---- tables -------------------------------------------------------------------------------------------------------
def wall_matrix(n, dtype=np.float64):
    """T_n = tridiag(-1, 2, -1) with 3 in both corners: the ghost cell is -psi, so psi = 0 on the wall face."""
    T = 2 * np.eye(n, dtype=dtype) - np.eye(n, k=1, dtype=dtype) - np.eye(n, k=-1, dtype=dtype)
    T[0, 0] = T[-1, -1] = 3
    return T


def tables(n, dtype=np.float64):
    """(lam, C): lam[k] = 2 - 2 cos(pi (k+1)/n), C[j, k] = sqrt(2/n) sin(pi (k+1)(j+1/2)/n), the last column divided by
    sqrt(2).  T_n = C diag(lam) C^T, C^T C = I; C is not symmetric."""
    pi = np.arccos(dtype(-1))
    k = np.arange(1, n + 1).astype(dtype)
    j = np.arange(n).astype(dtype) + dtype(0.5)
    Cm = np.sqrt(dtype(2) / dtype(n)) * np.sin(pi * np.outer(j, k) / dtype(n))
    Cm[:, -1] /= np.sqrt(dtype(2))
    return dtype(2) - dtype(2) * np.cos(pi * k / dtype(n)), Cm


# ---- fields -------------------------------------------------------------------------------------------------------
def omega(u, v, ulid, dx, dy):
    """omega (ny, nx) by ghost cells: -f at the walls, 2 ulid[i] - u above the top row; (vE - vW)/(2 dx) - (uN - uS)/(2 dy)."""
    U, V = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    ny, nx = U.shape
    vE = np.concatenate([V[:, 1:], -V[:, -1:]], axis=1)
    vW = np.concatenate([-V[:, :1], V[:, :-1]], axis=1)
    uN = np.concatenate([U[1:], (2 * np.asarray(ulid, dtype=np.float64) - U[-1])[None, :]], axis=0)
    uS = np.concatenate([-U[:1], U[:-1]], axis=0)
    return (vE - vW) / (2 * dx) - (uN - uS) / (2 * dy)


def psi_solve(om, dx, dy, dtype=np.float64, basis=None):
    """psi (ny, nx) from (cx Tx + cy Ty) psi = omega on all cells: Cy ((Cy^T Omega Cx) / (cy lamy[a] + cx lamx[b])) Cx^T.
    ``basis``: a function n -> (lam, C) in place of ``tables`` (the tables the solver uploads, in fp64)."""
    ny, nx = om.shape
    lx, Cx = tables(nx, dtype) if basis is None else basis(nx)
    ly, Cy = tables(ny, dtype) if basis is None else basis(ny)
    cx, cy = dtype(1) / (dtype(dx) * dtype(dx)), dtype(1) / (dtype(dy) * dtype(dy))
    h = (Cy.T @ om.astype(dtype) @ Cx) / (cy * ly[:, None] + cx * lx[None, :])
    return Cy @ h @ Cx.T


def psi_ring_rule(om, dx, dy):
    """The reference's rule on the same omega: psi = 0 at the centres of the boundary ring, Dirichlet on the interior."""
    import fv_post_numpy as P
    return P.psi_solve(om, dx, dy)


def kappa(nx, ny, dx, dy):
    """Condition number of cx Tx + cy Ty on all cells."""
    lx, _ = tables(nx)
    ly, _ = tables(ny)
    cx, cy = 1.0 / (dx * dx), 1.0 / (dy * dy)
    return float((cy * ly[-1] + cx * lx[-1]) / (cy * ly[0] + cx * lx[0]))


def omega_bound(u, v, ulid, dx, dy):
    """4 eps max(|u|, |v|, lid) (1/dx + 1/dy): two differences and a division per term."""
    top = max(float(np.max(np.abs(u))), float(np.max(np.abs(v))), float(np.max(np.abs(ulid))))
    return 4 * EPS * top * (1 / dx + 1 / dy)


def psi_bound(psi_ld, nx, ny, dx, dy):
    """4 eps kappa max|psi|."""
    return 4 * EPS * kappa(nx, ny, dx, dy) * float(np.max(np.abs(psi_ld)))


def cell_centres(nx, ny, Lx=1.0, Ly=1.0):
    return (np.arange(nx) + 0.5) * (Lx / nx), (np.arange(ny) + 0.5) * (Ly / ny)


def mask_bounds(xs, ys):
    return (int(np.count_nonzero(xs < 0.5)), int(xs.size - np.count_nonzero(xs > 0.5)),
            int(np.count_nonzero(ys < 0.5)), int(ys.size - np.count_nonzero(ys > 0.5)))


# ---- extrema ------------------------------------------------------------------------------------------------------
def _first_best(values):
    """(value, index) of the largest entry, ties to the lowest index, by strict comparisons from -inf: NaN and -inf never
    win; (-inf, -1) when nothing does."""
    vals = np.where(np.isnan(values), -np.inf, values)
    if vals.size == 0 or not np.any(vals > -np.inf):
        return -np.inf, -1
    at = int(np.argmax(vals))
    return float(vals[at]), at


def extrema(psi, om, bounds):
    """Slots 0 .. 15 of the result block (the LDC_FV_POST_* slots) by the device's rule."""
    ny, nx = psi.shape
    n = nx * ny
    ix_lt, ix_gt, jy_lt, jy_gt = bounds
    p, w = psi.ravel(), om.ravel()
    cells = np.arange(n)
    i, j = cells % nx, cells // nx
    _, cmin = _first_best(-p)
    _, cmax = _first_best(np.abs(w))
    ok = cmin >= 0 and cmax >= 0
    r = np.zeros(POST_LEN)
    r[PSI_MIN], r[OMEGA_CENTER], r[OMEGA_MAX] = (p[cmin], w[cmin], w[cmax]) if ok else (0.0, 0.0, 0.0)
    r[PSI_MIN_CELL], r[OMEGA_MAX_CELL] = (cmin, cmax) if ok else (-1, -1)
    regions = ((i >= ix_gt) & (j < jy_lt), (i < ix_lt) & (j < jy_lt), (i < ix_lt) & (j >= jy_gt))
    for q, mask in enumerate(regions):
        val, at = _first_best(p[mask])
        r[PSI_BR + q] = val
        r[PSI_BR_CELL + q] = cells[mask][at] if at >= 0 else -1
    bad = not (np.all(np.abs(w) <= BIG) and np.all(np.abs(p) <= BIG))
    r[NONFINITE] = 1.0 if (bad or not ok) else 0.0
    return r


# ---- refinement ---------------------------------------------------------------------------------------------------
def reflected(psi, i, j):
    """psi at (i, j) of the grid extended by odd reflection at the wall faces (+psi across a corner)."""
    ny, nx = psi.shape
    sign = 1.0
    if i < 0:
        i, sign = -1 - i, -sign
    if i >= nx:
        i, sign = 2 * nx - 1 - i, -sign
    if j < 0:
        j, sign = -1 - j, -sign
    if j >= ny:
        j, sign = 2 * ny - 1 - j, -sign
    return sign * psi[j, i]


def group(psi, om, cell, dx, dy, want_min, none=False, refine=1, dtype=np.float64):
    """One group of the result block, x, y, psi, omega, status, sx, sy, 0, for the extremum at ``cell`` (-1: none), every
    operation in the order and grouping of the kernel.  ``dtype=LD``: the same in long double (the floors stay fp64's)."""
    ny, nx = psi.shape
    r = np.zeros(GROUP_LEN, dtype=dtype)
    r[G_STATUS] = 1.0 if refine else -1.0
    if cell < 0:
        return r
    i, j = int(cell) % nx, int(cell) // nx
    f = dtype
    dx, dy = f(dx), f(dy)
    r[G_X], r[G_Y], r[G_PSI], r[G_OMEGA] = (f(i) + f(0.5)) * dx, (f(j) + f(0.5)) * dy, psi[j, i], om[j, i]
    if not refine or none:
        return r
    with np.errstate(all="ignore"):
        at = lambda a, b: f(reflected(psi, i + a, j + b))        # noqa: E731
        Cc, W, E, S, N = at(0, 0), at(-1, 0), at(1, 0), at(0, -1), at(0, 1)
        SW, SE, NW, NE = at(-1, -1), at(1, -1), at(-1, 1), at(1, 1)
        gx, gy = (E - W) * f(0.5), (N - S) * f(0.5)
        Hxx, Hyy, Hxy = (E - 2 * Cc) + W, (N - 2 * Cc) + S, (((NE - NW) - SE) + SW) * f(0.25)
        det = Hxx * Hyy - Hxy * Hxy
        eps = f(EPS)
        Fxx = 4 * eps * ((abs(E) + 2 * abs(Cc)) + abs(W))
        Fyy = 4 * eps * ((abs(N) + 2 * abs(Cc)) + abs(S))
        Fxy = eps * (((abs(NE) + abs(NW)) + abs(SE)) + abs(SW))
        definite = (abs(Hxx) > Fxx and abs(Hyy) > Fyy
                    and det > (Fxx * abs(Hyy) + Fyy * abs(Hxx)) + 2 * Fxy * abs(Hxy)
                    and (Hxx > 0 if want_min else Hxx < 0))
        if not definite:
            r[G_STATUS] = 2.0
            return r
        sx, sy = -(Hyy * gx - Hxy * gy) / det, -(Hxx * gy - Hxy * gx) / det
        x, y = ((f(i) + f(0.5)) + sx) * dx, ((f(j) + f(0.5)) + sy) * dy
        if not (abs(sx) <= 1.0) or not (abs(sy) <= 1.0) or not (0.0 <= x <= nx * dx) or not (0.0 <= y <= ny * dy):
            r[G_STATUS] = 3.0
            return r
        ps = Cc + f(0.5) * (gx * sx + gy * sy)
        w = f(om[j, i])
        if 0 < i < nx - 1 and 0 < j < ny - 1:
            o = lambda a, b: f(om[j + b, i + a])                 # noqa: E731
            wC, wW, wE, wS, wN = o(0, 0), o(-1, 0), o(1, 0), o(0, -1), o(0, 1)
            wSW, wSE, wNW, wNE = o(-1, -1), o(1, -1), o(-1, 1), o(1, 1)
            ax, ay = (wE - wW) * f(0.5), (wN - wS) * f(0.5)
            Axx, Ayy, Axy = (wE - 2 * wC) + wW, (wN - 2 * wC) + wS, (((wNE - wNW) - wSE) + wSW) * f(0.25)
            w = ((((wC + ax * sx) + ay * sy) + ((f(0.5) * Axx) * sx) * sx) + ((f(0.5) * Ayy) * sy) * sy) + (Axy * sx) * sy
        if not (abs(ps) <= BIG) or not (abs(w) <= BIG):
            r[G_STATUS] = 3.0
            return r
    r[:] = (x, y, ps, w, 0.0, sx, sy, 0.0)
    return r


def result_block(psi, om, bounds, dx, dy, refine=1, dtype=np.float64):
    """The whole result block: the LDC_FV_POST_* slots, then the groups of the primary minimum, BR, BL and TL."""
    r = np.zeros(RESULT_LEN, dtype=dtype)
    r[:POST_LEN] = extrema(psi, om, bounds)
    flagged = r[NONFINITE] != 0
    r[POST_LEN: POST_LEN + GROUP_LEN] = group(psi, om, int(r[PSI_MIN_CELL]), dx, dy, True, flagged, refine, dtype)
    for q in range(3):
        none = flagged or not (r[PSI_BR + q] > 0)
        lo = POST_LEN + (1 + q) * GROUP_LEN
        r[lo: lo + GROUP_LEN] = group(psi, om, int(r[PSI_BR_CELL + q]), dx, dy, False, none, refine, dtype)
    return r


def block_groups(r):
    """{name: the 8 doubles of its group}."""
    return {name: np.asarray(r[POST_LEN + q * GROUP_LEN: POST_LEN + (q + 1) * GROUP_LEN]) for q, name in enumerate(GROUPS)}


def metrics(r, nx, dx, dy):
    """The vortex-metrics dict a wall trial reports, from a result block: the primary minimum and the corners from the
    groups (a corner counts when its value is > 0), omega_max on the grid."""
    g = block_groups(r)
    cmax = int(r[OMEGA_MAX_CELL])
    out = dict(psi_min=float(g["min"][G_PSI]), psi_min_x=float(g["min"][G_X]), psi_min_y=float(g["min"][G_Y]),
               omega_center=float(g["min"][G_OMEGA]), omega_max=float(r[OMEGA_MAX]),
               omega_max_x=float((cmax % nx + 0.5) * dx), omega_max_y=float((cmax // nx + 0.5) * dy))
    for name in GROUPS[1:]:
        b = g[name]
        keep = r[PSI_BR + GROUPS.index(name) - 1] > 0
        vals = (b[G_PSI], b[G_OMEGA], b[G_X], b[G_Y]) if keep else (0.0, 0.0, 0.0, 0.0)
        out.update({f"psi_{name}": float(vals[0]), f"omega_{name}": float(vals[1]), f"psi_{name}_x": float(vals[2]),
                    f"psi_{name}_y": float(vals[3])})
    return out


# ---- states -------------------------------------------------------------------------------------------------------
def manufactured(nx, ny, Lx=1.0, Ly=1.0):
    """psi = -16 x^2 (1-x)^2 y^2 (1-y) e^{x/2} on the unit square (in x / Lx, y / Ly), u = psi_y, v = -psi_x at the cell
    centres, ulid = u(x, 1): (u, v, ulid, psi_exact), fields (ny, nx).  No-slip on three walls, u = ulid on the lid."""
    xs, ys = cell_centres(nx, ny)
    X, Y = np.meshgrid(xs, ys)
    a = lambda x: x**2 * (1 - x) ** 2 * np.exp(x / 2)                                            # noqa: E731
    da = lambda x: np.exp(x / 2) * (2 * x * (1 - x) ** 2 - 2 * x**2 * (1 - x) + 0.5 * x**2 * (1 - x) ** 2)  # noqa: E731
    b = lambda y: y**2 * (1 - y)                                                                 # noqa: E731
    db = lambda y: 2 * y - 3 * y**2                                                              # noqa: E731
    psi = -16 * a(X) * b(Y)
    return -16 * a(X) * db(Y) / Ly, 16 * da(X) * b(Y) / Lx, -16 * a(xs) * db(1.0) / Ly, psi


def smooth_state(nx, ny, seed=None):
    """A seeded smooth state: a few random Fourier modes per field, and a smooth lid profile: (u, v, ulid), (ny, nx)."""
    rng = np.random.default_rng(1000 * nx + ny if seed is None else seed)
    xs, ys = cell_centres(nx, ny)
    X, Y = np.meshgrid(xs, ys)
    out = []
    for _ in range(2):
        f = np.zeros((ny, nx))
        for _ in range(6):
            kx, ky = rng.integers(1, 4, size=2)
            f += rng.normal() * np.sin(np.pi * kx * X + rng.uniform(0, 3)) * np.cos(np.pi * ky * Y + rng.uniform(0, 3))
        out.append(f)
    return out[0], out[1], 1.0 + 0.3 * np.sin(2 * np.pi * xs + rng.uniform(0, 3))


def state_for_psi(target, dx, dy):
    """(u, v, ulid) whose omega is (cx Tx + cy Ty) target, so that the solve returns ``target`` up to rounding: v = 0 and
    per column u from -(uN - uS) / (2 dy) = omega upwards from u = 0 in the bottom row; the lid profile closes the top row."""
    ny, nx = target.shape
    om = (wall_matrix(ny) @ target) / (dy * dy) + (target @ wall_matrix(nx)) / (dx * dx)
    rhs = -2 * dy * om                                   # row j: uN - uS
    u = np.zeros((ny, nx))
    u[1] = rhs[0]                                        # (uS of row 0 is the ghost -u[0] = 0)
    for j in range(1, ny - 1):
        u[j + 1] = u[j - 1] + rhs[j]
    return u, np.zeros((ny, nx)), (rhs[-1] + u[-1] + u[-2]) / 2


def status_fields(nx=12, ny=10):
    """Target psi fields that reach every status code through the whole chain, with the statuses (primary, BR, BL, TL) the
    statement gives on the exact field: all zero; a vortex on the ring and no corner; the same with a BR vortex; a curved
    valley whose grid minimum lies more than a cell from the fitted one; a lowest cell with an indefinite fit; a positive
    ramp, whose lowest cell has a definite fit of the wrong sign."""
    xs, ys = cell_centres(nx, ny)
    X, Y = np.meshgrid(xs, ys)
    dx = 1.0 / nx
    wall = -(X / dx) * np.exp(-2 * X / dx) * np.exp(-((Y - 0.45) ** 2) / 0.05)
    corner = wall + 0.3 * np.exp(-((X - 0.8) ** 2 + (Y - 0.2) ** 2) / 0.01)
    I, J = np.meshgrid(np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64))
    di, dj = I - 6.584, J - 4.938        # a shallow curved valley: the lowest cell is (7, 6), its fit steps 1.3 cells down
    valley = -1 + 0.6133 * di**2 + 0.07835 * dj**2 - 0.2221 * di * dj + 0.00372 * di**3
    # a broad bowl around cell (5, 4) with its four diagonal neighbours moved by 0.05: Hxx = 0.2, Hyy = 0.002, Hxy = 0.05,
    # so the lowest cell's fit is indefinite (det < 0)
    saddle = -1 + 0.1 * (I - 5) ** 2 + 0.001 * (J - 4) ** 2
    for a, b in ((1, 1), (-1, -1), (1, -1), (-1, 1)):
        saddle[4 + b, 5 + a] += 0.05 * a * b
    # a positive ramp: the lowest cell is the corner cell 0, where the odd reflection gives Hxx = Hyy = -1.9 and
    # det > 0: a definite fit of the wrong sign for a minimum
    ramp = 1 + 0.1 * I + 0.1 * J
    return dict(zero=(np.zeros((ny, nx)), (2, 1, 1, 1)), ring=(wall, (0, 1, 1, 1)), corner=(corner, (0, 0, 1, 1)),
                valley=(valley, (3, None, None, None)),      # (None: whatever the corners of this field give)
                saddle=(saddle, (2, None, None, None)), ramp=(ramp, (2, None, None, None)))
