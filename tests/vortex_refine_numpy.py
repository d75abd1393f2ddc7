"""NumPy statement of ``ldc_vortex_refine`` (include/ldc_hip.h, csrc/ldc_vortex_refine.hip), in fp64 and in
``np.longdouble``, shared by tests/test_vortex_refine_cpu.py and tests/test_gpu_vortex_refine.py, with DERIVED rounding
bounds in the manner of tests/spectral_post_numpy.py.

The algorithm.  Per extremum (0 the primary minimum, 1 ... 3 the BR, BL, TL maxima) Newton's method on the gradient of the
tensor-product Lagrange interpolant of Psi, started at the grid node (i0, j0) and clipped to the box of its neighbouring
nodes.  At z: a = l_x(z_x), b = l_y(z_y) by the barycentric formula (the unit vector on a node); a1 = a Dx, a2 = a1 Dx,
b1 = b Dy, b2 = b1 Dy; w_k = Psi b_k; g = (a1.w0, a.w1), H = [[a2.w0, a1.w1], [a1.w1, a.w2]].  Statuses as the header lists
them.  Definiteness is judged against rounding: an entry of H counts only above F = 3 M 2^-53 (M = max(Mx, My):
three chained sums of at most M terms) times the sum of the magnitudes of its own terms, |a2| |Psi| |b| for Hxx,
|a1| |Psi| |b1| for Hxy, |a| |Psi| |b2| for Hyy, and det only above Fxx |Hyy| + Fyy |Hxx| + 2 Fxy |Hxy|.  (The Hessian of
x + y is the rounding of its own sums -- 1e-2 of that floor, its signs a matter of summation order and precision -- and
is indefinite by this rule in every order; the Hessians of the vortices of the tests stand 1e7 above it.)

The bounds.  u = 2^-53, gamma_n = n u / (1 - n u); a sum of n products in fp64 in ANY order, fused or not, errs by at most
gamma_n sum |x_i| |y_i| (Higham, Accuracy and Stability, 3.1-3.5).  ``eval_bound`` carries a running elementwise bound
through the chain exactly as ``spectral_post_numpy._stage`` does:

* a: t_i = w_i / (z - x_i) is two roundings, their sum S errs by gamma_{M+1} sum |t_i| = gamma_{M+1} Lambda |S| (Lambda =
  sum |a_i|, the Lebesgue function at z), the quotient t_i / S is one more: every a_i has the relative error
  e_a = gamma_{M+4} Lambda to first order (the second order, 1e-28, disappears in the factor 1.01);
* a1 = a Dx: E1 = (e_a + gamma_M) |a| |Dx|; a2 = a1 Dx: E2 = E1 |Dx| + gamma_M (|a1| + E1) |Dx|; b, b1, b2 alike;
* w_k = Psi b_k: Ew_k = |Psi| Eb_k + gamma_My |Psi| (|b_k| + Eb_k);
* a dot product p.q of Mx terms: Ep.(|q| + Eq) + |p|.Eq + gamma_Mx (|p| + Ep).(|q| + Eq).

Location.  Both iterations (the one under test and the long-double one) stop after a Newton step of at most 1e-13 L per
axis.  The error left after a Newton step is the step times the contraction factor of that step, which for a step of
1e-13 L is far below 1/2: the two stop rules together leave at most 1e-13 L.  The iteration under test converges to the zero
of the gradient AS IT EVALUATES IT, which lies |H^-1| dg from the exact one, dg the evaluation bound of the gradient:
    loc = 1e-13 L + |H^-1| dg.
psi*: the evaluation bound of a.Psi.b alone -- the gradient vanishes there, the move by loc changes psi by at most
1.5 |H| loc^2 (added: 1e-26).  omega*: the evaluation bound of a.W.b plus |grad omega| . loc.
The bounds are evaluated at the long-double solution with fp64 magnitudes (their own rounding disappears in 1.01)."""
import numpy as np

from spectral_post_numpy import LDBL, SLACK, U, gamma

MAX_STEPS, MAX_M, OUT_LEN = 20, 257, 32
REFINED, NO_CANDIDATE, INDEFINITE, CLIPPED, NOT_CONVERGED, WORSE, NOT_FINITE = range(7)
NAMES = ("primary", "BR", "BL", "TL")
IDX_SLOT = (0, 2, 3, 4)                 # entry of ldc_vortex_extrema_xy's index array an extremum starts from


def basis(x, w, z):
    """Lagrange basis values at z by the barycentric formula; the unit vector when z is a node."""
    d = z - x
    hit = np.flatnonzero(d == 0)
    if hit.size:
        a = np.zeros_like(x)
        a[hit[0]] = 1
        return a
    t = w / d
    return t / np.sum(t)


def evaluate(Psi, x, y, wx, wy, Dx, Dy, zx, zy):
    """(a, a1, a2, b, b1, b2) at z, the types of the inputs throughout."""
    a, b = basis(x, wx, zx), basis(y, wy, zy)
    a1, b1 = a @ Dx, b @ Dy
    return a, a1, a1 @ Dx, b, b1, b1 @ Dy


def refine_one(Psi, W, x, y, wx, wy, Dx, Dy, e, q, LD, dtype=np.float64):
    """The 8 output values of extremum e started at flat index q = i0 * LD + j0, and the final (zx, zy) in ``dtype``."""
    Mx, My = Psi.shape
    c = lambda v: np.asarray(v, dtype=dtype)          # noqa: E731
    out = np.zeros(8, dtype=dtype)
    i0, j0 = (-1, -1) if q < 0 else divmod(int(q), LD)
    on_grid = 0 <= i0 < Mx and 0 <= j0 < My
    if not on_grid or (e > 0 and not Psi[i0, j0] > 0):
        out[0] = NO_CANDIDATE
        return out, None
    Psi_, W_, x_, y_, wx_, wy_, Dx_, Dy_ = (c(v) for v in (Psi, W, x, y, wx, wy, Dx, Dy))
    pn, wn, xn, yn = Psi_[i0, j0], W_[i0, j0], x_[i0], y_[j0]
    xb = (x_[max(i0 - 1, 0)], x_[min(i0 + 1, Mx - 1)])
    yb = (y_[max(j0 - 1, 0)], y_[min(j0 + 1, My - 1)])
    xlo, xhi, ylo, yhi = min(xb), max(xb), min(yb), max(yb)
    tolx, toly = dtype(1e-13) * abs(x_[-1] - x_[0]), dtype(1e-13) * abs(y_[-1] - y_[0])
    floor_rel = dtype(3 * max(Mx, My)) * dtype(U)
    aP = np.abs(Psi_)
    zx, zy, status, steps = xn, yn, NOT_CONVERGED, 0
    with np.errstate(all="ignore"):
        for it in range(MAX_STEPS):
            a, a1, a2, b, b1, b2 = evaluate(Psi_, x_, y_, wx_, wy_, Dx_, Dy_, zx, zy)
            w0, w1, w2 = Psi_ @ b, Psi_ @ b1, Psi_ @ b2
            gx, gy, hxx, hxy, hyy = a1 @ w0, a @ w1, a2 @ w0, a1 @ w1, a @ w2
            if not np.all(np.isfinite(np.asarray([gx, gy, hxx, hxy, hyy], dtype=dtype))):
                status = NOT_FINITE
                break
            fxx, fxy, fyy = (floor_rel * (np.abs(p) @ (aP @ np.abs(q))) for p, q in ((a2, b), (a1, b1), (a, b2)))
            det, fdet = hxx * hyy - hxy * hxy, fxx * abs(hyy) + fyy * abs(hxx) + 2 * fxy * abs(hxy)
            sxx, syy = (hxx, hyy) if e == 0 else (-hxx, -hyy)
            if not (sxx > fxx and syy > fyy and det > fdet):
                status = INDEFINITE
                break
            tx, ty = zx - (hyy * gx - hxy * gy) / det, zy - (hxx * gy - hxy * gx) / det
            nx, ny = min(max(tx, xlo), xhi), min(max(ty, ylo), yhi)
            clipped = nx != tx or ny != ty
            sx, sy = nx - zx, ny - zy
            zx, zy, steps = nx, ny, it + 1
            if abs(sx) <= tolx and abs(sy) <= toly:
                status = CLIPPED if clipped else REFINED
                break
        a, a1, _, b, b1, _ = evaluate(Psi_, x_, y_, wx_, wy_, Dx_, Dy_, zx, zy)
        w0, w1 = Psi_ @ b, Psi_ @ b1
        psi, om, gx, gy = a @ w0, a @ (W_ @ b), a1 @ w0, a @ w1
        gnorm = np.sqrt(gx * gx + gy * gy)
    if status == REFINED:
        if not np.all(np.isfinite(np.asarray([zx, zy, psi, om, gnorm], dtype=dtype))):
            status = NOT_FINITE
        elif (not psi <= pn) if e == 0 else (not psi >= pn):
            status = WORSE
        elif (e == 1 and not (zx > 0.5 and zy < 0.5)) or (e == 2 and not (zx < 0.5 and zy < 0.5)) or \
                (e == 3 and not (zx < 0.5 and zy > 0.5)):
            status = WORSE
    ok = status == REFINED
    out[:] = [status, zx if ok else xn, zy if ok else yn, psi if ok else pn, om if ok else wn, steps, gnorm, 0]
    return out, (zx, zy)


def refine(Psi, W, x, y, wx, wy, Dx, Dy, idx, LD=None, dtype=np.float64):
    """The OUT_LEN values of one job: ``idx`` the five indices of ``spectral_post_numpy.extrema`` (pitch LD, default My)."""
    LD = Psi.shape[1] if LD is None else LD
    return np.concatenate([refine_one(Psi, W, x, y, wx, wy, Dx, Dy, e, int(idx[IDX_SLOT[e]]), LD, dtype)[0]
                           for e in range(4)])


def eval_bound(Psi, W, x, y, wx, wy, Dx, Dy, zx, zy, psi_err=None):
    """Bounds on an fp64 evaluation at z of (gx, gy, psi, omega) and the magnitudes that turn them into a location bound:
    dict with dg (2), dpsi, domega, H (2 x 2), grad_omega (2); everything in fp64 at the fp64 rounding of z.  ``psi_err``:
    an elementwise bound on what the entries of Psi themselves are off (data that was rounded on its way in)."""
    f = lambda v: np.asarray(v, dtype=np.float64)          # noqa: E731
    Psi, W, x, y, wx, wy, Dx, Dy = (f(v) for v in (Psi, W, x, y, wx, wy, Dx, Dy))
    Mx, My = Psi.shape
    a, a1, a2, b, b1, b2 = evaluate(Psi, x, y, wx, wy, Dx, Dy, np.float64(zx), np.float64(zy))

    def chain(v, D, M):
        """(|v|, E), (|v D|, E1), (|v D D|, E2) of one axis."""
        on_node = np.count_nonzero(v) == 1 and np.max(v) == 1.0
        ea = 0.0 if on_node else gamma(M + 4) * np.sum(np.abs(v))
        aD, gM = np.abs(D), gamma(M)
        v1 = v @ D
        E0 = ea * np.abs(v)
        E1 = (ea + gM) * (np.abs(v) @ aD)
        E2 = E1 @ aD + gM * ((np.abs(v1) + E1) @ aD)
        return (np.abs(v), E0), (np.abs(v1), E1), (np.abs(v1 @ D), E2)
    A, B = chain(a, Dx, Mx), chain(b, Dy, My)
    aP = np.abs(Psi)
    eP = np.zeros_like(aP) if psi_err is None else f(psi_err)

    def rows(F, eF, k):
        """(|F b_k| reach, bound) of the row pass."""
        mag, E = B[k]
        aF = np.abs(F) + eF
        return np.abs(F @ (b, b1, b2)[k]), aF @ E + gamma(My) * (aF @ (mag + E)) + eF @ mag

    def dot(k, wk):
        (pm, pE), (qm, qE) = A[k], wk
        return pE @ (qm + qE) + pm @ qE + gamma(Mx) * ((pm + pE) @ (qm + qE))
    w = [rows(Psi, eP, k) for k in range(3)]
    wW = [rows(W, np.zeros_like(aP), k) for k in range(2)]
    H = np.array([[a2 @ (Psi @ b), a1 @ (Psi @ b1)], [a1 @ (Psi @ b1), a @ (Psi @ b2)]])
    return dict(dg=SLACK * np.array([dot(1, w[0]), dot(0, w[1])]), dpsi=SLACK * dot(0, w[0]), domega=SLACK * dot(0, wW[0]),
                H=H, grad_omega=np.array([a1 @ (W @ b), a @ (W @ b1)]))


def bounds(Psi, W, x, y, wx, wy, Dx, Dy, zx, zy, psi_err=None):
    """(loc[2], dpsi, domega): how far an fp64 run of the algorithm may end from the long-double one at (zx, zy)."""
    x, y = np.asarray(x, float), np.asarray(y, float)
    b = eval_bound(Psi, W, x, y, wx, wy, Dx, Dy, zx, zy, psi_err)
    Hinv = np.abs(np.linalg.inv(b["H"]))
    loc = 1e-13 * np.array([abs(x[-1] - x[0]), abs(y[-1] - y[0])]) + SLACK * (Hinv @ b["dg"])
    dpsi = b["dpsi"] + 1.5 * float(loc @ np.abs(b["H"]) @ loc)
    domega = b["domega"] + SLACK * float(np.abs(b["grad_omega"]) @ loc)
    return loc, dpsi, domega


def compare(got, want_ld, Psi, W, x, y, wx, wy, Dx, Dy, psi_err=None):
    """Largest error / bound of the refined extrema of one job: ``got`` OUT_LEN fp64 values, ``want_ld`` the long-double
    ones; only extrema that both report REFINED are measured (the caller compares the statuses)."""
    worst = 0.0
    for e in range(4):
        g, w = got[8 * e: 8 * e + 8], want_ld[8 * e: 8 * e + 8]
        if int(g[0]) != REFINED or int(w[0]) != REFINED:
            continue
        loc, dpsi, domega = bounds(Psi, W, x, y, wx, wy, Dx, Dy, w[1], w[2], psi_err)
        err = np.abs(np.asarray(g[1:5], dtype=LDBL) - w[1:5]).astype(float)
        worst = max(worst, float(np.max(err / np.array([loc[0], loc[1], dpsi, domega]))))
    return worst


# ------------------------------------------------------------------------------------------------ grids and fields
def grid(kind, M):
    """(x, barycentric weights, D) of the solver's own axis on [0, 1]."""
    from solvers.spectral.basis.spectral import ChebyshevLobattoBasis, LegendreLobattoBasis
    from solvers.spectral.sg import _axis_operators, barycentric_weights
    basis_ = {"chebyshev": ChebyshevLobattoBasis, "legendre": LegendreLobattoBasis}[kind](domain=(0.0, 1.0))
    x, D = _axis_operators(basis_, kind, M)[:2]
    return x, barycentric_weights(kind, x), D


QUADRATICS = [(0.5308, 0.5652, 1.0), (0.8640, 0.1118, -1.0), (0.0833, 0.0781, -1.0), (0.37, 0.93, 1.0)]
QUADRATIC_SIZES = [(4, 4), (8, 12), (32, 32), (50, 50), (128, 47), (256, 256)]            # (nx, ny): N, one node more
CAVITY_SIZES = [(24, 24), (32, 40), (50, 50), (96, 64), (129, 48), (256, 256)]
GPU_SHAPES = [(5, 5), (9, 13), (33, 33), (51, 51), (65, 65), (129, 48), (48, 129), (257, 257)]      # (Mx, My) nodes


def quadratic(x, y, x0, y0, s, dtype=np.float64):
    """(psi, elementwise bound on its fp64 rounding, d psi / dx, d psi / dy) of
    s ((x-x0)^2 + 2 (y-y0)^2 + 0.3 (x-x0)(y-y0)) - 0.1 s on the grid."""
    X, Y = np.asarray(x, dtype)[:, None] - dtype(x0), np.asarray(y, dtype)[None, :] - dtype(y0)
    three_tenths, tenth = dtype(3) / dtype(10), dtype(1) / dtype(10)
    psi = dtype(s) * (X * X + 2 * Y * Y + three_tenths * X * Y) - tenth * dtype(s)
    mag = np.abs(X * X) + 2 * np.abs(Y * Y) + 0.3 * np.abs(X * Y) + 0.1
    return psi, gamma(12) * mag.astype(float), dtype(s) * (2 * X + three_tenths * Y + 0 * Y), dtype(s) * (4 * Y + three_tenths * X)


def quadratic_start(x, y, x0, y0, LD):
    """Flat index of the node nearest to (x0, y0) in the norm of the quadratic: its grid extremum up to ties."""
    X, Y = x[:, None] - x0, y[None, :] - y0
    q = int(np.argmin(X * X + 2 * Y * Y + 0.3 * X * Y))
    return (q // y.size) * LD + q % y.size


def cavity(x, y, dtype=np.float64):
    """The synthetic cavity: a primary minimum and three corner eddies of Gaussians; W = cos 3x sin 2y."""
    X, Y = np.asarray(x, dtype)[:, None], np.asarray(y, dtype)[None, :]
    d = lambda v: dtype(v) / dtype(1000)          # noqa: E731  (decimal constants exactly in either type)
    g = lambda cx, cy, s: np.exp(-((X - d(cx)) ** 2 + (Y - d(cy)) ** 2) / d(s))          # noqa: E731
    psi = -g(530, 570, 80) + d(20) * g(860, 110, 10) + d(10) * g(80, 80, 5) + d(50) * g(70, 900, 4)
    return psi, np.cos(3 * X) * np.sin(2 * Y)


def device_call(jobs_np, LD=None):
    """Run ``ldc_vortex_refine`` once on a list of jobs (Psi, W, x, y, wx, wy, Dx, Dy, idx) of host arrays: uploads each
    job padded to its own pitch, returns the list of OUT_LEN result vectors.  GPU tests only."""
    import ctypes as C
    import torch
    from solvers.spectral import ldc_lib as L
    L.require_device()
    keep, arr = [], (L.RefineJob * len(jobs_np))()
    for k, (Psi, W, x, y, wx, wy, Dx, Dy, idx) in enumerate(jobs_np):
        Mx, My = Psi.shape
        ld = (My + 3 if LD is None else LD)
        ldd = max(Mx, My) + 1

        def up(a, shape=None, dt=np.float64):
            full = np.full(shape if shape else a.shape, np.nan if dt == np.float64 else 0, dtype=dt)
            full[tuple(slice(0, n) for n in a.shape)] = a
            t = torch.from_numpy(full).cuda()
            keep.append(t)
            return t
        flat = np.asarray(idx, dtype=np.int64)
        flat = np.where(flat < 0, -1, (flat // My) * ld + flat % My).astype(np.int32)          # idx comes with pitch My
        t = [up(Psi, (Mx, ld)), up(W, (Mx, ld)), up(x), up(y), up(wx), up(wy), up(Dx, (Mx, ldd)), up(Dy, (My, ldd)),
             up(flat, None, np.int32), up(np.full(OUT_LEN, -7.0))]
        for name, tt in zip(("Psi", "W", "x", "y", "wx", "wy", "Dx", "Dy", "idx", "out"), t):
            setattr(arr[k], name, tt.data_ptr())
        arr[k].Mx, arr[k].My, arr[k].LD, arr[k].LDD = Mx, My, ld, ldd
    L.check(L.lib().ldc_vortex_refine(arr, len(jobs_np), L.stream_ptr()), "ldc_vortex_refine")
    torch.cuda.synchronize()
    return [keep[10 * k + 9].cpu().numpy() for k in range(len(jobs_np))]
