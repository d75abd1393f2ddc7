"""Extended-precision statements of the spectral post-processing entry points (include/ldc_hip.h: ``ldc_gemm_nt``,
``ldc_poisson_fastdiag``, ``ldc_vortex_extrema_xy``), shared by tests/test_spectral_post_cpu.py and
tests/test_gpu_spectral_post.py: the NT product and the four-product streamfunction solve in ``np.longdouble`` (80-bit,
as tests/fv_post_numpy.py assumes) with DERIVED error bounds, the extrema rule, and the seeded inputs of the tests.

The bounds.  u = 2^-53, gamma_n = n u / (1 - n u).  A sum of n products accumulated in fp64 in ANY order, with or without
fused multiply-adds, errs by at most gamma_n (|A| |B|^T) (Higham, Accuracy and Stability, 3.1-3.5); the kernel's n is
16 K16 -- every k of the padded blocks is accumulated.  The division by lam_r[i] + lam_c[j] is one more rounding: the sum of
the two eigenvalues is formed here in fp64 exactly as the kernel forms it (one IEEE addition, the same bits), so only the
quotient's rounding is added.  The long-double value itself errs by 2^-11 of the bound; the factor 1.01 covers it."""
import numpy as np

LDBL = np.longdouble
U = 2.0 ** -53
SLACK = 1.01


def gamma(n):
    return n * U / (1.0 - n * U)


def _ld(a):
    return np.asarray(a, dtype=LDBL)


def gemm_nt(A, B, R16, K16, transpose_out=0, lam_r=None, lam_c=None):
    """(C, bound) of ``ldc_gemm_nt``: C = A[:16R, :16K] @ B[:16R, :16K].T, divided by lam_r[i] + lam_c[j] where both are
    given, transposed where asked; long double, and the elementwise bound on an fp64 evaluation of the same (the bound
    itself in fp64: its own rounding, 1e-14 of it, disappears in the factor 1.01)."""
    r, k = 16 * R16, 16 * K16
    a, b = np.asarray(A[:r, :k], float), np.asarray(B[:r, :k], float)
    c, mag, g = _ld(a) @ _ld(b).T, np.abs(a) @ np.abs(b).T, gamma(k)
    bound = g * mag
    if lam_r is not None:
        den = np.asarray(lam_r[:r], float)[:, None] + np.asarray(lam_c[:r], float)[None, :]     # fp64 sum, as on the device
        c, bound = c / _ld(den), (g + U * (1.0 + g)) * mag / np.abs(den)
    bound = SLACK * bound
    return (c.T, bound.T) if transpose_out else (c, bound)


def _stage(M, value, bound, n, left):
    """One product of the chain: M @ value (left) or value @ M.T in long double, with the running bound
    |M| bound + gamma_n |M| (|value| + bound) in fp64."""
    g, aM, reach = gamma(n), np.abs(M), np.abs(np.asarray(value, float)) + bound
    if left:
        return _ld(M) @ value, aM @ bound + g * (aM @ reach)
    return value @ _ld(M).T, bound @ aM.T + g * (reach @ aM.T)


def fastdiag(Qx, Qxinv, Qy, Qyinv, lamx, lamy, F):
    """(Psi, bound) of ``ldc_poisson_fastdiag`` on unpadded operators: Psi = Qx [(Qxinv F Qyinv^T) / (lamx_i + lamy_j)] Qy^T
    in long double, in the kernel's order of products, with the running bound of an fp64 evaluation carried through the
    four stages (n = the padded contraction length 16 ceil(max(mx, my) / 16))."""
    Qx, Qxinv, Qy, Qyinv = (np.asarray(a, float) for a in (Qx, Qxinv, Qy, Qyinv))
    n = 16 * ((max(F.shape) + 15) // 16)
    v, e = _stage(Qyinv, _ld(F), np.zeros(F.shape), n, left=False)   # X = F Qyinv^T
    v, e = _stage(Qxinv, v, e, n, left=True)                         # Qxinv X ...
    den = np.asarray(lamx, float)[:, None] + np.asarray(lamy, float)[None, :]            # fp64 sum, as on the device
    v, e = v / _ld(den), (e + U * (np.abs(np.asarray(v, float)) + e)) / np.abs(den)      # ... / (lamx_i + lamy_j): one rounding
    v, e = _stage(Qy, v, e, n, left=False)                           # Y = Phat Qy^T
    v, e = _stage(Qx, v, e, n, left=True)                            # Psi = Qx Y
    return v, SLACK * e


def _first(values, candidates, largest):
    """Flat index of the first (C order) extreme entry of ``values`` among ``candidates``; NaN is never one; -1 if none."""
    flat = values.ravel()
    ok = candidates.ravel() & ~np.isnan(flat)
    if not ok.any():
        return -1
    best = flat[ok].max() if largest else flat[ok].min()
    return int(np.flatnonzero(ok & (flat == best))[0])


def extrema(Psi, W, x, y, LD=None):
    """(val[5], idx[5]) by the documented rule of ``ldc_vortex_extrema_xy`` on Mx x My node arrays: 0 argmin Psi, 1 the
    SIGNED W at the argmax of |W|, 2-4 argmax Psi over BR (x > 0.5, y < 0.5), BL (x < 0.5, y < 0.5), TL (x < 0.5, y > 0.5),
    strict; first node in C order on ties; a NaN node is never chosen; idx = i * LD + j (LD: the device's row pitch,
    default My), and -1 / NaN where there is no candidate."""
    Mx, My = Psi.shape
    LD = My if LD is None else LD
    X, Y = np.asarray(x, float)[:Mx, None], np.asarray(y, float)[None, :My]
    everywhere = np.ones((Mx, My), dtype=bool)
    picks = [(Psi, everywhere, False, Psi), (np.abs(W), everywhere, True, W),
             (Psi, (X > 0.5) & (Y < 0.5), True, Psi), (Psi, (X < 0.5) & (Y < 0.5), True, Psi),
             (Psi, (X < 0.5) & (Y > 0.5), True, Psi)]
    val, idx = np.full(5, np.nan), np.full(5, -1, dtype=np.int64)
    for k, (key, mask, largest, source) in enumerate(picks):
        q = _first(key, mask, largest)
        if q >= 0:
            val[k], idx[k] = source.ravel()[q], (q // My) * LD + q % My
    return val, idx


def vortex_table(Psi, W, x, y):
    """The vortex-metrics dict that the host builds from ``extrema``: ValueError where psi_min or omega_max has no
    candidate, zeros for a corner region without a positive psi."""
    Mx, My = Psi.shape
    val, idx = extrema(Psi, W, x, y)
    if idx[0] < 0 or idx[1] < 0:
        raise ValueError("no finite node")
    at = lambda k: divmod(int(idx[k]), My)          # noqa: E731
    i, j = at(0)
    out = dict(psi_min=float(val[0]), psi_min_x=float(x[i]), psi_min_y=float(y[j]), omega_center=float(W[i, j]))
    i, j = at(1)
    out.update(omega_max=float(val[1]), omega_max_x=float(x[i]), omega_max_y=float(y[j]))
    for k, name in ((2, "BR"), (3, "BL"), (4, "TL")):
        vals = (0.0, 0.0, 0.0, 0.0)
        if idx[k] >= 0 and val[k] > 0:
            i, j = at(k)
            vals = (float(val[k]), float(W[i, j]), float(x[i]), float(y[j]))
        out[f"psi_{name}"], out[f"omega_{name}"], out[f"psi_{name}_x"], out[f"psi_{name}_y"] = vals
    return out


# ------------------------------------------------------------------------------------------------ seeded inputs
# (R16, K16, LD) of the product test: K = 3, 5, 7, 17 deal the four waves unequal shares of the k-groups; R != K both ways
GEMM_SHAPES = [(1, 1, 16), (1, 1, 32), (2, 1, 32), (1, 3, 48), (3, 2, 48), (2, 5, 96), (5, 4, 80), (4, 7, 112), (17, 17, 272)]
# inner sizes (Mx - 2, My - 2) of the streamfunction test
FASTDIAG_SIZES = [(7, 7), (15, 15), (16, 16), (17, 17), (31, 31), (19, 27), (47, 128), (128, 47), (127, 127), (255, 255),
                  (271, 271)]
# (Mx, My, LD) of the extrema test: 2 x 2 the smallest the ABI takes; up to 32 x 32 one node per thread at the most; beyond,
# the stride loop (33 x 31 = 1023 is the last size without it); LD > My throughout except 32 x 32
EXTREMA_SIZES = [(2, 2, 16), (9, 9, 16), (32, 32, 32), (31, 33, 48), (33, 31, 48), (33, 33, 48), (17, 129, 144), (257, 257, 272)]


def wide_range(rng, shape):
    """Normal entries times 10**uniform(-3, 3): sums of these cancel for real."""
    return rng.standard_normal(shape) * 10.0 ** rng.uniform(-3.0, 3.0, shape)


def lobatto(M):
    """Chebyshev-Gauss-Lobatto nodes on [0, 1]."""
    return 0.5 * (1.0 - np.cos(np.pi * np.arange(M) / (M - 1)))


def with_half(M):
    """Increasing nodes on [0, 1], one of them 0.5 exactly."""
    x = np.linspace(0.0, 1.0, M)
    x[M // 2] = 0.5
    return x


def smooth_plus_noise(rng, mx, my):
    s, t = np.linspace(0.0, 1.0, mx)[:, None], np.linspace(0.0, 1.0, my)[None, :]
    return np.sin(3.0 * s + 1.0) * np.cos(2.0 * t - 0.5) + 4.0 * s * t + 0.3 * rng.standard_normal((mx, my))


def orthogonal_times_diagonal(rng, m):
    """(Q, Q^-1): a random orthogonal matrix times a diagonal in [0.5, 2] (cond <= 4), and its inverse to long-double
    accuracy (two Newton steps X <- X (2 I - Q X) from the fp64 inverse) rounded to fp64."""
    O, _ = np.linalg.qr(rng.standard_normal((m, m)))
    Q = O * rng.uniform(0.5, 2.0, m)[None, :]
    X, Ql, two = _ld(np.linalg.inv(Q)), _ld(Q), 2 * np.eye(m, dtype=LDBL)
    for _ in range(2):
        X = X @ (two - Ql @ X)
    return Q, np.asarray(X, dtype=np.float64)


def fastdiag_case(kind, mx, my):
    """(Qx, Qxinv, Qy, Qyinv, lamx, lamy, F) for an mx x my inner grid.  ``chebyshev`` / ``legendre``: the solver's own
    ``_interior_eigenbasis`` of that basis' second-derivative matrices on [0, 1]; ``synthetic``: two different random
    well-conditioned bases with negative eigenvalues away from 0, in which a swap of x and y or a lost transposition
    cannot cancel.  F: seeded, smooth plus noise."""
    rng = np.random.default_rng(100000 + 1000 * mx + my)
    if kind == "synthetic":
        (Qx, Qxi), (Qy, Qyi) = orthogonal_times_diagonal(rng, mx), orthogonal_times_diagonal(rng, my)
        lamx, lamy = -rng.uniform(1.0, 300.0, mx), -rng.uniform(1.0, 300.0, my)
    else:
        from solvers.spectral.basis.spectral import ChebyshevLobattoBasis, LegendreLobattoBasis
        from solvers.spectral.sg import _axis_operators, _interior_eigenbasis
        basis = {"chebyshev": ChebyshevLobattoBasis, "legendre": LegendreLobattoBasis}[kind](domain=(0.0, 1.0))
        lamx, Qx, Qxi = _interior_eigenbasis(_axis_operators(basis, kind, mx + 2)[2])
        lamy, Qy, Qyi = _interior_eigenbasis(_axis_operators(basis, kind, my + 2)[2])
    return Qx, Qxi, Qy, Qyi, lamx, lamy, smooth_plus_noise(rng, mx, my)


def extrema_cases(Mx, My, seed=0):
    """[(name, Psi, W, x, y)] on an Mx x My node grid: the fields on which the rules of the kernel decide."""
    rng = np.random.default_rng(1000 * Mx + My + seed)
    n = Mx * My
    x, y = lobatto(Mx), lobatto(My)
    normal = lambda: rng.standard_normal((Mx, My))                         # noqa: E731
    integers = lambda: rng.integers(-3, 4, (Mx, My)).astype(float)         # noqa: E731
    cases = [("random", normal(), normal(), x, y)]

    def planted(a, b):
        """Integer fields -3 .. 3 (ties everywhere) with equal extrema at flat nodes a and b where the grid has them."""
        P, W = integers(), integers()
        for k, q in enumerate((a, b)):
            if q < n:
                P.ravel()[q], W.ravel()[q] = -7.0, (-9.0, 9.0)[k]
        return P, W
    cases.append(("ties_one_thread_two_strides", *planted(5, 5 + 1024), x, y))
    cases.append(("ties_last_thread_then_first", *planted(1023, 1024), x, y))
    cases.append(("constant", np.full((Mx, My), 2.5), np.full((Mx, My), -1.5), x, y))
    xh, yh = with_half(Mx), with_half(My)
    P = normal()
    P[xh == 0.5, :] = 10.0                                                  # the largest psi sits on the lines x = 0.5 and
    P[:, yh == 0.5] = 10.0                                                  # y = 0.5, which belong to no region
    cases.append(("nodes_at_one_half", P, normal(), xh, yh))
    cases.append(("region_without_positive_psi", -np.abs(integers()), normal(), x, y))
    cases.append(("empty_regions", normal(), normal(), np.linspace(0.6, 1.0, Mx), y))     # every x > 0.5: no BL, no TL
    W = rng.uniform(-1.0, 1.0, (Mx, My))
    W.ravel()[n // 3], W.ravel()[(2 * n) // 3] = 4.0, -5.0
    cases.append(("omega_max_is_negative", normal(), W, x, y))
    zeros = lambda: np.where(rng.random((Mx, My)) < 0.5, 0.0, -0.0)       # noqa: E731
    P, W = zeros(), zeros()
    P.ravel()[0], W.ravel()[0] = -0.0, 0.0
    cases.append(("signed_zeros", P, W, x, y))
    P, W = normal(), normal()
    P[rng.random((Mx, My)) < 0.3] = np.nan
    W[rng.random((Mx, My)) < 0.3] = np.nan
    P.ravel()[0] = W.ravel()[0] = np.nan
    fin = np.where(np.isnan(P), np.inf, P)
    P.ravel()[int(np.argmin(fin))] = np.nan                                # the smallest finite psi becomes NaN too
    cases.append(("some_nan", P, W, x, y))
    cases.append(("all_nan", np.full((Mx, My), np.nan), np.full((Mx, My), np.nan), x, y))
    return cases


def same_bits(a, b):
    """Equal as bit patterns (the sign of a zero counts), every NaN alike."""
    a, b = np.asarray(a, float), np.asarray(b, float)
    return bool(np.all((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))))


def runner_up_gap(values, mask):
    """Best minus second best of ``values`` over ``mask`` (largest first); inf with fewer than two nodes."""
    top = np.sort(values[mask])[-2:]
    return float(top[1] - top[0]) if top.size == 2 else np.inf
