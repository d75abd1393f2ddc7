"""NumPy restatement of the finite-volume prolongation (include/ldc_fv.h, ldc_fv_prolong_enqueue; test helper).

``prolong(coarse, fine)`` takes two ``FVState`` objects of tests/fv_numpy.py and overwrites the fine one's u, v, p, fx and
fy with what the HIP kernel (csrc/ldc_fv_prolong.hip) computes from the coarse one, operation by operation in the same
order: the kernel is compiled without contraction of multiply-adds, so both round alike.  ``sequenced_run`` is the
coarse-to-fine sequence on the restatement: the bound of the GPU test and the lead-in check of the CPU test come from it.
"""
from __future__ import annotations

import numpy as np


def hierarchy(nx, ny, n_levels, coarsest_n, min_n=8):
    """(nx, ny) per level, coarse -> fine: halve both (n // 2) while both stay >= coarsest_n and >= min_n, at most
    n_levels levels.  Stated here on its own, not imported from the product."""
    out = [(int(nx), int(ny))]
    while len(out) < n_levels:
        cx, cy = out[-1][0] // 2, out[-1][1] // 2
        if min(cx, cy) < max(coarsest_n, min_n):
            break
        out.append((cx, cy))
    return out[::-1]


def nodes(n, h):
    """The extended coarse axis: 0, the n cell centres, n h."""
    return np.concatenate([[0.0], (np.arange(n) + 0.5) * h, [n * h]])


def locate(n_c, h_c, n_f, h_f):
    """(k, t) per fine centre: the left node (the largest node <= x, at most n_c) and the weight in its interval."""
    e = nodes(n_c, h_c)
    x = (np.arange(n_f) + 0.5) * h_f
    k = np.clip(np.searchsorted(e, x, side="right") - 1, 0, n_c)
    t = (x - e[k]) / (e[k + 1] - e[k])
    return k, t


def extend(f, kind, ulid=None):
    """The coarse (ny, nx) field with its ring: u, v = 0 on the walls and corners, u = ulid on the lid; p repeats the
    nearest cell."""
    ny, nx = f.shape
    if kind == "p":
        return np.pad(f, 1, mode="edge")
    g = np.zeros((ny + 2, nx + 2))
    g[1:-1, 1:-1] = f
    if kind == "u":
        g[-1, 1:-1] = ulid
    return g


def interpolate(g, kx, tx, ky, ty):
    """Bilinear, x first: lo = a + tx (b - a) on row ky, hi on row ky + 1, then lo + ty (hi - lo)."""
    KY, KX = ky[:, None], kx[None, :]
    TX, TY = tx[None, :], ty[:, None]
    a, b = g[KY, KX], g[KY, KX + 1]
    lo = a + TX * (b - a)
    a1, b1 = g[KY + 1, KX], g[KY + 1, KX + 1]
    hi = a1 + TX * (b1 - a1)
    return lo + TY * (hi - lo)


def prolong(coarse, fine):
    kx, tx = locate(coarse.nx, coarse.dx, fine.nx, fine.dx)
    ky, ty = locate(coarse.ny, coarse.dy, fine.ny, fine.dy)
    fine.u = interpolate(extend(coarse.u, "u", coarse.ulid), kx, tx, ky, ty)
    fine.v = interpolate(extend(coarse.v, "v"), kx, tx, ky, ty)
    p = interpolate(extend(coarse.p, "p"), kx, tx, ky, ty)
    fine.p = p - p[0, 0]
    ux, vy = fine.faces(fine.u, fine.v)
    fine.fx, fine.fy = fine.rho * ux * fine.dy, fine.rho * vy * fine.dx
    fine.fx[:, 0] = fine.fx[:, -1] = 0.0
    fine.fy[0, :] = fine.fy[-1, :] = 0.0
    return fine


def mdot(state):
    return np.concatenate([state.fx.ravel(), state.fy.ravel()])


def sequenced_run(make_state, sizes, tol, max_iter=20000):
    """Level by level on the restatement: ``make_state(nx, ny)`` builds an FVState, the coarsest starts from rest, every
    other from the prolongation of the level below, each to ``tol``.  Returns (states, record rows per level)."""
    states, rows = [], []
    for nx, ny in sizes:
        s = make_state(nx, ny)
        if states:
            prolong(states[-1], s)
        rows.append(s.run(max_iter, tol=tol))
        states.append(s)
    return states, rows


# max |difference| between the converged fine fields of the sequenced run 16^2 -> 32^2 and of the lone run from rest on
# the restatement (Re = 100, TVD, tolerance 1e-6: 1978 + 2824 iterations against 2760; both stop on a rate-bound rule).
# tests/test_fv_prolong_cpu.py checks the figures, tests/test_gpu_fv_fsg.py allows the device twice as much.
SEQ_16_32_DUV = 4.0e-4
SEQ_16_32_DP = 1.4e-3
