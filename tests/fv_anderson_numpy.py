"""NumPy restatement of the Anderson acceleration of the finite-volume SIMPLE iteration (test helper).

It states what ``fv_anderson_kernel`` (csrc/ldc_fv_anderson.hip, include/ldc_fv.h) does after every SIMPLE iteration,
around ``fv_numpy.FVState.step``: the state is the concatenation ``[u | v | p | mdot]``, x the state the iteration
started from, g the state after it.

- The first iteration of a solve only keeps g as the next x (the device kernel has no x before it).  From the second
  on f = g - x; from the third on dG = g - g_prev and dF = f - f_prev replace the oldest of ``depth`` columns, a ring
  whose slot order is the order of the columns in the system.
- With ``it`` the count of iterations done: ``it < start`` or no column, the next state is g.  Otherwise A = dF^T dF
  and b = dF^T f over the u, v, p entries, lambda = 1e-12 trace(A) / m on the diagonal, A gamma = b by Cholesky, the
  next state g - sum_i gamma_i dG_i over all entries, p[0] written as 0.0.
- The fallback: a pivot that is not > 0 or a gamma that is not finite.  The next state is g, the ring is emptied,
  g_prev and f_prev stay, and the fallback is counted.
- A latched or NaN iteration is not mixed.

``cond`` is the largest 2-norm condition number of the regularised A the run has met.
"""
from __future__ import annotations

import numpy as np

LAMBDA = 1e-12
MAX_DEPTH = 16


def pack(s) -> np.ndarray:
    return np.concatenate([s.u.ravel(), s.v.ravel(), s.p.ravel(), s.fx.ravel(), s.fy.ravel()])


def unpack(s, x):
    n = s.nx * s.ny
    s.set_state(x[:n], x[n:2 * n], x[2 * n:3 * n], x[3 * n:])


def regularised(dF, f):
    """(A + lambda I, b) of the columns ``dF`` (rows: the u, v, p entries) and the residual ``f``."""
    m = dF.shape[1]
    A = dF.T @ dF
    return A + LAMBDA * np.trace(A) / m * np.eye(m), dF.T @ f


def cholesky_solve(A, b):
    """gamma of A gamma = b by the kernel's Cholesky, or None where it takes the fallback."""
    m = len(b)
    R = np.array(A, dtype=float)
    for i in range(m):
        for k in range(i + 1):
            s = R[i, k] - np.dot(R[i, :k], R[k, :k])
            if k == i:
                if not s > 0.0:
                    return None
                R[i, i] = np.sqrt(s)
            else:
                R[i, k] = s / R[k, k]
    y = np.zeros(m)
    for i in range(m):
        y[i] = (b[i] - np.dot(R[i, :i], y[:i])) / R[i, i]
    g = np.zeros(m)
    for i in range(m - 1, -1, -1):
        g[i] = (y[i] - np.dot(R[i + 1:, i], g[i + 1:])) / R[i, i]
    return g if np.all(np.isfinite(g)) else None


class Mixer:
    """The kernel's history of one trial: ``mix(g, it)`` returns the next state."""

    def __init__(self, n_cells: int, depth: int, start: int):
        if not (1 <= depth <= MAX_DEPTH and start >= 1):
            raise ValueError("depth 1 ... 16, start >= 1")
        self.n3, self.depth, self.start = 3 * n_cells, depth, start
        self.reset()
        self.cond, self.fallbacks, self.gammas = 0.0, 0, []

    def reset(self):
        """A zeroed astate: no x, no columns."""
        self.calls, self.ncol, self.pos = 0, 0, 0
        self.x = self.gp = self.fp = None
        self.dG = self.dF = None

    def mix(self, g: np.ndarray, it: int) -> np.ndarray:
        calls, self.calls = self.calls, self.calls + 1
        if calls == 0:
            self.x = g.copy()
            return g.copy()
        f = g - self.x
        if calls >= 2:
            if self.dG is None:
                self.dG, self.dF = np.zeros((g.size, self.depth)), np.zeros((g.size, self.depth))
            self.dG[:, self.pos], self.dF[:, self.pos] = g - self.gp, f - self.fp
            self.pos = (self.pos + 1) % self.depth
            self.ncol = min(self.ncol + 1, self.depth)
        self.gp, self.fp = g.copy(), f.copy()
        m = self.ncol
        nxt = g.copy()
        if it >= self.start and m > 0:
            A, b = regularised(self.dF[: self.n3, :m], f[: self.n3])
            with np.errstate(all="ignore"):
                gamma = cholesky_solve(A, b)
            if gamma is None:
                self.fallbacks += 1
                self.ncol, self.pos = 0, 0
            else:
                self.cond = max(self.cond, float(np.linalg.cond(A)))
                self.gammas.append(gamma)
                for k in range(m):
                    nxt = nxt - gamma[k] * self.dG[:, k]
                nxt[2 * (self.n3 // 3)] = 0.0
        self.x = nxt.copy()
        return nxt


def run(state, K, depth=5, start=10, tol=None, warmup=10):
    """K accelerated iterations of ``state`` (an ``FVState``), or until the latch (rel < tol once ``warmup`` iterations
    are done, tested on the SIMPLE iteration's own row as the kernel does); depth 0: the plain iteration.  Returns
    (record rows, the mixer or None)."""
    mixer = Mixer(state.nx * state.ny, depth, start) if depth > 0 else None
    rows = []
    for k in range(K):
        row = state.step()
        rows.append(row)
        if not np.isfinite(row[0]) or (tol is not None and k >= warmup and row[0] < tol):
            break
        if mixer is not None:
            unpack(state, mixer.mix(pack(state), k + 1))
    return np.array(rows), mixer
