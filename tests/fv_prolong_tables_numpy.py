"""NumPy restatement of the finite-volume transfer on tensor grids with any spacing per axis (include/ldc_fv.h,
ldc_fv_prolong_tables_enqueue; test helper).

``prolong(coarse, fine)`` takes two states that expose ``xc``, ``yc``, the tables ``hx``, ``hy``, ``gxf``, ``gyf`` and
``faces`` -- an ``FVStretchedState`` of tests/fv_stretched_numpy.py (or a subclass), or a uniform ``FVState`` wrapped by
``with_tables`` -- and overwrites the fine one's u, v, p, fx and fy with what the HIP kernel (csrc/ldc_fv_prolong_tables.hip)
computes from the coarse one, operation by operation in the same order: the kernel is compiled without contraction of
multiply-adds, so both round alike.  The ring, the interpolant and the pin of p are those of tests/fv_prolong_numpy.py
(``extend``, ``interpolate``); the nodes come from the coarse centre tables and the fluxes from the fine face tables.
``sequenced_run`` is the coarse-to-fine sequence on the restatement, as tests/fv_prolong_numpy.py has it.
"""
from __future__ import annotations

import numpy as np

from fv_prolong_numpy import extend, hierarchy, interpolate, mdot  # noqa: F401  (hierarchy, mdot: for the tests)
from fv_stretched_numpy import axis_tables, tanh_vertices


def with_tables(state, Lx=1.0, Ly=1.0):
    """A uniform ``FVState`` with the equal-spacing tables of its mesh attached (the vertices k L / n through ``axis_tables``,
    as ``solvers.fv.solver.transfer_axis`` builds them at beta = 0), and ``faces`` by those tables.  Returns the state."""
    state.Lx, state.Ly = float(Lx), float(Ly)
    state.xc, state.hx, state.dxf, state.gxf = axis_tables(tanh_vertices(state.nx, Lx, 0.0))
    state.yc, state.hy, state.dyf, state.gyf = axis_tables(tanh_vertices(state.ny, Ly, 0.0))
    return state


def domain(state):
    """(Lx, Ly) of a state: the last vertex of a stretched one, what ``with_tables`` was given for a wrapped uniform one."""
    if hasattr(state, "xv"):
        return float(state.xv[-1]), float(state.yv[-1])
    return state.Lx, state.Ly


def nodes(xc, L):
    """The extended coarse axis: 0, the n cell centres, L."""
    return np.concatenate([[0.0], np.asarray(xc, float), [float(L)]])


def locate(xc_c, L, xc_f):
    """(k, t) per fine centre: the left node (the largest node <= x, at most n_c) and the weight in its interval."""
    e = nodes(xc_c, L)
    x = np.asarray(xc_f, float)
    k = np.clip(np.searchsorted(e, x, side="right") - 1, 0, len(xc_c))
    t = (x - e[k]) / (e[k + 1] - e[k])
    return k, t


def table_faces(state, fu, fv):
    """The inner +x / +y face values by the tables, in the order of ``FVStretchedState.faces``: g f_N + (1 - g) f_P."""
    g = state.gxf[1:-1][None, :]
    ux = g * fu[:, 1:] + (1.0 - g) * fu[:, :-1]
    g = state.gyf[1:-1][:, None]
    vy = g * fv[1:, :] + (1.0 - g) * fv[:-1, :]
    return ux, vy


def prolong(coarse, fine):
    Lx, Ly = domain(fine)
    kx, tx = locate(coarse.xc, Lx, fine.xc)
    ky, ty = locate(coarse.yc, Ly, fine.yc)
    fine.u = interpolate(extend(coarse.u, "u", coarse.ulid), kx, tx, ky, ty)
    fine.v = interpolate(extend(coarse.v, "v"), kx, tx, ky, ty)
    p = interpolate(extend(coarse.p, "p"), kx, tx, ky, ty)
    fine.p = p - p[0, 0]
    ux, vy = table_faces(fine, fine.u, fine.v)
    ny, nx = fine.u.shape
    fine.fx, fine.fy = np.zeros((ny, nx + 1)), np.zeros((ny + 1, nx))           # the wall faces: exactly 0.0
    fine.fx[:, 1:-1] = fine.rho * (ux * fine.hy[:, None])
    fine.fy[1:-1, :] = fine.rho * (vy * fine.hx[None, :])
    return fine


def sequenced_run(make_state, sizes, tol, max_iter=20000):
    """Level by level on the restatement: ``make_state(nx, ny)`` builds a state with tables, the coarsest starts from rest,
    every other from the prolongation of the level below, each to ``tol``.  Returns (states, record rows per level)."""
    states, rows = [], []
    for nx, ny in sizes:
        s = make_state(nx, ny)
        if states:
            prolong(states[-1], s)
        rows.append(s.run(max_iter, tol=tol))
        states.append(s)
    return states, rows


# The sequenced run 16^2 -> 32^2 against the lone 32^2 run from rest on the restatement (FVSeparableState: Re = 100, TVD,
# alpha 0.4 / 0.2, beta 1.5, consistent pressure equation with the separable preconditioner, tolerance 1e-6): iterations per
# level, of the lone run, and max |difference| of the converged fine fields.  tests/test_fv_prolong_tables_cpu.py checks the
# figures, tests/test_gpu_fv_fsg_tables.py allows the device twice the differences and one iteration either way.
# Measured: 441 + 569 iterations against 864 (all three stop on the rate-bound rule), 1.11e-4 in u and v, 1.07e-3 in p.
SEQ_16_32_ITERS = (441, 569)
SEQ_16_32_LONE_ITERS = 864
SEQ_16_32_DUV = 1.2e-4
SEQ_16_32_DP = 1.1e-3
