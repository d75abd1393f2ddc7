"""NumPy restatement of the transfer of a finite-volume state to the nodes of a tensor grid (include/ldc_fv.h,
ldc_fv_sample_nodes; test helper), and of the spectral solve that starts from it.

``sample(...)`` returns what the HIP kernel (csrc/ldc_fv_sample.hip) computes, operation by operation in the same order:
the ring, the nodes of the extended axis and the bilinear rule are the functions of tests/fv_prolong_numpy.py (the
roundings are stated there, once); what is added here is the left node of an ARBITRARY coordinate and the target's own
boundary values.  ``seed_oracle`` runs a ``FVConsistentState`` to its tolerance and puts the sampled state into an
``OracleSG``: the counts of DESIGN.md 3 come from it.
"""
from __future__ import annotations

import numpy as np

import fv_prolong_numpy as P


def locate_at(n, h, x):
    """(k, t) per coordinate: the left node of the extended axis (the largest node <= x, at most n) and the weight in its
    interval -- ``fv_prolong_numpy.locate`` for coordinates that are not cell centres of a fine grid."""
    e = P.nodes(n, h)
    x = np.asarray(x, dtype=np.float64)
    k = np.clip(np.searchsorted(e, x, side="right") - 1, 0, n)
    t = (x - e[k]) / (e[k + 1] - e[k])
    return k, t


def sample(u, v, p, ulid, dx, dy, x, y, ulid_nodes):
    """U, V (Mx, My) and P (Mx - 2, My - 2), indexed [ix, iy], from the FV fields u, v, p (ny, nx) with lid profile
    ``ulid`` (nx): the bilinear interpolant of the ring-extended field at the interior nodes, x first; the target's
    boundary values on the boundary (walls 0.0, the lid ``ulid_nodes``, which wins the two top corners); p not shifted."""
    ny, nx = u.shape
    kx, tx = locate_at(nx, dx, x)
    ky, ty = locate_at(ny, dy, y)
    U = P.interpolate(P.extend(u, "u", ulid), kx, tx, ky, ty).T.copy()
    V = P.interpolate(P.extend(v, "v"), kx, tx, ky, ty).T.copy()
    Pf = P.interpolate(P.extend(p, "p"), kx, tx, ky, ty).T
    for f in (U, V):
        f[0, :] = 0.0
        f[-1, :] = 0.0
        f[:, 0] = 0.0
    U[:, -1] = ulid_nodes
    V[:, -1] = 0.0
    return U, V, np.ascontiguousarray(Pf[1:-1, 1:-1])


def sample_state(state, x, y, ulid_nodes):
    """``sample`` of an ``FVState`` (tests/fv_numpy.py)."""
    return sample(state.u, state.v, state.p, state.ulid, state.dx, state.dy, x, y, ulid_nodes)


def seed_cells(N, cells=0):
    return int(cells) if cells else max(16, int(N))


def fv_seed(Re, nx, ny, tol, alpha_uv=0.7, alpha_p=0.3, max_iter=20000, **kw):
    """The FV seed on the restatement: ``FVConsistentState``, TVD, run to ``tol``.  Returns (state, iterations, latched);
    a state that went NaN comes back with latched False."""
    from fv_consistent_numpy import FVConsistentState
    s = FVConsistentState(nx, ny, Re, alpha_uv=alpha_uv, alpha_p=alpha_p, convection_scheme="TVD", **kw)
    its, latched = 0, False
    with np.errstate(all="ignore"):
        for k in range(max_iter):                 # FVState.run with a stop on the first record that is not finite
            row = s.step()
            its = k + 1
            if not np.all(np.isfinite(row)):
                break
            if k >= 10 and row[0] < tol:
                latched = True
                break
    return s, its, latched


def put(oracle, state):
    """The sampled FV state as the oracle's u, v, p (its own nodes and lid profile)."""
    oracle.u, oracle.v, oracle.p = sample_state(state, oracle.ax.x, oracle.ay.x, oracle.u_lid)
    return oracle


def seed_oracle(N, Re, cells=0, seed_tol=1e-6, ny=None, **oracle_kw):
    """An ``OracleSG`` started from the FV seed of ``cells`` (0: max(16, N)) cells per axis; (oracle, seed iterations)."""
    from oracle.ldc_oracle import OracleSG
    o = OracleSG(N, Re, ny=ny, **oracle_kw)
    fv_kw = dict(Lx=o.Lx, Ly=o.Ly, lid_velocity=o.U)
    for k in ("corner_treatment", "corner_smoothing"):
        fv_kw[k] = oracle_kw.get(k, dict(corner_treatment="smoothing", corner_smoothing=0.15)[k])
    s, its, ok = fv_seed(Re, seed_cells(N, cells), seed_cells(o.Ny, cells), seed_tol, **fv_kw)
    if not ok:
        raise RuntimeError(f"the FV seed did not converge in {its} iterations")
    return put(o, s), its
