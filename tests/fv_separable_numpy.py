"""NumPy restatement of the separable scaled preconditioner of the stretched-grid pressure CG (test helper;
csrc/ldc_fv_stretched_sep.hip, ldc_fv_set_preconditioner).

``FVSeparableState`` is ``fv_stretched_numpy.FVStretchedState`` with another ``precondition``; the operator, b, the start,
the stop rule, the cap and everything around the solve are the parent's.

  the model of D   G_ij = hx_i hy_j / (hy_j ax_i + hx_i ay_j), ax_i = 1 / dx[i] + 1 / dx[i+1] (the walls' d is h / 2): V / a_P of
                   pure diffusion, mu left out;
  its fit          l = log G, m = mean(l), a_i = exp(mean_j l_ij - m / 2), b_j = exp(mean_i l_ij - m / 2); on the inner faces
                   a_f[k] = g[k] a[k] + (1 - g[k]) a[k-1], the rule that takes D to a face;
  its operator     L_s = My (x) Kx^a + Ky^b (x) Mx, Kx^a the 1-D Neumann stiffness with the weights rho a_f / d, Mx = diag(hx a);
                   K q = lam M q, Q^T M Q = I, ascending, index 0 the zero mode;
                   L_s+ R = Qy ((Qy^T R Qx) / (lamy_a + lamx_b)) Qx^T with entry (0, 0) set to 0;
  the scaling      per solve s = sqrt(a_i b_j / D), D = V / (a_P + 1e-14);  z = s . L_s+ (s . r).
"""
from __future__ import annotations

import numpy as np

from fv_stretched_numpy import FVStretchedState


def separable_fit(hx, dxf, hy, dyf):
    """(a (nx), b (ny), G (ny, nx))."""
    ax = 1.0 / dxf[:-1] + 1.0 / dxf[1:]
    ay = 1.0 / dyf[:-1] + 1.0 / dyf[1:]
    G = (hy[:, None] * hx[None, :]) / (hy[:, None] * ax[None, :] + hx[None, :] * ay[:, None])
    ell = np.log(G)
    m = ell.mean()
    return np.exp(ell.mean(axis=0) - 0.5 * m), np.exp(ell.mean(axis=1) - 0.5 * m), G


def weighted_stiffness(d, g, a, rho=1.0):
    """The 1-D Neumann stiffness with the weights rho a_f / d on the inner faces."""
    n = a.size
    af = g[1:n] * a[1:] + (1.0 - g[1:n]) * a[:-1]
    w = rho * af / d[1:n]
    K = np.zeros((n, n))
    i = np.arange(n - 1)
    K[i, i] += w
    K[i + 1, i + 1] += w
    K[i, i + 1] -= w
    K[i + 1, i] -= w
    return K


def separable_eig(h, d, g, a, rho=1.0):
    """(lam ascending, Q as columns, K, M as a vector) of K q = lam M q with Q^T M Q = I."""
    from scipy.linalg import eigh
    K = weighted_stiffness(d, g, a, rho)
    M = h * a
    lam, Q = eigh(K, np.diag(M))
    # (lam[1] stays near rho (pi / L)^2 whatever n is, while lam[-1] grows like 1 / h_min^2: from about 600 cells on
    # lam[1] / lam[-1] falls below 1e-6, so lam[1] is held against the former, as the library holds it)
    assert abs(lam[0]) < 1e-9 * lam[-1] and lam[1] > 0.5 * rho * (np.pi / h.sum()) ** 2, "one zero mode, first"
    return lam, Q, K, M


def axis_table(a, lam, Q):
    """One axis' table of ldc_fv_set_preconditioner: [a (n) | lam (n) | Q (n x n, row-major, column k the k-th vector)]."""
    return np.concatenate([a, lam, np.ascontiguousarray(Q).ravel()])


class FVSeparableState(FVStretchedState):
    def __init__(self, *args, **kw):
        kw.setdefault("pressure_equation", "consistent")
        super().__init__(*args, **kw)
        self.sa, self.sb, self.G = separable_fit(self.hx, self.dxf, self.hy, self.dyf)
        self.slamx, self.sQx, self.sKx, self.sMx = separable_eig(self.hx, self.dxf, self.gxf, self.sa, self.rho)
        self.slamy, self.sQy, self.sKy, self.sMy = separable_eig(self.hy, self.dyf, self.gyf, self.sb, self.rho)
        den = self.slamx[None, :] + self.slamy[:, None]
        den[0, 0] = 1.0
        self.sinv_den = 1.0 / den
        self.sinv_den[0, 0] = 0.0
        self.scale = None                   # s of the solve in hand (solve_pressure sets it from D)

    def tables(self):
        return axis_table(self.sa, self.slamx, self.sQx), axis_table(self.sb, self.slamy, self.sQy)

    def separable_dense(self):
        """L_s = My (x) Kx^a + Ky^b (x) Mx as a dense matrix, cells c = j nx + i."""
        return np.kron(np.diag(self.sMy), self.sKx) + np.kron(self.sKy, np.diag(self.sMx))

    def separable_pinv(self, r):
        return self.sQy @ ((self.sQy.T @ r @ self.sQx) * self.sinv_den) @ self.sQx.T

    def scaling(self, D):
        return np.sqrt((self.sb[:, None] * self.sa[None, :]) / D)

    def precondition(self, r):
        return self.scale * self.separable_pinv(self.scale * r)

    def solve_pressure(self, D, rhs):
        self.scale = self.scaling(D)
        return super().solve_pressure(D, rhs)
