"""NumPy restatement of the SIMPLE iteration on a wall-clustered (tanh) tensor grid (test helper; csrc/ldc_fv_stretched.hip).

``FVStretchedState`` is ``fv_consistent_numpy.FVConsistentState`` with the geometry read from per-axis tables instead of
the two numbers dx, dy: the reference's own discretisation rules (its assembly, Rhie-Chow, gradient and pressure-matrix
code read ``face_interp_factors``, ``vector_d_CE``, ``d_Cb`` and ``cell_volumes``) on the mesh

    x_k = Lx s(k / nx),  y_k = Ly s(k / ny),  s(xi) = (1 + tanh(beta (2 xi - 1)) / tanh(beta)) / 2,  s(xi) = xi at beta = 0,

cell centres at the vertex midpoints.  Per axis: widths h (n), centre distances d_i = xc[i+1] - xc[i] and face weights
g_i = (xv[i+1] - xc[i]) / d_i (n - 1 inner faces; phi_f = g phi_N + (1 - g) phi_P), wall distances h_0 / 2 and h_{n-1} / 2,
V = hx_i hy_j.  The kernel's tables are ``axis_tables``: h (n), then d and g per face k = 0 .. n (the walls' d is h / 2).

What changes against the uniform restatement, statement for statement:
  gradient     the mean of the available one-sided slopes (f_N - f_P) / d, with the pinned-cell exclusions;
  assembly     inner diffusion mu |S| / d, wall diffusion mu |S| / (h / 2), pressure source - grad p V, D = V / (a_P + 1e-14),
               the lid profile at the stretched face centres; the deferred correction as it was;
  faces        g-weighted u*, v*, grad p, D and u', v'; walls the owner's value; mdot = rho u_f |S|, |S| = hy_j or hx_i;
  reference    A = Hy (x) Kx + Ky (x) Hx with weights rho |S| / d, solved exactly by fast diagonalisation with the generalised
               eigenpairs Kx q = lam Hx q, Q^T Hx Q = I: X = Qy ((Qy^T B Qx) / (lamy_a + lamx_b)) Qx^T, zero mode dropped,
               the c_0 and y - y_0 rules as they were (the uniform code's four products with ax = ay = 1); FV-Q4 kept;
  consistent   w_f = rho D_f |S| / d with the g-weighted D_f, PCG preconditioned by the operator above;
  omega, E, Z, P   d f / dx at P = (f_e - f_w) / hx_i with g-weighted face values and the wall's own value on wall faces
               (0; the lid PROFILE for u at the lid; 0 for omega), sums weighted by V.  At beta = 0 with a constant lid this
               is algebraically the ghost-cell rule of ``FVState``.
"""
from __future__ import annotations

import numpy as np

from fv_consistent_numpy import FVConsistentState


def tanh_vertices(n, L, beta):
    """The n + 1 vertices of one axis."""
    xi = np.arange(n + 1) / n
    if beta == 0:
        return L * xi
    return L * (0.5 * (1.0 + np.tanh(beta * (2.0 * xi - 1.0)) / np.tanh(beta)))


def axis_tables(xv):
    """(xc, h, d, g) of the vertices ``xv``: centres and widths (n); per face k = 0 .. n the distance d (walls: h / 2, inner:
    xc[k] - xc[k-1]) and the weight g of the cell behind the face, (xv[k] - xc[k-1]) / d (walls: 0, never read)."""
    xv = np.asarray(xv, float)
    n = xv.size - 1
    xc = 0.5 * (xv[:-1] + xv[1:])
    h = xv[1:] - xv[:-1]
    d, g = np.zeros(n + 1), np.zeros(n + 1)
    d[0], d[n] = 0.5 * h[0], 0.5 * h[-1]
    d[1:n] = xc[1:] - xc[:-1]
    g[1:n] = (xv[1:n] - xc[:-1]) / d[1:n]
    return xc, h, d, g


def generalised_eig(h, d, rho=1.0):
    """(lam ascending, Q as columns) of K q = lam H q with Q^T H Q = I: K the 1-D Neumann stiffness with the weights
    rho / d of the inner faces, H = diag(h).  Index 0 is the zero mode (a constant)."""
    from scipy.linalg import eigh
    n = h.size
    w = rho / d[1:n]
    K = np.zeros((n, n))
    i = np.arange(n - 1)
    K[i, i] += w
    K[i + 1, i + 1] += w
    K[i, i + 1] -= w
    K[i + 1, i] -= w
    lam, Q = eigh(K, np.diag(h))
    # (lam[1] stays near rho (pi / L)^2 whatever n is, while lam[-1] grows like 1 / h_min^2: from about 600 cells on
    # lam[1] / lam[-1] falls below 1e-6, so lam[1] is held against the former, as the library holds it)
    assert abs(lam[0]) < 1e-9 * lam[-1] and lam[1] > 0.5 * rho * (np.pi / h.sum()) ** 2, "one zero mode, first"
    return lam, Q


def lid_profile_at(xf, Lx=1.0, lid_velocity=1.0, corner_treatment="none", corner_smoothing=0.15):
    """u on the lid faces with centres ``xf``, as the reference's mesh builder evaluates it (simple_structured.py:244-262)."""
    xf = np.asarray(xf, float)
    xi = xf / Lx
    if corner_treatment in ("polynomial", "saad"):
        return 16.0 * xi**2 * (1.0 - xi) ** 2 * lid_velocity
    u = np.full(xf.size, float(lid_velocity))
    if corner_treatment == "smoothing":
        d = corner_smoothing * Lx
        lo, hi = xf < d, xf > (Lx - d)
        u[lo] = 0.5 * (1 - np.cos(np.pi * xf[lo] / d)) * lid_velocity
        u[hi & ~lo] = 0.5 * (1 - np.cos(np.pi * (Lx - xf[hi & ~lo]) / d)) * lid_velocity
    return u


class FVStretchedState(FVConsistentState):
    def __init__(self, nx, ny, Re, Lx=1.0, Ly=1.0, lid_velocity=1.0, corner_treatment="none", corner_smoothing=0.15,
                 grid_stretch=1.5, **kw):
        super().__init__(nx, ny, Re, Lx=Lx, Ly=Ly, lid_velocity=lid_velocity, corner_treatment=corner_treatment,
                         corner_smoothing=corner_smoothing, **kw)
        if not grid_stretch >= 0:
            raise ValueError(grid_stretch)
        self.beta = float(grid_stretch)
        self.xv, self.yv = tanh_vertices(nx, Lx, self.beta), tanh_vertices(ny, Ly, self.beta)
        self.xc, self.hx, self.dxf, self.gxf = axis_tables(self.xv)
        self.yc, self.hy, self.dyf, self.gyf = axis_tables(self.yv)
        self.V = self.hy[:, None] * self.hx[None, :]
        del self.dx, self.dy                # (nothing of the uniform geometry is read here)
        self.ulid = lid_profile_at(self.xc, Lx, lid_velocity, corner_treatment, corner_smoothing)
        self.lamx, self.Qx = generalised_eig(self.hx, self.dxf, self.rho)
        self.lamy, self.Qy = generalised_eig(self.hy, self.dyf, self.rho)
        den = self.lamx[None, :] + self.lamy[:, None]
        den[0, 0] = 1.0
        self.inv_den = 1.0 / den
        self.inv_den[0, 0] = 0.0

    # ------------------------------------------------------------------ pieces
    def gradient(self, f):
        """The mean of the one-sided slopes a cell has, pinned cell 0 zero and skipped by its neighbours."""
        dx, dy = self.dxf[1:-1][None, :], self.dyf[1:-1][:, None]
        okW = np.ones_like(f, bool)
        okW[:, 0] = False
        okW[0, 1] = False
        okE = np.ones_like(f, bool)
        okE[:, -1] = False
        okS = np.ones_like(f, bool)
        okS[0, :] = False
        okS[1, 0] = False
        okN = np.ones_like(f, bool)
        okN[-1, :] = False
        dW = np.zeros_like(f)
        dW[:, 1:] = (f[:, :-1] - f[:, 1:]) / (-dx)
        dE = np.zeros_like(f)
        dE[:, :-1] = (f[:, 1:] - f[:, :-1]) / dx
        dS = np.zeros_like(f)
        dS[1:, :] = (f[:-1, :] - f[1:, :]) / (-dy)
        dN = np.zeros_like(f)
        dN[:-1, :] = (f[1:, :] - f[:-1, :]) / dy
        sx = np.where(okW, dW, 0.0) + np.where(okE, dE, 0.0)
        cx = okW.astype(int) + okE.astype(int)
        sy = np.where(okS, dS, 0.0) + np.where(okN, dN, 0.0)
        cy = okS.astype(int) + okN.astype(int)
        gx = np.where(cx > 0, sx / np.maximum(cx, 1), 0.0)
        gy = np.where(cy > 0, sy / np.maximum(cy, 1), 0.0)
        gx[0, 0] = gy[0, 0] = 0.0
        return gx, gy

    def assemble(self):
        ny, nx = self.ny, self.nx
        Dx = self.mu * self.hy[:, None] / self.dxf[None, :]         # (ny, nx + 1): every x face, the walls included
        Dy = self.mu * self.hx[None, :] / self.dyf[:, None]         # (ny + 1, nx)
        fx, fy = self.fx, self.fy
        aP = np.zeros((ny, nx))
        aW, aE, aS, aN = (np.zeros((ny, nx)) for _ in range(4))
        mi, Di = fx[:, 1:-1], Dx[:, 1:-1]
        aP[:, :-1] += np.maximum(mi, 0) + Di
        aE[:, :-1] = np.minimum(mi, 0) - Di
        aP[:, 1:] += Di - np.minimum(mi, 0)
        aW[:, 1:] = -(np.maximum(mi, 0) + Di)
        mj, Dj = fy[1:-1, :], Dy[1:-1, :]
        aP[:-1, :] += np.maximum(mj, 0) + Dj
        aN[:-1, :] = np.minimum(mj, 0) - Dj
        aP[1:, :] += Dj - np.minimum(mj, 0)
        aS[1:, :] = -(np.maximum(mj, 0) + Dj)
        bu, bv = np.zeros((ny, nx)), np.zeros((ny, nx))
        for sl, mo, Db, bcu in (((slice(None), 0), -fx[:, 0], Dx[:, 0], 0.0), ((slice(None), nx - 1), fx[:, nx], Dx[:, nx], 0.0),
                                ((0, slice(None)), -fy[0, :], Dy[0, :], 0.0), ((ny - 1, slice(None)), fy[ny, :], Dy[ny, :], self.ulid)):
            aP[sl] += Db + mo
            bu[sl] += (Db + mo) * bcu
        if self.tvd:
            for phi, b in ((self.u, bu), (self.v, bv)):
                dc = self._dc(mi, phi[:, :-1], phi[:, 1:])
                b[:, :-1] -= dc
                b[:, 1:] += dc
                dc = self._dc(mj, phi[:-1, :], phi[1:, :])
                b[:-1, :] -= dc
                b[1:, :] += dc
        return (aP, aW, aE, aS, aN), bu, bv

    def faces(self, fu, fv, wall_x=None, wall_y=None):
        """+x / +y face values: g-weighted inside, the owner's value on the walls (or ``wall_x`` = (west, east) and
        ``wall_y`` = (south, north), the walls' own values)."""
        ny, nx = self.ny, self.nx
        g = self.gxf[1:-1][None, :]
        ux = np.empty((ny, nx + 1))
        ux[:, 1:-1] = g * fu[:, 1:] + (1.0 - g) * fu[:, :-1]
        ux[:, 0], ux[:, -1] = (fu[:, 0], fu[:, -1]) if wall_x is None else wall_x
        g = self.gyf[1:-1][:, None]
        vy = np.empty((ny + 1, nx))
        vy[1:-1, :] = g * fv[1:, :] + (1.0 - g) * fv[:-1, :]
        vy[0, :], vy[-1, :] = (fv[0, :], fv[-1, :]) if wall_y is None else wall_y
        return ux, vy

    def weights(self, D):
        gx, gy = self.gxf[1:-1][None, :], self.gyf[1:-1][:, None]
        wx = (self.rho * (gx * D[:, 1:] + (1.0 - gx) * D[:, :-1])) * (self.hy[:, None] / self.dxf[1:-1][None, :])
        wy = (self.rho * (gy * D[1:, :] + (1.0 - gy) * D[:-1, :])) * (self.hx[None, :] / self.dyf[1:-1][:, None])
        return wx, wy

    def reference_dense(self):
        """The constant-coefficient operator Hy (x) Kx + Ky (x) Hx as a dense matrix (weights rho |S| / d)."""
        wx = self.rho * self.hy[:, None] / self.dxf[1:-1][None, :] * np.ones((self.ny, self.nx - 1))
        wy = self.rho * self.hx[None, :] / self.dyf[1:-1][:, None] * np.ones((self.ny - 1, self.nx))
        return self.dense(wx, wy)

    # ------------------------------------------------------------------ one iteration
    def step(self, capture=None):
        u0, v0 = self.u, self.v
        hx, hy = self.hx[None, :], self.hy[:, None]
        gx, gy = self.gradient(self.p)
        d, bu, bv = self.assemble()
        aP = d[0]
        a = self.alpha_uv
        diagR = aP * (1.0 / a)
        scale = (1.0 - a) / a
        ru = bu - gx * self.V + scale * aP * u0
        rv = bv - gy * self.V + scale * aP * v0
        us = self.bicgstab(d, diagR, ru)
        vs = self.bicgstab(d, diagR, rv)
        D = self.V / (aP + 1e-14)
        # Rhie-Chow (FV-Q2: grad_p_bar minus the inline interpolation, zero to rounding)
        ux, vy = self.faces(us, vs)
        gxf, _ = self.faces(gx, gx)
        _, gyf = self.faces(gy, gy)
        Dxf, Dyf = self.faces(D, D)
        wx_, wy_ = self.gxf[1:-1][None, :], self.gyf[1:-1][:, None]
        ux[:, 1:-1] -= Dxf[:, 1:-1] * (gxf[:, 1:-1] - ((1.0 - wx_) * gx[:, :-1] + wx_ * gx[:, 1:]))
        vy[1:-1, :] -= Dyf[1:-1, :] * (gyf[1:-1, :] - ((1.0 - wy_) * gy[:-1, :] + wy_ * gy[1:, :]))
        fxs, fys = self.rho * (ux * hy), self.rho * (vy * hx)
        fxs[:, 0] = fxs[:, -1] = 0.0
        fys[0, :] = fys[-1, :] = 0.0
        rhs = -self.divergence(fxs, fys)
        rhs.flat[0] = 0.0
        if self.pressure_equation == "reference":
            pp = self.pressure_solve(rhs)
        else:
            pp, wx, wy = self.solve_pressure(D, rhs)
        gpx, gpy = self.gradient(pp)
        up, vp = -D * gpx, -D * gpy
        self.u, self.v = us + up, vs + vp
        self.p = self.p + self.alpha_p * pp
        if self.pressure_equation == "reference":
            upx, vpy = self.faces(up, vp)
            self.fx = fxs + self.rho * (upx * hy)         # FV-Q4: wall faces take rho u'_P |S|
            self.fy = fys + self.rho * (vpy * hx)
        else:
            self.fx, self.fy = fxs.copy(), fys.copy()
            self.fx[:, 1:-1] -= wx * (pp[:, 1:] - pp[:, :-1])
            self.fy[1:-1, :] -= wy * (pp[1:, :] - pp[:-1, :])
        self.u_prime, self.v_prime = up, vp
        if capture is not None:
            capture.update(grad_p=np.concatenate([gx.ravel(), gy.ravel()]),
                           diag=np.concatenate([x.ravel() for x in d]), b=np.concatenate([bu.ravel(), bv.ravel()]),
                           u_star=us.ravel(), v_star=vs.ravel(),
                           mdot_star=np.concatenate([fxs.ravel(), fys.ravel()]), rhs_p=rhs.ravel(),
                           p_prime=pp.ravel(), u_prime=up.ravel(), v_prime=vp.ravel(),
                           mdot=np.concatenate([self.fx.ravel(), self.fy.ravel()]))
        ch_u = np.linalg.norm(self.u - u0) / (np.linalg.norm(u0) + 1e-12)
        ch_v = np.linalg.norm(self.v - v0) / (np.linalg.norm(v0) + 1e-12)
        return np.array([max(ch_u, ch_v), np.linalg.norm(up), np.linalg.norm(vp),
                         np.linalg.norm(self.divergence(self.fx, self.fy)), *self.quantities(), 0.0])

    # ------------------------------------------------------------------ omega, E, Z, P (Gauss rule)
    def _gauss_grad(self, f, lid):
        """(d f / dx, d f / dy) at the cells: (f_e - f_w) / hx and (f_n - f_s) / hy; walls 0, the lid ``lid`` (nx values)."""
        zx, zy = np.zeros(self.ny), np.zeros(self.nx)
        fx, fy = self.faces(f, f, wall_x=(zx, zx), wall_y=(zy, lid))
        return (fx[:, 1:] - fx[:, :-1]) / self.hx[None, :], (fy[1:, :] - fy[:-1, :]) / self.hy[:, None]

    def vorticity(self):
        dvdx, _ = self._gauss_grad(self.v, np.zeros(self.nx))
        _, dudy = self._gauss_grad(self.u, self.ulid)
        return dvdx - dudy

    def quantities(self):
        w = self.vorticity()
        gx, gy = self._gauss_grad(w, np.zeros(self.nx))
        return (0.5 * float(np.sum((self.u * self.u + self.v * self.v) * self.V)), 0.5 * float(np.sum((w * w) * self.V)),
                0.5 * float(np.sum((gx**2 + gy**2) * self.V)))


# ---------------------------------------------------------------------- psi on the stretched grid (solvers.fv.solver)
def streamfunction_matrix(dxf, dyf):
    """The non-uniform 5-point operator on the interior cells (ring = 0): per axis
    (2 / (d_w + d_e)) ((psi_E - psi_P) / d_e - (psi_P - psi_W) / d_w), rows in the order j (outer), i (inner); dense."""
    nx, ny = dxf.size - 1, dyf.size - 1

    def axis(d, n):                         # (n - 2) x (n - 2), cells 1 .. n - 2; d[k] is the face between k - 1 and k
        T = np.zeros((n - 2, n - 2))
        for r, k in enumerate(range(1, n - 1)):
            dw, de = d[k], d[k + 1]
            s = 2.0 / (dw + de)
            T[r, r] = -s * (1.0 / de + 1.0 / dw)
            if r > 0:
                T[r, r - 1] = s / dw
            if r < n - 3:
                T[r, r + 1] = s / de
        return T
    return np.kron(np.eye(ny - 2), axis(dxf, nx)) + np.kron(axis(dyf, ny), np.eye(nx - 2))


# ---------------------------------------------------------------------- centreline extrema (Botella & Peyret's table)
BOTELLA_RE1000 = dict(u_min=-0.3885698, v_max=0.3769447, v_min=-0.5270771)


def _parabola_extremum(x, f, k):
    """The extremum of the parabola through (x[k-1 .. k+1], f[k-1 .. k+1]) (Newton form, any spacing)."""
    x0, x1, x2 = x[k - 1: k + 2]
    f0, f1, f2 = f[k - 1: k + 2]
    d01, d12 = (f1 - f0) / (x1 - x0), (f2 - f1) / (x2 - x1)
    c = (d12 - d01) / (x2 - x0)
    xs = 0.5 * (x0 + x1) - 0.5 * d01 / c
    return float(f0 + d01 * (xs - x0) + c * (xs - x0) * (xs - x1))


def centreline_extrema(u, v, xc, yc):
    """min u on the vertical centreline, max v and min v on the horizontal one, for (ny, nx) fields with even nx, ny on a grid
    that is symmetric about the centre: the centreline is a face, its value the mean of the two cells beside it; each extremum
    by a parabola through the three cells around the discrete one."""
    ny, nx = u.shape
    assert nx % 2 == 0 and ny % 2 == 0
    uc = 0.5 * (u[:, nx // 2 - 1] + u[:, nx // 2])
    vc = 0.5 * (v[ny // 2 - 1, :] + v[ny // 2, :])
    return dict(u_min=_parabola_extremum(yc, uc, int(np.argmin(uc))), v_max=_parabola_extremum(xc, vc, int(np.argmax(vc))),
                v_min=_parabola_extremum(xc, vc, int(np.argmin(vc))))
