"""NumPy restatement of the SIMPLE iteration with the consistent pressure equation (test helper; csrc/ldc_fv_wide_pressure.inc).

``FVConsistentState`` is ``fv_numpy.FVState`` with one change: the pressure correction is solved with the operator that
also corrects the face fluxes,

    (A x)_P = sum over the inner faces f of P of w_f (x_P - x_N),   w_f = rho (D_P / 2 + D_N / 2) |S_f| / d_f,

D = V / (a_P + 1e-14), b = rhs_p with entry 0 replaced by minus the sum of the others, p' = x - x_0, and the inner faces
take mdot = mdot* - w_f (p'_N - p'_P); wall faces stay exactly 0.0.  ``pressure_solver="direct"`` solves the pinned system
(x_0 = 0) by a dense solve; ``"cg"`` is the kernel's loop: conjugate gradients from x = 0, preconditioned by the fast
diagonalisation of the constant-coefficient Laplacian with the zero mode dropped, stopped at |r| <= pressure_tol |b| or after
``pressure_max_iters`` iterations.  ``pressure_equation="reference"`` is ``FVState``, statement for statement.
"""
from __future__ import annotations

import numpy as np

from fv_numpy import FVState


class FVConsistentState(FVState):
    def __init__(self, *args, pressure_equation="consistent", pressure_solver="cg", pressure_tol=1e-8,
                 pressure_max_iters=200, **kw):
        super().__init__(*args, **kw)
        if pressure_equation not in ("reference", "consistent"):
            raise ValueError(pressure_equation)
        self.pressure_equation, self.pressure_solver = pressure_equation, pressure_solver
        self.pressure_tol, self.pressure_max_iters = float(pressure_tol), int(pressure_max_iters)
        self.cg_iters = []                  # CG iterations of every pressure solve
        self.cg_caps = 0                    # solves accepted at the cap
        self.last = {}                      # b, x, the weights and |b| of the last pressure solve

    # ------------------------------------------------------------------ the operator
    def weights(self, D):
        """w on the inner x faces (ny, nx - 1) and the inner y faces (ny - 1, nx)."""
        wx = (self.rho * (0.5 * D[:, :-1] + 0.5 * D[:, 1:])) * (self.dy / self.dx)
        wy = (self.rho * (0.5 * D[:-1, :] + 0.5 * D[1:, :])) * (self.dx / self.dy)
        return wx, wy

    @staticmethod
    def apply(wx, wy, x):
        y = np.zeros_like(x)
        dxf = wx * (x[:, 1:] - x[:, :-1])
        dyf = wy * (x[1:, :] - x[:-1, :])
        y[:, :-1] -= dxf
        y[:, 1:] += dxf
        y[:-1, :] -= dyf
        y[1:, :] += dyf
        return y

    def dense(self, wx, wy):
        """A as a dense (n, n) matrix, cells c = j nx + i."""
        ny, nx = self.ny, self.nx
        n = nx * ny
        A = np.zeros((n, n))
        c = np.arange(n).reshape(ny, nx)
        for w, P, N in ((wx, c[:, :-1], c[:, 1:]), (wy, c[:-1, :], c[1:, :])):
            P, N, w = P.ravel(), N.ravel(), w.ravel()
            np.add.at(A, (P, P), w)
            np.add.at(A, (N, N), w)
            np.add.at(A, (P, N), -w)
            np.add.at(A, (N, P), -w)
        return A

    def precondition(self, r):
        """z = L+ r: the fast diagonalisation without the zero mode (no entry-0 insertion, no shift)."""
        return self.Qy @ ((self.Qy.T @ r @ self.Qx) * self.inv_den) @ self.Qx.T

    def pcg(self, wx, wy, b):
        """The kernel's loop; returns (x, iterations, accepted at the cap)."""
        bn = np.linalg.norm(b)
        x = np.zeros_like(b)
        if bn == 0:
            return x, 0, False
        r = b.copy()
        p = rz_prev = None
        for k in range(self.pressure_max_iters):
            if np.linalg.norm(r) <= self.pressure_tol * bn:
                return x, k, False
            z = self.precondition(r)
            rz = float(np.sum(r * z))
            p = z if k == 0 else z + (rz / rz_prev) * p
            q = self.apply(wx, wy, p)
            alpha = rz / float(np.sum(p * q))
            x = x + alpha * p
            r = r - alpha * q
            rz_prev = rz
        return x, self.pressure_max_iters, bool(np.linalg.norm(r) > self.pressure_tol * bn)

    def solve_pressure(self, D, rhs):
        """p' = x - x_0 of A x = b, and the weights."""
        wx, wy = self.weights(D)
        b = rhs.copy()
        b.flat[0] = -np.sum(rhs.ravel()[1:])
        if self.pressure_solver == "direct":
            A = self.dense(wx, wy)
            x = np.zeros(b.size)
            x[1:] = np.linalg.solve(A[1:, 1:], b.ravel()[1:])
            x = x.reshape(b.shape)
            its = 0
        else:
            x, its, capped = self.pcg(wx, wy, b)
            self.cg_iters.append(its)
            self.cg_caps += int(capped)
        self.last = dict(b=b, x=x, wx=wx, wy=wy, bnorm=float(np.linalg.norm(b)), iters=its)
        return x - x.flat[0], wx, wy

    # ------------------------------------------------------------------ one iteration
    def step(self, capture=None):
        if self.pressure_equation == "reference":
            return super().step(capture)
        u0, v0 = self.u, self.v
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
        ux, vy = self.faces(us, vs)
        gxf, _ = self.faces(gx, gx)
        _, gyf = self.faces(gy, gy)
        Dxf, Dyf = self.faces(D, D)
        ux[:, 1:-1] -= Dxf[:, 1:-1] * (gxf[:, 1:-1] - ((1.0 - 0.5) * gx[:, :-1] + 0.5 * gx[:, 1:]))
        vy[1:-1, :] -= Dyf[1:-1, :] * (gyf[1:-1, :] - ((1.0 - 0.5) * gy[:-1, :] + 0.5 * gy[1:, :]))
        fxs, fys = self.rho * ux * self.dy, self.rho * vy * self.dx
        fxs[:, 0] = fxs[:, -1] = 0.0
        fys[0, :] = fys[-1, :] = 0.0
        rhs = -self.divergence(fxs, fys)
        rhs.flat[0] = 0.0
        pp, wx, wy = self.solve_pressure(D, rhs)
        gpx, gpy = self.gradient(pp)
        up, vp = -D * gpx, -D * gpy
        self.u, self.v = us + up, vs + vp
        self.p = self.p + self.alpha_p * pp
        self.fx, self.fy = fxs.copy(), fys.copy()
        self.fx[:, 1:-1] -= wx * (pp[:, 1:] - pp[:, :-1])         # wall faces: exactly 0.0 (FV-Q4 does not apply)
        self.fy[1:-1, :] -= wy * (pp[1:, :] - pp[:-1, :])
        self.u_prime, self.v_prime = up, vp
        if capture is not None:
            capture.update(u_star=us.ravel(), v_star=vs.ravel(), mdot_star=np.concatenate([fxs.ravel(), fys.ravel()]),
                           rhs_p=rhs.ravel(), p_prime=pp.ravel(), u_prime=up.ravel(), v_prime=vp.ravel(),
                           mdot=np.concatenate([self.fx.ravel(), self.fy.ravel()]))
        ch_u = np.linalg.norm(self.u - u0) / (np.linalg.norm(u0) + 1e-12)
        ch_v = np.linalg.norm(self.v - v0) / (np.linalg.norm(v0) + 1e-12)
        return np.array([max(ch_u, ch_v), np.linalg.norm(up), np.linalg.norm(vp),
                         np.linalg.norm(self.divergence(self.fx, self.fy)), *self.quantities(), 0.0])
