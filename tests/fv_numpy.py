"""Vectorised NumPy restatement of one SIMPLE iteration of the finite-volume solver (test helper).

It states, array by array, what the HIP kernel (csrc/ldc_fv_kernel.inc) computes, so that the CPU suite can check the
arithmetic against the reference's fixtures (g14) and the GPU suite can check the TVD path, which the fixtures cannot
cover (DESIGN.md FV-Q1).  Same layouts as include/ldc_fv.h: cells ``c = j*nx + i`` as (ny, nx) arrays; face fluxes
``fx`` (ny, nx+1) in +x and ``fy`` (ny+1, nx) in +y; the momentum matrix as five diagonals.

The linear solves are the kernel's: Jacobi-preconditioned BiCGSTAB with SciPy's iteration and stopping rule
(rtol relative to |b|, atol = 0, x0 = 0, ``max_lin_iters`` = 1000 iterations, non-convergence accepted; ``iters``
and ``exits`` record each solve's count and which test ended it), and the pinned pressure correction by fast
diagonalisation.

``psi_up`` selects the TVD limiter value for faces with mdot >= 0 (FV-Q1): "muscl" (the product), "zero" or "one".
"""
from __future__ import annotations

import numpy as np


def lid_profile(nx, Lx=1.0, lid_velocity=1.0, corner_treatment="none", corner_smoothing=0.15):
    """u on the lid faces, as the reference's mesh builder evaluates it (simple_structured.py:244-262)."""
    x = np.linspace(0, Lx, nx + 1)
    xf = 0.5 * (x[:-1] + x[1:])
    xi = xf / Lx
    if corner_treatment in ("polynomial", "saad"):
        return 16.0 * xi**2 * (1.0 - xi) ** 2 * lid_velocity
    if corner_treatment == "smoothing":
        d = corner_smoothing * Lx
        u = np.full(nx, float(lid_velocity))
        lo, hi = xf < d, xf > (Lx - d)
        u[lo] = 0.5 * (1 - np.cos(np.pi * xf[lo] / d)) * lid_velocity
        u[hi & ~lo] = 0.5 * (1 - np.cos(np.pi * (Lx - xf[hi & ~lo]) / d)) * lid_velocity
        return u
    return np.full(nx, float(lid_velocity))


def neumann_eig(n):
    """Eigen-decomposition of the 1-D Neumann second difference (diag 1, 2, ..., 2, 1; off-diagonals -1)."""
    T = 2 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1)
    T[0, 0] = T[-1, -1] = 1.0
    lam, Q = np.linalg.eigh(T)
    return lam, Q


def muscl(r):
    return np.where(r > 0, np.maximum(0.0, np.minimum(np.minimum(2.0, 2.0 * r), 0.5 * (1 + r))), 0.0)


class FVState:
    def __init__(self, nx, ny, Re, Lx=1.0, Ly=1.0, lid_velocity=1.0, corner_treatment="none",
                 corner_smoothing=0.15, alpha_uv=0.4, alpha_p=0.2, linear_solver_tol=1e-9,
                 convection_scheme="TVD", psi_up="muscl", rho=1.0, max_lin_iters=1000):
        self.nx, self.ny = nx, ny
        self.dx, self.dy = Lx / nx, Ly / ny
        self.V = self.dx * self.dy
        self.rho = rho
        self.mu = rho * lid_velocity * Lx / Re
        self.lid = lid_velocity
        self.alpha_uv, self.alpha_p, self.tol = alpha_uv, alpha_p, linear_solver_tol
        self.tvd = convection_scheme == "TVD"
        self.psi_up = psi_up
        self.ulid = lid_profile(nx, Lx, lid_velocity, corner_treatment, corner_smoothing)
        self.u = np.zeros((ny, nx))
        self.v = np.zeros((ny, nx))
        self.p = np.zeros((ny, nx))
        self.fx = np.zeros((ny, nx + 1))
        self.fy = np.zeros((ny + 1, nx))
        self.lamx, self.Qx = neumann_eig(nx)
        self.lamy, self.Qy = neumann_eig(ny)
        ax, ay = self.dy / self.dx, self.dx / self.dy
        den = ax * self.lamx[None, :] + ay * self.lamy[:, None]
        den[0, 0] = 1.0
        self.inv_den = 1.0 / den
        self.inv_den[0, 0] = 0.0
        self.max_lin_iters = max_lin_iters
        self.iters = []                     # BiCGSTAB iterations of each momentum solve
        self.exits = []                     # and why each stopped: b0, r, s, rho, omega, rv or cap

    # ------------------------------------------------------------------ pieces
    def gradient(self, f):
        """Central differences, pinned cell 0 zero and skipped by its neighbours, one-sided at walls."""
        okW = np.ones_like(f, bool)
        okW[:, 0] = False
        okW[0, 1] = False                   # the west neighbour of cell 1 is the pinned cell
        okE = np.ones_like(f, bool)
        okE[:, -1] = False
        okS = np.ones_like(f, bool)
        okS[0, :] = False
        okS[1, 0] = False
        okN = np.ones_like(f, bool)
        okN[-1, :] = False
        dW = np.zeros_like(f)
        dW[:, 1:] = (f[:, :-1] - f[:, 1:]) / (-self.dx)
        dE = np.zeros_like(f)
        dE[:, :-1] = (f[:, 1:] - f[:, :-1]) / self.dx
        dS = np.zeros_like(f)
        dS[1:, :] = (f[:-1, :] - f[1:, :]) / (-self.dy)
        dN = np.zeros_like(f)
        dN[:-1, :] = (f[1:, :] - f[:-1, :]) / self.dy
        sx = np.where(okW, dW, 0.0) + np.where(okE, dE, 0.0)
        cx = okW.astype(int) + okE.astype(int)
        sy = np.where(okS, dS, 0.0) + np.where(okN, dN, 0.0)
        cy = okS.astype(int) + okN.astype(int)
        gx = np.where(cx > 0, sx / np.maximum(cx, 1), 0.0)
        gy = np.where(cy > 0, sy / np.maximum(cy, 1), 0.0)
        gx[0, 0] = gy[0, 0] = 0.0
        return gx, gy

    def _dc(self, m, phiP, phiN):
        """TVD deferred correction of a face with owner P (west / south) and neighbour N, flux m (P -> N)."""
        pos = m >= 0
        F_low = m * np.where(pos, phiP, phiN)
        r_pos = (phiN - phiP) / (phiP - (2 * phiP - phiN) + 1e-12)
        r_neg = (phiP - phiN) / (phiN - (2 * phiN - phiP) + 1e-12)
        psi_neg = muscl(r_neg)
        if self.psi_up == "muscl":
            psi_pos = muscl(r_pos)
        else:
            psi_pos = np.full_like(m, 0.0 if self.psi_up == "zero" else 1.0)
        psi = np.where(pos, psi_pos, psi_neg)
        up, down = np.where(pos, phiP, phiN), np.where(pos, phiN, phiP)
        return m * (up + 0.5 * psi * (down - up)) - F_low

    def assemble(self):
        """Five diagonals (aP unrelaxed) and the right-hand sides b_u, b_v before the pressure term."""
        ny, nx = self.ny, self.nx
        Dx, Dy = self.mu * self.dy / self.dx, self.mu * self.dx / self.dy
        Dbx, Dby = self.mu * self.dy / (0.5 * self.dx), self.mu * self.dx / (0.5 * self.dy)
        fx, fy = self.fx, self.fy
        aP = np.zeros((ny, nx))
        aW, aE, aS, aN = (np.zeros((ny, nx)) for _ in range(4))
        mi = fx[:, 1:-1]                    # internal x faces, owner (j, i), neighbour (j, i+1)
        aP[:, :-1] += np.maximum(mi, 0) + Dx
        aE[:, :-1] = np.minimum(mi, 0) - Dx
        aP[:, 1:] += Dx - np.minimum(mi, 0)
        aW[:, 1:] = -(np.maximum(mi, 0) + Dx)
        mj = fy[1:-1, :]
        aP[:-1, :] += np.maximum(mj, 0) + Dy
        aN[:-1, :] = np.minimum(mj, 0) - Dy
        aP[1:, :] += Dy - np.minimum(mj, 0)
        aS[1:, :] = -(np.maximum(mj, 0) + Dy)
        bu, bv = np.zeros((ny, nx)), np.zeros((ny, nx))
        # boundary faces: outward flux mo, diffusion 2 D; b += (Db + mo) * bc
        for sl, mo, Db, bcu in (((slice(None), 0), -fx[:, 0], Dbx, 0.0), ((slice(None), nx - 1), fx[:, nx], Dbx, 0.0),
                                ((0, slice(None)), -fy[0, :], Dby, 0.0), ((ny - 1, slice(None)), fy[ny, :], Dby, self.ulid)):
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

    @staticmethod
    def matvec(d, diagP, x):
        y = diagP * x
        y[:, 1:] += d[1][:, 1:] * x[:, :-1]
        y[:, :-1] += d[2][:, :-1] * x[:, 1:]
        y[1:, :] += d[3][1:, :] * x[:-1, :]
        y[:-1, :] += d[4][:-1, :] * x[1:, :]
        return y

    def bicgstab(self, d, diagP, b, maxiter=None):
        """SciPy's BiCGSTAB (right preconditioning) with a Jacobi preconditioner; non-convergence accepted."""
        maxiter = self.max_lin_iters if maxiter is None else maxiter
        bn = np.linalg.norm(b)
        if bn == 0:
            self.iters.append(0)
            self.exits.append("b0")
            return np.zeros_like(b)
        atol = self.tol * bn
        x = np.zeros_like(b)
        r = b.copy()
        rt = r.copy()
        rhotol = np.finfo(float).eps ** 2
        rho_prev = omega = alpha = None
        p = v = None
        it = 0
        why = "cap"
        for it in range(maxiter):
            if np.linalg.norm(r) < atol:
                why = "r"
                break
            rho = np.vdot(rt, r)
            if abs(rho) < rhotol:
                why = "rho"
                break
            if it > 0:
                if abs(omega) < rhotol:
                    why = "omega"
                    break
                beta = (rho / rho_prev) * (alpha / omega)
                p = r + beta * (p - omega * v)
            else:
                p = r.copy()
            phat = p / diagP
            v = self.matvec(d, diagP, phat)
            rv = np.vdot(rt, v)
            if rv == 0:
                why = "rv"
                break
            alpha = rho / rv
            s = r - alpha * v
            if np.linalg.norm(s) < atol:
                x = x + alpha * phat
                it += 1
                why = "s"
                break
            shat = s / diagP
            t = self.matvec(d, diagP, shat)
            omega = np.vdot(t, s) / np.vdot(t, t)
            x = x + alpha * phat + omega * shat
            r = s - omega * t
            rho_prev = rho
        else:
            it = maxiter
        self.iters.append(it)
        self.exits.append(why)
        return x

    def pressure_solve(self, b):
        """The pinned Neumann Laplacian solved exactly: c = b with c_0 = -sum_{i>=1} b_i, y = L^+ c, x = y - y_0."""
        c = b.copy()
        c.flat[0] = -np.sum(b.ravel()[1:])
        h = self.Qy.T @ c @ self.Qx
        y = self.Qy @ (h * self.inv_den) @ self.Qx.T
        return y - y.flat[0]

    def faces(self, fu, fv):
        """+x / +y face values: linear interpolation inside (g = 1/2), the owner's value on the walls."""
        ny, nx = self.ny, self.nx
        ux = np.empty((ny, nx + 1))
        ux[:, 1:-1] = 0.5 * fu[:, 1:] + (1.0 - 0.5) * fu[:, :-1]
        ux[:, 0], ux[:, -1] = fu[:, 0], fu[:, -1]
        vy = np.empty((ny + 1, nx))
        vy[1:-1, :] = 0.5 * fv[1:, :] + (1.0 - 0.5) * fv[:-1, :]
        vy[0, :], vy[-1, :] = fv[0, :], fv[-1, :]
        return ux, vy

    @staticmethod
    def divergence(fx, fy):
        return fx[:, 1:] - fx[:, :-1] + fy[1:, :] - fy[:-1, :]

    # ------------------------------------------------------------------ one iteration
    def step(self, capture=None):
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
        # Rhie-Chow (FV-Q2: grad_p_bar minus the inline interpolation, zero to rounding)
        ux, vy = self.faces(us, vs)
        gxf, _ = self.faces(gx, gx)
        _, gyf = self.faces(gy, gy)
        Dxf, Dyf = self.faces(D, D)
        ux[:, 1:-1] -= Dxf[:, 1:-1] * (gxf[:, 1:-1] - ((1.0 - 0.5) * gx[:, :-1] + 0.5 * gx[:, 1:]))
        vy[1:-1, :] -= Dyf[1:-1, :] * (gyf[1:-1, :] - ((1.0 - 0.5) * gy[:-1, :] + 0.5 * gy[1:, :]))
        fxs, fys = self.rho * ux * self.dy, self.rho * vy * self.dx
        fxs[:, 0] = fxs[:, -1] = 0.0        # wall faces carry the boundary velocity: no normal component
        fys[0, :] = fys[-1, :] = 0.0
        rhs = -self.divergence(fxs, fys)
        rhs.flat[0] = 0.0
        pp = self.pressure_solve(rhs)
        gpx, gpy = self.gradient(pp)
        up, vp = -D * gpx, -D * gpy
        self.u, self.v = us + up, vs + vp
        self.p = self.p + self.alpha_p * pp
        upx, vpy = self.faces(up, vp)
        self.fx = fxs + self.rho * upx * self.dy      # FV-Q4: wall faces take rho u'_P |S|
        self.fy = fys + self.rho * vpy * self.dx
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

    # ------------------------------------------------------------------ E, Z, P (ghost cells, base.py:359-450)
    def _ghost_grad(self, f, bc_lid):
        g = np.zeros((self.ny + 2, self.nx + 2))
        g[1:-1, 1:-1] = f
        g[0, 1:-1] = -f[0, :]
        g[-1, 1:-1] = 2 * bc_lid - f[-1, :]
        g[1:-1, 0] = -f[:, 0]
        g[1:-1, -1] = -f[:, -1]
        return ((g[1:-1, 2:] - g[1:-1, :-2]) / (2 * self.dx), (g[2:, 1:-1] - g[:-2, 1:-1]) / (2 * self.dy))

    def vorticity(self):
        dvdx, _ = self._ghost_grad(self.v, 0.0)
        _, dudy = self._ghost_grad(self.u, self.lid)
        return dvdx - dudy

    def quantities(self):
        dA = self.dx * self.dy
        w = self.vorticity()
        gx, gy = self._ghost_grad(w, 0.0)
        return (0.5 * float(np.sum(self.u * self.u + self.v * self.v) * dA), 0.5 * float(np.sum(w * w) * dA),
                0.5 * float(np.sum(gx**2 + gy**2) * dA))

    def set_state(self, u, v, p, mdot):
        ny, nx = self.ny, self.nx
        self.u, self.v, self.p = (np.asarray(a, float).reshape(ny, nx).copy() for a in (u, v, p))
        self.fx = np.asarray(mdot[: ny * (nx + 1)], float).reshape(ny, nx + 1).copy()
        self.fy = np.asarray(mdot[ny * (nx + 1):], float).reshape(ny + 1, nx).copy()

    def run(self, K, tol=None, warmup=10):
        """K iterations (or until the reference's latch: rel < tol after the warm-up); returns the record rows."""
        rows = []
        for k in range(K):
            rows.append(self.step())
            if tol is not None and k >= warmup and rows[-1][0] < tol:
                break
        return np.array(rows)
