#!/usr/bin/env python3
"""Generate the g17 fixtures: the *reference* FV solver on a wall-clustered (tanh) tensor grid.

TEST INFRASTRUCTURE, like make_golden_fv.py, whose stand-ins and helpers it imports.  The reference's discretisation is
mesh-general (its assembly, Rhie-Chow, gradient and pressure-matrix code read ``face_interp_factors``, ``vector_d_CE``,
``d_Cb`` and ``cell_volumes``); only its mesh builder is uniform.  So, while a solver is constructed, ``linspace`` inside the
reference's mesh module returns the tanh vertices

    x_k = L s(k / n),  s(xi) = (1 + tanh(beta (2 xi - 1)) / tanh(beta)) / 2,

then ``mesh.cell_volumes`` is overwritten with the true areas and ``A_p`` rebuilt.  Faces are mapped to (j, i) by
``searchsorted`` on the vertices (``faces_to_structured`` of make_golden_fv.py assumes uniform spacing).

All cases are Upwind with LINEAR_TOL 1e-12.  Record columns 4 - 6 (E, Z, P) are the reference's uniform ghost-cell formulas
and mean nothing here: the trajectories keep columns 0 - 3.

Usage:  python tests/golden/make_golden_fv_stretched.py
"""
from __future__ import annotations

import importlib
import json

import numpy as np

import make_golden_fv as G

OUT = G.OUT
WIDE = G.WIDE


def tanh_vertices(n, L, beta):
    xi = np.arange(n + 1) / n
    if beta == 0:
        return L * xi
    return L * (0.5 * (1.0 + np.tanh(beta * (2.0 * xi - 1.0)) / np.tanh(beta)))


class _StretchedNumpy:
    """numpy, but ``linspace(0, L, n + 1)`` gives the tanh vertices."""

    def __init__(self, beta):
        self._beta = beta

    def __getattr__(self, name):
        return getattr(np, name)

    def linspace(self, lo, hi, num):
        assert lo == 0
        return tanh_vertices(num - 1, hi, self._beta)


def make_fv(nx, ny, Re, beta, lid="none", **kw):
    G._install_shims()
    meshmod = importlib.import_module("shared.meshing.simple_structured")
    real = meshmod.np
    meshmod.np = _StretchedNumpy(beta)
    try:
        mod, s = G.make_fv(nx, ny, Re, lid=lid, **kw)
    finally:
        meshmod.np = real
    xv, yv = tanh_vertices(nx, s.params.Lx, beta), tanh_vertices(ny, s.params.Ly, beta)
    hx, hy = np.diff(xv), np.diff(yv)
    s.mesh.cell_volumes[:] = (hy[:, None] * hx[None, :]).ravel()
    xc, yc = 0.5 * (xv[:-1] + xv[1:]), 0.5 * (yv[:-1] + yv[1:])
    X, Y = np.meshgrid(xc, yc)
    assert np.allclose(s.mesh.cell_centers[:, 0], X.ravel(), atol=1e-14) and np.allclose(s.mesh.cell_centers[:, 1], Y.ravel(), atol=1e-14)
    s.A_p = s._build_pressure_correction_matrix()
    s._xv, s._yv = xv, yv
    return mod, s


def faces_to_structured(s, mdot):
    """Reference face array -> [fx (ny, nx+1) | fy (ny+1, nx)] fluxes in +x / +y, faces found by their coordinates."""
    m = s.mesh
    nx, ny = s.params.nx, s.params.ny
    xv, yv = s._xv, s._yv
    xm, ym = 0.5 * (xv[:-1] + xv[1:]), 0.5 * (yv[:-1] + yv[1:])
    fx, fy = np.full((ny, nx + 1), np.nan), np.full((ny + 1, nx), np.nan)
    for f in range(mdot.shape[0]):
        S, fc = m.vector_S_f[f], m.face_centers[f]
        if abs(S[0]) > abs(S[1]):
            i, j = int(np.argmin(np.abs(xv - fc[0]))), int(np.searchsorted(yv, fc[1]) - 1)
            assert abs(xv[i] - fc[0]) < 1e-12 and abs(ym[j] - fc[1]) < 1e-12
            fx[j, i] = mdot[f] * np.sign(S[0])
        else:
            i, j = int(np.searchsorted(xv, fc[0]) - 1), int(np.argmin(np.abs(yv - fc[1])))
            assert abs(xm[i] - fc[0]) < 1e-12 and abs(yv[j] - fc[1]) < 1e-12
            fy[j, i] = mdot[f] * np.sign(S[1])
    assert not np.isnan(fx).any() and not np.isnan(fy).any()
    return np.concatenate([fx.ravel(), fy.ravel()])


def seed_state(s, rng):
    """make_golden_fv.seed_state with this file's face map."""
    from solvers.fv.assembly.rhie_chow import mdot_calculation
    from solvers.fv.core.helpers import interpolate_velocity_to_face
    x, y = s.mesh.cell_centers[:, 0], s.mesh.cell_centers[:, 1]

    def smooth():
        f = np.zeros_like(x)
        for kx in range(1, 4):
            for ky in range(1, 4):
                f += rng.normal() / (kx * ky) * np.sin(np.pi * kx * x) * np.sin(np.pi * ky * y)
        return 0.3 * f
    a = s.arrays
    a.u[:], a.v[:], a.p[:] = smooth(), smooth(), smooth()
    a.mdot[:] = mdot_calculation(s.mesh, s.rho, interpolate_velocity_to_face(s.mesh, a.u, a.v))
    return a.u.copy(), a.v.copy(), a.p.copy(), faces_to_structured(s, a.mdot)


def step_group(out, meta, seed, cases):
    for tag, nx, ny, Re, beta, kw in cases:
        mod, s = make_fv(nx, ny, Re, beta, **kw)
        rng = np.random.default_rng(seed)
        u0, v0, p0, m0 = seed_state(s, rng)
        cap = {"asm": [], "solve": []}
        real_asm, real_solve = mod.assemble_diffusion_convection_matrix, mod.scipy_solver

        def asm(*a, **k):
            r = real_asm(*a, **k)
            cap["asm"].append(r)
            return r

        def solve(A, b, **k):
            x, M = real_solve(A, b, **k)
            cap["solve"].append((b.copy(), x.copy()))
            return x, M
        mod.assemble_diffusion_convection_matrix, mod.scipy_solver = asm, solve
        try:
            s.step()
        finally:
            mod.assemble_diffusion_convection_matrix, mod.scipy_solver = real_asm, real_solve
        a = s.arrays
        row, col, data, bu = cap["asm"][0]
        diag = G.coo_to_diagonals(s, row, col, data)
        assert np.array_equal(diag, G.coo_to_diagonals(s, *cap["asm"][1][:3])), "u and v share one momentum matrix"
        out.update({
            f"{tag}_u0": u0, f"{tag}_v0": v0, f"{tag}_p0": p0, f"{tag}_mdot0": m0,
            f"{tag}_grad_p": np.concatenate([a.grad_p[:, 0], a.grad_p[:, 1]]),
            f"{tag}_diag": diag.ravel(), f"{tag}_b": np.concatenate([bu, cap["asm"][1][3]]),
            f"{tag}_u_star": cap["solve"][0][1], f"{tag}_v_star": cap["solve"][1][1],
            f"{tag}_mdot_star": faces_to_structured(s, a.mdot_star), f"{tag}_rhs_p": cap["solve"][2][0],
            f"{tag}_p_prime": cap["solve"][2][1], f"{tag}_u_prime": a.u_prime.copy(), f"{tag}_v_prime": a.v_prime.copy(),
            f"{tag}_mdot": faces_to_structured(s, a.mdot), f"{tag}_u": a.u.copy(), f"{tag}_v": a.v.copy(),
            f"{tag}_p": a.p.copy()})
        meta[tag] = dict(kind="step", nx=nx, ny=ny, Re=Re, lid="none", beta=beta, mu=s.mu, **G.PARAMS, **kw)
        print(tag, "one step")


def run(out, meta, nx, ny, Re, K, lid, beta, **kw):
    _, s = make_fv(nx, ny, Re, beta, lid=lid, **kw)
    tag = f"nx{nx}_ny{ny}_Re{Re}_{lid}_K{K}"
    a = s.arrays
    u_prev, v_prev = a.u.copy(), a.v.copy()
    rows = []
    for _ in range(K):
        a.u, a.v, a.p = s.step()
        ru = np.linalg.norm(a.u - u_prev) / (np.linalg.norm(u_prev) + 1e-12)
        rv = np.linalg.norm(a.v - v_prev) / (np.linalg.norm(v_prev) + 1e-12)
        res = s._compute_algebraic_residuals()
        rows.append([max(ru, rv), res["u_residual"], res["v_residual"], res["continuity_residual"]])
        u_prev, v_prev = a.u.copy(), a.v.copy()
    out.update({f"{tag}_rec": np.array(rows), f"{tag}_u": a.u.copy(), f"{tag}_v": a.v.copy(),
                f"{tag}_p": a.p.copy(), f"{tag}_mdot": faces_to_structured(s, a.mdot)})
    meta[tag] = dict(kind="traj", nx=nx, ny=ny, Re=float(Re), K=K, lid=lid, beta=beta, mu=s.mu, **G.PARAMS, **kw)
    print(tag, "rel", rows[-1][0])


def main():
    out, meta = {}, {}
    step_group(out, meta, 17, (("13x17", 13, 17, 100.0, 1.5, {}),("37x50", 37, 50, 400.0, 1.0, WIDE)))
    for lid in ("none", "saad"):
        run(out, meta, 16, 16, 100, 40, lid, 1.5)
    run(out, meta, 13, 17, 100, 40, "none", 1.5)
    run(out, meta, 8, 67, 100, 30, "none", 1.0)
    run(out, meta, 37, 50, 400, 25, "smoothing", 1.0, **WIDE)
    np.savez_compressed(OUT / "g17_fv_stretched.npz", **out)
    (OUT / "g17_fv_stretched.json").write_text(json.dumps(meta, indent=1))


if __name__ == "__main__":
    main()
