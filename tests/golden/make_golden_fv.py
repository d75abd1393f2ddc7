#!/usr/bin/env python3
"""Generate the g14 and g15 fixtures of the finite-volume (SIMPLE) solver by running the *reference* FV solver.

TEST INFRASTRUCTURE, like make_golden.py: the reference is imported read-only, by path, and only the numbers it
produces are written (``g14_fv_*`` / ``g15_fv_*`` ``.npz`` / ``.json`` next to this file).  Stand-ins registered before the import:

* ``numba``: ``njit`` / ``jitclass`` are identities, ``prange`` is ``range``, ``numba.types`` accepts any spec;
* ``pyamg``: ``smoothed_aggregation_solver(A).aspreconditioner()`` becomes an exact sparse LU solve (SciPy
  ``splu``), so the pressure-correction BiCGSTAB lands on the same solution to well below its 1e-9 tolerance;
* ``mlflow`` / ``pyvista`` placeholders and an empty ``solvers`` package, as in make_golden.py.

Every case uses ``convection_scheme="Upwind"``: the reference's TVD branch reads ``psi`` before assignment when
``mdot >= 0`` (DESIGN.md FV-Q1), which plain Python refuses.  The TVD path is pinned by the stored converged fields
under data/validation/fv instead.

Layouts of the stored arrays (the product's own, include/ldc_fv.h): cells ``c = j*nx + i``; face fluxes as two blocks,
``fx[j][i]`` (i = 0..nx, flux in +x through the face at x_i) then ``fy[j][i]`` (j = 0..ny, flux in +y); the momentum
matrix as five diagonals ``aP, aW, aE, aS, aN`` (aP unrelaxed).

Usage:  python tests/golden/make_golden_fv.py [--only g14|g15]
"""
from __future__ import annotations

import importlib
import json
import sys
import types
from pathlib import Path

import numpy as np

REF = Path("/root/reference")
OUT = Path(__file__).resolve().parent

LINEAR_TOL = 1e-12          # tighter than the YAML's 1e-9: the fixtures pin the discretisation, not a stopping point
PARAMS = dict(alpha_uv=0.4, alpha_p=0.2, linear_solver_tol=LINEAR_TOL, convection_scheme="Upwind", limiter="MUSCL")


def _install_shims():
    class _Spec:
        def __getattr__(self, name):
            return self

        def __getitem__(self, item):
            return self

        def __call__(self, *a, **k):
            return self

    nb = types.ModuleType("numba")

    def njit(*args, **kwargs):
        if len(args) == 1 and callable(args[0]) and not kwargs:
            return args[0]
        return lambda f: f

    nb.njit = nb.jit = njit
    nb.prange = range
    nb.types = _Spec()
    exp = types.ModuleType("numba.experimental")
    exp.jitclass = lambda *a, **k: (lambda cls: cls)
    nb.experimental = exp
    sys.modules["numba"] = nb
    sys.modules["numba.experimental"] = exp

    amg = types.ModuleType("pyamg")

    def smoothed_aggregation_solver(A, **kw):
        from scipy.sparse.linalg import LinearOperator, splu
        lu = splu(A.tocsc())
        return types.SimpleNamespace(aspreconditioner=lambda: LinearOperator(A.shape, matvec=lu.solve))

    amg.smoothed_aggregation_solver = smoothed_aggregation_solver
    sys.modules["pyamg"] = amg

    ml = types.ModuleType("mlflow")
    ml.active_run = lambda: None
    ml.log_metrics = lambda *a, **k: None
    sys.modules["mlflow"] = ml
    pv = types.ModuleType("pyvista")
    pv.StructuredGrid = type("StructuredGrid", (), {})
    sys.modules["pyvista"] = pv

    for p in (str(REF / "src"),):
        if p not in sys.path:
            sys.path.insert(0, p)
    pkg = types.ModuleType("solvers")
    pkg.__path__ = [str(REF / "src" / "solvers")]
    sys.modules["solvers"] = pkg


def ref_solver_module():
    _install_shims()
    return importlib.import_module("solvers.fv.solver")


def make_fv(nx, ny, Re, lid="none", **kw):
    mod = ref_solver_module()
    args = dict(name="fv", Re=float(Re), nx=nx, ny=ny, tolerance=1e-6, max_iterations=10_000_000,
                corner_treatment=lid, **PARAMS)
    args.update(kw)
    return mod, mod.FVSolver(**args)


# --------------------------------------------------------------------------- layout converters
def faces_to_structured(s, mdot):
    """Reference face array -> [fx (ny, nx+1) | fy (ny+1, nx)] fluxes in +x / +y."""
    m = s.mesh
    nx, ny = s.params.nx, s.params.ny
    dx, dy = s.params.Lx / nx, s.params.Ly / ny
    fx, fy = np.full((ny, nx + 1), np.nan), np.full((ny + 1, nx), np.nan)
    for f in range(mdot.shape[0]):
        S = m.vector_S_f[f]
        fc = m.face_centers[f]
        if abs(S[0]) > abs(S[1]):
            i, j = int(round(fc[0] / dx)), int(np.floor(fc[1] / dy))
            fx[j, i] = mdot[f] * np.sign(S[0])
        else:
            i, j = int(np.floor(fc[0] / dx)), int(round(fc[1] / dy))
            fy[j, i] = mdot[f] * np.sign(S[1])
    assert not np.isnan(fx).any() and not np.isnan(fy).any()
    return np.concatenate([fx.ravel(), fy.ravel()])


def coo_to_diagonals(s, row, col, data):
    from scipy.sparse import csr_matrix
    nx, ny = s.params.nx, s.params.ny
    n = nx * ny
    A = csr_matrix((data, (row, col)), shape=(n, n)).toarray()
    c = np.arange(n)
    i, j = c % nx, c // nx
    out = np.zeros((5, n))
    out[0] = A[c, c]
    out[1, i > 0] = A[c[i > 0], c[i > 0] - 1]
    out[2, i < nx - 1] = A[c[i < nx - 1], c[i < nx - 1] + 1]
    out[3, j > 0] = A[c[j > 0], c[j > 0] - nx]
    out[4, j < ny - 1] = A[c[j < ny - 1], c[j < ny - 1] + nx]
    keep = np.zeros_like(A)
    keep[c, c] = 1
    keep[c[i > 0], c[i > 0] - 1] = keep[c[i < nx - 1], c[i < nx - 1] + 1] = 1
    keep[c[j > 0], c[j > 0] - nx] = keep[c[j < ny - 1], c[j < ny - 1] + nx] = 1
    assert np.all(A[keep == 0] == 0), "momentum matrix is not five-diagonal"
    return out


def record_row(s, u_prev, v_prev):
    """One row of the reference's solve loop (base.py:250-276): rel, |u'|, |v'|, |div mdot|, E, Z, P, DT = 0."""
    a = s.arrays
    ru = np.linalg.norm(a.u - u_prev) / (np.linalg.norm(u_prev) + 1e-12)
    rv = np.linalg.norm(a.v - v_prev) / (np.linalg.norm(v_prev) + 1e-12)
    res = s._compute_algebraic_residuals()
    return [max(ru, rv), res["u_residual"], res["v_residual"], res["continuity_residual"],
            s._compute_energy(), s._compute_enstrophy(), s._compute_palinstrophy(), 0.0]


def seed_state(s, rng):
    """A smooth random state: u, v, p as low-order sine series, mdot from interpolated velocities (walls included)."""
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


# --------------------------------------------------------------------------- groups
def g14_step():
    """One iteration's intermediates at N = 16 (and 12 x 20) from a seeded smooth state."""
    _step_group("g14_fv_step", 14, (("N16", 16, 16, 100.0, {}), ("12x20", 12, 20, 400.0, {})))


def _step_group(name, seed, cases):
    out, meta = {}, {}
    for tag, nx, ny, Re, kw in cases:
        mod, s = make_fv(nx, ny, Re, **kw)
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
        diag = coo_to_diagonals(s, row, col, data)
        diag_v = coo_to_diagonals(s, *cap["asm"][1][:3])
        assert np.array_equal(diag, diag_v), "u and v share one momentum matrix"
        out.update({
            f"{tag}_u0": u0, f"{tag}_v0": v0, f"{tag}_p0": p0, f"{tag}_mdot0": m0,
            f"{tag}_grad_p": np.concatenate([a.grad_p[:, 0], a.grad_p[:, 1]]),
            f"{tag}_diag": diag.ravel(), f"{tag}_b": np.concatenate([bu, cap["asm"][1][3]]),
            f"{tag}_u_star": cap["solve"][0][1], f"{tag}_v_star": cap["solve"][1][1],
            f"{tag}_mdot_star": faces_to_structured(s, a.mdot_star), f"{tag}_rhs_p": cap["solve"][2][0],
            f"{tag}_p_prime": cap["solve"][2][1], f"{tag}_u_prime": a.u_prime.copy(), f"{tag}_v_prime": a.v_prime.copy(),
            f"{tag}_mdot": faces_to_structured(s, a.mdot), f"{tag}_u": a.u.copy(), f"{tag}_v": a.v.copy(),
            f"{tag}_p": a.p.copy()})
        meta[tag] = dict(nx=nx, ny=ny, Re=Re, lid="none", mu=s.mu, **PARAMS, **kw)
    np.savez_compressed(OUT / f"{name}.npz", **out)
    (OUT / f"{name}.json").write_text(json.dumps(meta, indent=1))


def g14_trajectories():
    """Trajectories from rest with their record rows; lids none and saad; one nx != ny case."""
    cases = [(16, 16, 100, 50), (32, 32, 400, 100), (48, 48, 1000, 40)]
    out, meta = {}, {}
    for nx, ny, Re, K in cases:
        for lid in ("none", "saad"):
            _run(out, meta, nx, ny, Re, K, lid)
    _run(out, meta, 24, 16, 100, 30, "none")
    np.savez_compressed(OUT / "g14_fv_traj.npz", **out)
    (OUT / "g14_fv_traj.json").write_text(json.dumps(meta, indent=1))


def _run(out, meta, nx, ny, Re, K, lid, **kw):
    _, s = make_fv(nx, ny, Re, lid=lid, **kw)
    tag = f"nx{nx}_ny{ny}_Re{Re}_{lid}_K{K}"
    a = s.arrays
    u_prev, v_prev = a.u.copy(), a.v.copy()
    rows = []
    for _ in range(K):
        a.u, a.v, a.p = s.step()
        rows.append(record_row(s, u_prev, v_prev))
        u_prev, v_prev = a.u.copy(), a.v.copy()
    out.update({f"{tag}_rec": np.array(rows), f"{tag}_u": a.u.copy(), f"{tag}_v": a.v.copy(),
                f"{tag}_p": a.p.copy(), f"{tag}_mdot": faces_to_structured(s, a.mdot)})
    meta[tag] = dict(nx=nx, ny=ny, Re=float(Re), K=K, lid=lid, mu=s.mu, **PARAMS, **kw)
    print(tag, "rel", rows[-1][0])


# --------------------------------------------------------------------------- g15: odd sizes, Lx != Ly, lid != 1
WIDE = dict(Lx=2.0, Ly=0.5, lid_velocity=2.0)       # the 37 x 50 cases


def g15_step():
    """One iteration's intermediates at 13 x 17 and at 37 x 50 cells (1850: more than three strides of the kernel's
    512 threads) on a 2 x 0.5 cavity with lid speed 2."""
    _step_group("g15_fv_step", 15, (("13x17", 13, 17, 100.0, {}), ("37x50", 37, 50, 400.0, WIDE)))


def g15_trajectories():
    """Trajectories from rest at sizes that are no multiple of 4 (nor of the 16 x 16 tile), a thin rectangle, and the
    wide cavity with the smoothed lid."""
    out, meta = {}, {}
    _run(out, meta, 13, 17, 100, 40, "none")
    _run(out, meta, 9, 30, 400, 30, "none")
    _run(out, meta, 8, 67, 100, 30, "none")
    _run(out, meta, 37, 50, 400, 25, "smoothing", **WIDE)
    np.savez_compressed(OUT / "g15_fv_traj.npz", **out)
    (OUT / "g15_fv_traj.json").write_text(json.dumps(meta, indent=1))


def g15_converged(nx=13, ny=17, Re=100.0, tolerance=1e-4, margin=1e-4):
    """The reference's own solve() to its stopping rule: iteration count, metrics, time series and final fields.

    The count is only a fair demand on another implementation if rounding cannot move it: rel at the stopping
    iteration and at the one before must each be ``margin`` (relative) away from the tolerance."""
    _, s = make_fv(nx, ny, Re, tolerance=tolerance, max_iterations=5000)
    s.solve()
    m = {k: (v.item() if isinstance(v, np.generic) else v) for k, v in s.metrics.__dict__.items()}
    m["wall_time_seconds"] = float(m["wall_time_seconds"])
    ts = {k: list(map(float, v)) if v else [] for k, v in s.time_series.__dict__.items()}
    rel = ts["rel_iter_residual"]
    assert m["converged"] and len(rel) == m["iterations"] - 10, "every recorded iteration kept (no downsampling)"
    margins = dict(at_stop=(tolerance - rel[-1]) / tolerance, before_stop=(rel[-2] - tolerance) / tolerance)
    assert margins["at_stop"] >= margin and margins["before_stop"] >= margin, margins
    a = s.arrays
    meta = dict(nx=nx, ny=ny, Re=Re, lid="none", tolerance=tolerance, mu=s.mu, **PARAMS, metrics=m, margins=margins,
                time_series_len={k: len(v) for k, v in ts.items()})
    (OUT / "g15_fv_converged.json").write_text(json.dumps(meta, indent=1))
    np.savez_compressed(OUT / "g15_fv_converged.npz", u=s.fields.u, v=s.fields.v, p=s.fields.p,
                        mdot=faces_to_structured(s, a.mdot), **{f"ts_{k}": np.array(v) for k, v in ts.items()})
    print("converged", nx, ny, Re, "iterations", m["iterations"], "margins", margins)


def g15_lid_profiles(nx=13, ny=8, Lx=2.0, lid_velocity=2.0):
    """u on the lid faces, as the reference's mesh builder sets it, west to east."""
    _install_shims()
    from shared.meshing.simple_structured import create_structured_mesh_2d
    out = {}
    for lid in ("none", "saad", "smoothing"):
        m = create_structured_mesh_2d(nx=nx, ny=ny, Lx=Lx, Ly=1.0, lid_velocity=lid_velocity, corner_treatment=lid,
                                      corner_smoothing=0.15)
        top = [f for f in m.boundary_faces if abs(m.face_centers[f][1] - 1.0) < 1e-10]
        top.sort(key=lambda f: m.face_centers[f][0])
        assert len(top) == nx
        out[lid] = np.array([m.boundary_values[f][0] for f in top])
    np.savez_compressed(OUT / "g15_fv_lid.npz", **out)
    meta = dict(nx=nx, Lx=Lx, lid_velocity=lid_velocity, corner_smoothing=0.15)
    (OUT / "g15_fv_lid.json").write_text(json.dumps(meta, indent=1))


GROUPS = {"g14": (g14_step, g14_trajectories), "g15": (g15_step, g15_trajectories, g15_converged, g15_lid_profiles)}

if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=sorted(GROUPS), help="one group (default: all)")
    for name in ([ap.parse_args().only] if ap.parse_args().only else sorted(GROUPS)):
        for fn in GROUPS[name]:
            fn()
