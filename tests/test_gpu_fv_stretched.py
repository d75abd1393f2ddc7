"""Wall-clustered (tanh) grids of one-CU finite-volume trials (grid="tanh", ldc_fv_set_grid, csrc/ldc_fv_stretched.hip) on the
GPU: Upwind trajectories against the reference's own code on such a mesh (g17), TVD trajectories of both pressure equations
against the NumPy restatement (tests/fv_stretched_numpy.py), grid_stretch = 0 against the uniform kernels, bit equality in
mixed batches and across repeats, a solve to the latch with its centreline extrema against Botella & Peyret, and the launcher."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"
sys.path.insert(0, str(Path(__file__).resolve().parent))
from fv_stretched_numpy import BOTELLA_RE1000, FVStretchedState, centreline_extrema, tanh_vertices  # noqa: E402

from conftest import PKG  # noqa: E402

pytestmark = pytest.mark.gpu

FIELDS = ("u", "v", "p", "mdot")
MODES = {"reference": "reference", "consistent_cu": "consistent"}        # the solver's name -> the restatement's


@pytest.fixture(scope="module")
def fv():
    import __graft_entry__ as g
    g.build()
    from solvers.fv.batched import BatchedFVSolver
    from solvers.fv.solver import FVSolver
    return FVSolver, BatchedFVSolver


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def _rows_rel(got, ref):
    den = np.where(ref == 0.0, 1.0, np.abs(ref))
    return float(np.max(np.abs(got - ref) / den))


def _mdot(o):
    return np.concatenate([o.fx.ravel(), o.fy.ravel()])


# ------------------------------------------------------------------------------------------- the reference's own code
def test_upwind_trajectories_match_the_reference_on_the_stretched_mesh(fv):
    """All five g17 trajectories, pressure_equation="reference": u, v, p, mdot and record columns 0 - 3 to 1e-8, as
    tests/test_gpu_fv.py asks against g14."""
    FVSolver, _ = fv
    g = np.load(GOLD / "g17_fv_stretched.npz")
    meta = json.loads((GOLD / "g17_fv_stretched.json").read_text())
    trajs = {t: m for t, m in meta.items() if m["kind"] == "traj"}
    assert len(trajs) == 5
    for tag, m in trajs.items():
        s = FVSolver(name="fv", Re=m["Re"], nx=m["nx"], ny=m["ny"], Lx=m.get("Lx", 1.0), Ly=m.get("Ly", 1.0),
                     lid_velocity=m.get("lid_velocity", 1.0), corner_treatment=m["lid"], alpha_uv=m["alpha_uv"],
                     alpha_p=m["alpha_p"], linear_solver_tol=m["linear_solver_tol"], convection_scheme=m["convection_scheme"],
                     grid="tanh", grid_stretch=m["beta"], tolerance=1e-30, max_iterations=m["K"], check_every=256)
        s.solve()
        ref = g[f"{tag}_rec"]
        st = s.state()
        devs = {k: _rel(st[k], g[f"{tag}_{k}"]) for k in FIELDS}
        rows = float(np.max(np.abs(s.history[:, :4] - ref) / np.abs(ref)))
        print(f"{tag}: records {rows:.2e}, fields {devs}")
        assert s.history.shape == (m["K"], 8)
        assert rows <= 1e-8, tag
        for k, d in devs.items():
            assert d <= 1e-8, (tag, k)
        xs = np.unique(s.fields.x)
        assert np.allclose(xs, 0.5 * (tanh_vertices(m["nx"], m.get("Lx", 1.0), m["beta"])[1:]
                                      + tanh_vertices(m["nx"], m.get("Lx", 1.0), m["beta"])[:-1]), rtol=1e-14)
        s.close()


# ------------------------------------------------------------------------------------------- TVD against the restatement
@pytest.mark.parametrize("mode", ["consistent_cu", "reference"])
@pytest.mark.parametrize("nx,ny,beta", [(16, 16, 1.5), (24, 16, 1.0)])
def test_tvd_trajectories_match_the_restatement(fv, nx, ny, beta, mode):
    """30 TVD iterations from rest, both pressure equations, every record column (E, Z, P by the Gauss rule) to 1e-9.
    |div mdot| (column 3) of the consistent equation is zero to the CG tolerance in both runs and has no digits to compare:
    it is held against the size of the fluxes instead."""
    FVSolver, _ = fv
    K = 30
    s = FVSolver(name="fv", Re=100.0, nx=nx, ny=ny, convection_scheme="TVD", alpha_uv=0.4, alpha_p=0.2,
                 linear_solver_tol=1e-12, grid="tanh", grid_stretch=beta, pressure_equation=mode, pressure_tol=1e-12,
                 tolerance=1e-30, max_iterations=K, check_every=8)
    s.solve()
    o = FVStretchedState(nx, ny, 100.0, linear_solver_tol=1e-12, convection_scheme="TVD", grid_stretch=beta,
                         pressure_equation=MODES[mode], pressure_solver="direct")
    rec = o.run(K)
    st = s.state()
    devs = {k: _rel(st[k], ref) for k, ref in (("u", o.u.ravel()), ("v", o.v.ravel()), ("p", o.p.ravel()), ("mdot", _mdot(o)))}
    cols = [0, 1, 2, 4, 5, 6] if mode == "consistent_cu" else list(range(7))
    print(f"{nx}x{ny} beta {beta} {mode}: records {_rows_rel(s.history[:, cols], rec[:, cols]):.2e}, "
          f"div {np.max(np.abs(s.history[:, 3] - rec[:, 3])):.2e}, fields {devs}, {s.counters()}")
    assert s.history.shape == rec.shape
    assert _rows_rel(s.history[:, cols], rec[:, cols]) <= 1e-9
    assert np.max(np.abs(s.history[:, 3] - rec[:, 3])) <= 1e-9 * np.max(np.abs(_mdot(o)))
    for k, d in devs.items():
        assert d <= 1e-9, k
    if mode == "consistent_cu":
        c = s.counters()
        assert c["pressure_caps"] == 0 and c["pressure_solves"] == K
        m = st["mdot"]
        fx, fy = m[: ny * (nx + 1)].reshape(ny, nx + 1), m[ny * (nx + 1):].reshape(ny + 1, nx)
        assert not fx[:, 0].any() and not fx[:, -1].any() and not fy[0].any() and not fy[-1].any()      # walls: exactly 0.0
    s.close()


# ------------------------------------------------------------------------------------------- beta = 0: the uniform kernels
@pytest.mark.parametrize("mode", ["reference", "consistent_cu"])
@pytest.mark.parametrize("nx,ny", [(16, 16), (13, 17)])
def test_zero_stretch_follows_the_uniform_kernel(fv, nx, ny, mode):
    """grid="tanh", grid_stretch=0 (uniform vertices through the new kernel) against the uniform kernel of the same mode, 20
    TVD iterations: fields and every record column to 1e-9 (the constant lid: the Gauss rule is the ghost-cell rule)."""
    FVSolver, _ = fv
    kw = dict(name="fv", Re=100.0, nx=nx, ny=ny, convection_scheme="TVD", alpha_uv=0.4, alpha_p=0.2, linear_solver_tol=1e-12,
              pressure_equation=mode, pressure_tol=1e-12, tolerance=1e-30, max_iterations=20, check_every=8)
    a = FVSolver(**kw, grid="tanh", grid_stretch=0.0)
    a.solve()
    b = FVSolver(**kw)
    b.solve()
    sa, sb = a.state(), b.state()
    devs = {k: _rel(sa[k], sb[k]) for k in FIELDS}
    cols = [0, 1, 2, 4, 5, 6] if mode == "consistent_cu" else list(range(7))
    print(f"{nx}x{ny} {mode}: records {_rows_rel(a.history[:, cols], b.history[:, cols]):.2e}, fields {devs}")
    assert _rows_rel(a.history[:, cols], b.history[:, cols]) <= 1e-9
    assert np.max(np.abs(a.history[:, 3] - b.history[:, 3])) <= 1e-9 * np.max(np.abs(sb["mdot"]))
    for k, d in devs.items():
        assert d <= 1e-9, k
    assert _rel(a.fields.x, b.fields.x) <= 1e-15 and _rel(a.fields.y, b.fields.y) <= 1e-15
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------- bit equality
BATCH = [dict(nx=13, ny=17, grid="tanh", grid_stretch=1.5, pressure_equation="consistent_cu"),
         dict(nx=32, ny=32, grid="tanh", grid_stretch=1.5, pressure_equation="consistent_cu", Re=400.0),
         dict(nx=16, ny=16, pressure_equation="consistent_cu"),
         dict(nx=16, ny=16, grid="tanh", grid_stretch=1.0, pressure_equation="reference", corner_treatment="saad"),
         dict(nx=16, ny=16)]
BASE = dict(name="fv", Re=100.0, convection_scheme="TVD", alpha_uv=0.4, alpha_p=0.2, linear_solver_tol=1e-9, tolerance=1e-30,
            check_every=32)


def _lone(FVSolver, kw, chunks=(24,)):
    s = FVSolver(**dict(BASE, **kw))
    s._begin(1e-30)
    rows = np.concatenate([s._advance(k)[0] for k in chunks], axis=0)
    out = (rows, s.state(), s.counters())
    s.close()
    return out


def test_a_mixed_batch_is_bit_equal_to_the_lone_runs(fv):
    """One ldc_fv_batch_enqueue over a stretched 13 x 17, a stretched 32 x 32, a uniform 16 x 16 (all consistent), a stretched
    16 x 16 in the other pressure mode and a uniform reference trial: four launch groups.  Every trial is bit-equal to its lone
    run; the uniform ones run the kernels they ran before (their code objects are unchanged: profiles/fv_stretched.md)."""
    import torch
    from solvers.fv import ldc_fv_lib as F
    FVSolver, _ = fv
    lone = [_lone(FVSolver, kw) for kw in BATCH]
    batch = [FVSolver(**dict(BASE, **kw)) for kw in BATCH]
    for s in batch:
        s._begin(1e-30)
    F.batch_enqueue([s.handle for s in batch], 24, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for s, (rows, st, c) in zip(batch, lone):
        assert np.array_equal(s.t["rec"][:24].cpu().numpy(), rows)
        got = s.state()
        for k in FIELDS:
            assert np.array_equal(got[k], st[k]), k
        assert s.counters() == c and c["iterations"] == 24 and c["nan"] == 0
        s.close()


def test_the_batched_solver_takes_stretched_trials(fv):
    """BatchedFVSolver over the same mix, to each trial's own cap: histories and fields are those of the lone solves."""
    FVSolver, Batched = fv
    trials = [dict(BASE, **kw, max_iterations=20 + 3 * q) for q, kw in enumerate(BATCH[:4])]
    b = Batched(trials)
    b.solve()
    assert not b.errors
    for t, s in zip(trials, b.solvers):
        one = FVSolver(**t)
        one.solve()
        assert np.array_equal(one.history, s.history)
        for k in ("u", "v", "p"):
            assert np.array_equal(getattr(one.fields, k), getattr(s.fields, k)), k
        one.close()
    b.close()


def test_a_repeat_solve_on_one_handle_is_bit_equal(fv):
    """Two solves from the same state on ONE handle, and a third in other chunks: the same bits (fixed summation order, no
    state kept in the kernel between launches)."""
    FVSolver, _ = fv
    for kw in (BATCH[0], BATCH[3]):
        s = FVSolver(**dict(BASE, **kw))
        runs = []
        for chunks in ((24,), (24,), (7, 1, 16)):
            z = np.zeros(s.n_cells)
            s.set_state(z, z, z, np.zeros(s.t["mdot"].numel()))
            s._begin(1e-30)
            rows = np.concatenate([s._advance(k)[0] for k in chunks], axis=0)
            runs.append((rows, s.state(), s.counters()))
        for rows, st, c in runs[1:]:
            assert np.array_equal(rows, runs[0][0]) and c == runs[0][2]
            for k in FIELDS:
                assert np.array_equal(st[k], runs[0][1][k]), k
        s.close()


# ------------------------------------------------------------------------------------------- a solve to the latch
def test_convergence_at_32_re1000_beats_the_uniform_grid(fv):
    """32 x 32, Re 1000, beta 1.5, TVD, consistent_cu, 0.7 / 0.3, tolerance 1e-7 (tools/fv_stretched_converged.py): the
    restatement stops after 1704 iterations with rel 4.6e-4 (before) and 7.7e-4 (at the stop) relative away from the tolerance,
    so rounding cannot move the count.  The three centreline extrema agree with the restatement's to 1e-6, each is strictly
    closer to Botella & Peyret's than in the uniform 32 x 32 run of the same settings, and no pressure solve hits its cap."""
    FVSolver, _ = fv
    want = json.loads((GOLD / "g17_fv_stretched_converged.json").read_text())
    assert want["iterations"] == 1704 and min(want["margins"].values()) >= 1e-4
    kw = dict(name="fv", Re=1000.0, nx=32, ny=32, convection_scheme="TVD", alpha_uv=0.7, alpha_p=0.3, linear_solver_tol=1e-9,
              pressure_equation="consistent_cu", pressure_tol=1e-8, pressure_max_iters=200, tolerance=1e-7,
              max_iterations=5000, check_every=512)
    err = {}
    for name, grid in (("tanh", dict(grid="tanh", grid_stretch=1.5)), ("uniform", {})):
        s = FVSolver(**kw, **grid)
        s.solve()
        c = s.counters()
        assert s.metrics.converged and c["pressure_caps"] == 0 and c["linear_giveups"] == 0 and c["nan"] == 0
        ny, nx = s.shape_full
        xs, ys = s.fields.x.reshape(ny, nx)[0], s.fields.y.reshape(ny, nx)[:, 0]
        ext = centreline_extrema(s.fields.u.reshape(ny, nx), s.fields.v.reshape(ny, nx), xs, ys)
        err[name] = {k: abs(abs(ext[k]) - abs(BOTELLA_RE1000[k])) for k in ext}
        print(name, int(s.metrics.iterations), ext, err[name], c)
        if name == "tanh":
            assert int(s.metrics.iterations) == want["iterations"]
            for k in ext:
                assert abs(ext[k] - want["extrema"][k]) <= 1e-6, k
            assert c["pressure_iterations"] / c["pressure_solves"] == pytest.approx(want["cg_iterations_mean"], abs=1.0)
            m = s.compute_vortex_metrics()                   # the host route with the stretched psi and omega
            assert -0.13 < m["psi_min"] < -0.09 and 0.4 < m["psi_min_x"] < 0.65 and 0.45 < m["psi_min_y"] < 0.7
            assert s.streamfunction().shape == (32, 32) and np.all(s.streamfunction()[0] == 0.0)
        s.close()
    for k in err["tanh"]:
        assert err["tanh"][k] < err["uniform"][k], k


# ------------------------------------------------------------------------------------------- the launcher
def test_main_runs_a_stretched_trial(tmp_path):
    r = subprocess.run([sys.executable, str(PKG / "main.py"), "solver=fv", "N=16", "+solver.grid=tanh",
                        "+solver.pressure_equation=consistent_cu"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    res = list(tmp_path.rglob("results.json"))
    assert res, r.stderr[-3000:]
    rec = json.loads(res[0].read_text())
    assert rec["solver"] == "fv" and rec["metrics"]["converged"] == 1
    assert "u_L2_error" in rec["validation_errors"] and "u_rel" in rec["ghia"] and rec["metrics"]["psi_min"] < 0
    sys.path.insert(0, str(PKG / "src"))
    from solvers.vtkio import read_vts
    vts = list(tmp_path.rglob("solution.vts"))
    assert vts, r.stderr[-3000:]
    pts = read_vts(vts[0])["points"]
    xv = tanh_vertices(16, 1.0, 1.5)                         # the default grid_stretch
    assert np.allclose(np.unique(pts[:, 0]), 0.5 * (xv[1:] + xv[:-1]), rtol=0, atol=1e-12)
    assert np.allclose(np.unique(pts[:, 1]), 0.5 * (xv[1:] + xv[:-1]), rtol=0, atol=1e-12)
