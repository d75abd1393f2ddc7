"""Finite-volume solver on the GPU (include/ldc_fv.h): one iteration's intermediates and trajectories against the
reference's fixtures (g14), the TVD path against the NumPy restatement, batches against lone runs, a converged field
against the reference's stored solution, and the launcher end to end."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"
sys.path.insert(0, str(Path(__file__).resolve().parent))
from fv_numpy import FVState  # noqa: E402

from conftest import PKG  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fv():
    import __graft_entry__ as g
    g.build()
    from solvers.fv.solver import FVSolver
    return FVSolver


def _make(FVSolver, m, **kw):
    args = dict(name="fv", Re=m["Re"], nx=m["nx"], ny=m["ny"], corner_treatment=m.get("lid", "none"),
                alpha_uv=m["alpha_uv"], alpha_p=m["alpha_p"], linear_solver_tol=m["linear_solver_tol"],
                convection_scheme=m["convection_scheme"], tolerance=1e-30, max_iterations=10**6, check_every=256)
    args.update(kw)
    return FVSolver(**args)


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


@pytest.mark.parametrize("tag", ["N16", "12x20"])
def test_step_debug_matches_reference_intermediates(fv, tag):
    g = np.load(GOLD / "g14_fv_step.npz")
    m = json.loads((GOLD / "g14_fv_step.json").read_text())[tag]
    s = _make(fv, m)
    s.set_state(g[f"{tag}_u0"], g[f"{tag}_v0"], g[f"{tag}_p0"], g[f"{tag}_mdot0"])
    out = s.step_debug()
    for k, v in out.items():
        assert np.all(np.isfinite(v)), k
        bound = 1e-8 if k == "p_prime" else 1e-10
        assert _rel(v, g[f"{tag}_{k}"]) <= bound, (k, _rel(v, g[f"{tag}_{k}"]))
    st = s.state()
    for k in ("u", "v", "p"):
        assert _rel(st[k], g[f"{tag}_{k}"]) <= 1e-10, k
    s.close()


def test_upwind_trajectories_match_reference(fv):
    g = np.load(GOLD / "g14_fv_traj.npz")
    for tag, m in json.loads((GOLD / "g14_fv_traj.json").read_text()).items():
        s = _make(fv, m, max_iterations=m["K"])
        s.solve()
        ref = g[f"{tag}_rec"]
        assert s.history.shape == ref.shape
        assert np.max(np.abs(s.history[:, :7] - ref[:, :7]) / np.abs(ref[:, :7])) <= 1e-8, tag
        st = s.state()
        for k in ("u", "v", "p", "mdot"):
            assert _rel(st[k], g[f"{tag}_{k}"]) <= 1e-8, (tag, k)
        s.close()


@pytest.mark.parametrize("nx,ny,Re,lid,K", [(16, 16, 100.0, "none", 60), (32, 24, 400.0, "saad", 80),
                                            (48, 48, 1000.0, "none", 40)])
def test_tvd_trajectories_match_restatement(fv, nx, ny, Re, lid, K):
    m = dict(nx=nx, ny=ny, Re=Re, lid=lid, alpha_uv=0.4, alpha_p=0.2, linear_solver_tol=1e-12,
             convection_scheme="TVD")
    s = _make(fv, m, max_iterations=K)
    s.solve()
    o = FVState(nx, ny, Re, corner_treatment=lid, linear_solver_tol=1e-12, convection_scheme="TVD")
    rec = o.run(K)
    assert np.max(np.abs(s.history[:, :7] - rec[:, :7]) / np.abs(rec[:, :7])) <= 1e-9
    st = s.state()
    for k, ref in (("u", o.u), ("v", o.v), ("p", o.p)):
        assert _rel(st[k], ref.ravel()) <= 1e-9, k
    s.close()


def test_batch_is_bit_equal_to_lone_runs(fv):
    import torch
    from solvers.fv import ldc_fv_lib as F
    cases = [dict(Re=100.0), dict(Re=400.0, corner_treatment="saad"), dict(Re=1000.0)]
    base = dict(name="fv", nx=24, ny=24, convection_scheme="TVD", alpha_uv=0.4, alpha_p=0.2, linear_solver_tol=1e-9,
                tolerance=1e-30, check_every=64)
    lone = []
    for c in cases:
        s = fv(**base, **c)
        s._begin(1e-30)
        rows, _, _ = s._advance(64)
        lone.append((rows, s.state()))
        s.close()
    batch = [fv(**base, **c) for c in cases]
    for s in batch:
        s._begin(1e-30)
    F.batch_enqueue([s.handle for s in batch], 64, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for s, (rows, st) in zip(batch, lone):
        assert np.array_equal(s.t["rec"][:64].cpu().numpy(), rows)
        for k in ("u", "v", "p", "mdot"):
            assert np.array_equal(s.state()[k], st[k]), k
        assert s.counters()["iterations"] == 64
        s.close()


def test_converged_N128_Re100_reaches_the_reference_field(fv):
    """TVD to tolerance 1e-6 at N = 128 against data/validation/fv/Re100 (the reference's own converged field): the
    restatement reaches 3.6e-7 / 3.4e-7 relative L2 (profiles/fv_q1_table.md)."""
    s = fv(name="fv", Re=100.0, nx=128, ny=128, convection_scheme="TVD", alpha_uv=0.4, alpha_p=0.2,
           linear_solver_tol=1e-9, tolerance=1e-6, max_iterations=40000)
    s.solve()
    assert s.metrics.converged
    err = s.compute_validation_errors()
    assert err["u_L2_error"] < 2e-6 and err["v_L2_error"] < 2e-6, err
    c = s.counters()
    assert c["linear_giveups"] == 0 and c["nan"] == 0
    s.close()


def test_main_runs_solver_fv(tmp_path):
    r = subprocess.run([sys.executable, str(PKG / "main.py"), "solver=fv", "N=32", "Re=100"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    res = list(tmp_path.rglob("results.json"))
    assert res, r.stderr[-3000:]
    rec = json.loads(res[0].read_text())
    assert rec["solver"] == "fv" and rec["metrics"]["converged"] == 1
    assert "u_L2_error" in rec["validation_errors"] and "u_rel" in rec["ghia"]
    assert rec["metrics"]["psi_min"] < 0 and rec["metrics"]["iterations"] > 10
