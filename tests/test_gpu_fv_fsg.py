"""Coarse-to-fine sequencing of the finite-volume solver on the GPU (solvers/fv/fsg.py, BatchedFVFSGSolver): the
sequence 16^2 -> 32^2 lone and batched against the same steps done by hand and against the solve from rest, batches of
mixed sizes and depths against lone sequenced solves, continuation in Re, a NaN on a coarse level, and the launcher."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import fv_prolong_numpy as P  # noqa: E402

from conftest import PKG  # noqa: E402

pytestmark = pytest.mark.gpu

YAML = dict(convection_scheme="TVD", alpha_uv=0.4, alpha_p=0.2, linear_solver_tol=1e-9)      # conf/solver/fv.yaml
FLAGSHIP = dict(YAML, nx=32, ny=32, Re=100.0, tolerance=1e-6, max_iterations=20000, check_every=512)
STATE = ("u", "v", "p", "mdot")


@pytest.fixture(scope="module")
def fv():
    import __graft_entry__ as g
    g.build()
    from solvers.fv.batched import BatchedFVFSGSolver
    from solvers.fv.fsg import FVFSGSolver
    from solvers.fv.solver import FVSolver, prolong
    return FVSolver, FVFSGSolver, BatchedFVFSGSolver, prolong


@pytest.fixture(scope="module")
def flagship(fv):
    """The lone sequenced solve 16^2 -> 32^2 (Re = 100, TVD, tolerance 1e-6), shared and left unchanged."""
    s = fv[1](name="fv_fsg", **FLAGSHIP)
    s.solve()
    yield s
    s.close()


def _assert_same_trial(a, b, what):
    assert a.metrics.iterations == b.metrics.iterations and a.metrics.converged == b.metrics.converged, what
    assert a.history.shape == b.history.shape and np.array_equal(a.history, b.history), what
    sa, sb = a.state(), b.state()
    for k in STATE:
        assert np.array_equal(sa[k], sb[k]), (what, k)
    ma, mb = a.metrics.as_dict(), b.metrics.as_dict()
    for k in mb:
        if k != "wall_time_seconds":
            assert np.array_equal(ma[k], mb[k]), (what, k, ma[k], mb[k])


def test_the_sequence_converges_and_counts_its_levels(flagship):
    s = flagship
    print("iterations per level", s.level_iterations, "seconds", s.metrics.wall_time_seconds)
    assert s.level_sizes() == [(16, 16), (32, 32)]
    assert s.metrics.converged and len(s.level_iterations) == 2
    assert s.metrics.iterations == s.level_iterations[1] == len(s.history) > 10
    assert s.level_iterations[0] > 10 and s.metrics.final_residual < 1e-6
    assert s.history[0, 0] < 0.1                  # the fine level starts near its solution (the restatement: 1.5e-2)
    assert np.array_equal(s.fields.u, s.state()["u"]) and s.metrics.psi_min < 0


def test_the_sequence_is_the_same_steps_done_by_hand(fv, flagship):
    FVSolver, _, _, prolong = fv
    coarse = FVSolver(name="fv", **dict(FLAGSHIP, nx=16, ny=16))
    coarse.solve()
    fine = FVSolver(name="fv", **FLAGSHIP)
    prolong([(coarse, fine)])
    fine.solve()
    assert [coarse.metrics.iterations, fine.metrics.iterations] == flagship.level_iterations
    _assert_same_trial(flagship, fine, "by hand")
    coarse.close(), fine.close()


def test_the_sequence_ends_where_the_solve_from_rest_ends(fv, flagship):
    """Both stop on a rate-bound rule, so they end a few 1e-4 apart: the bound is twice what the two runs of the NumPy
    restatement differ by (tests/test_fv_prolong_cpu.py checks those figures), the margin for the device's own rounding
    path to the latch."""
    lone = fv[0](name="fv", **FLAGSHIP)
    lone.solve()
    a, b = flagship.state(), lone.state()
    duv = max(float(np.max(np.abs(a[k] - b[k]))) for k in ("u", "v"))
    dp = float(np.max(np.abs(a["p"] - b["p"])))
    print("iterations: from rest", lone.metrics.iterations, "sequenced", flagship.level_iterations,
          " max |du|, |dv|:", duv, " max |dp|:", dp)
    assert lone.metrics.converged
    assert 0 < duv < 2 * P.SEQ_16_32_DUV and 0 < dp < 2 * P.SEQ_16_32_DP
    lone.close()


def test_a_batch_of_the_sequence_equals_the_lone_one(fv, flagship):
    batch = fv[2]([dict(FLAGSHIP, name="fv_fsg"), dict(FLAGSHIP, name="fv_fsg", vortex_metrics="device")])
    metrics = batch.solve()
    assert batch.errors == {} and all(m is not None and m.converged for m in metrics)
    for s in batch.solvers:
        assert s.level_iterations == flagship.level_iterations and s.metrics.iterations == s.level_iterations[1]
    _assert_same_trial(batch.solvers[0], flagship, "batched")
    for k in STATE:
        assert np.array_equal(batch.solvers[1].state()[k], flagship.state()[k]), k
    assert abs(batch.solvers[1].metrics.psi_min / flagship.metrics.psi_min - 1) < 1e-9      # (device metrics, one launch)
    batch.close()


def test_a_batch_of_mixed_sizes_and_depths_equals_lone_sequences(fv):
    """Three levels, two levels (40 halves once: 20 >= 16, 10 is not) and one level (48 x 20 cannot halve) in ONE batch."""
    _, FVFSGSolver, Batched, _ = fv
    common = dict(YAML, name="fv_fsg", tolerance=1e-5, max_iterations=20000, check_every=256)
    trials = [dict(common, nx=64, ny=64, Re=100.0, n_levels=3),
              dict(common, nx=40, ny=40, Re=400.0, n_levels=3, corner_treatment="saad", coarse_tolerance_factor=10.0),
              dict(common, nx=48, ny=20, Re=100.0)]
    batch = Batched(trials)
    assert [s.level_sizes() for s in batch.solvers] == [[(16, 16), (32, 32), (64, 64)], [(20, 20), (40, 40)], [(48, 20)]]
    batch.solve()
    assert batch.errors == {}
    for q, t in enumerate(trials):
        lone = FVFSGSolver(**t)
        lone.solve()
        print(q, "iterations per level", lone.level_iterations)
        assert lone.metrics.converged and batch.solvers[q].level_iterations == lone.level_iterations
        assert len(lone.level_iterations) == (3, 2, 1)[q]
        _assert_same_trial(batch.solvers[q], lone, q)
        lone.close()
    batch.close()


def test_continuation_in_re_runs_the_fine_level_only(fv):
    FVSolver, FVFSGSolver, _, _ = fv
    common = dict(YAML, nx=32, ny=32, tolerance=1e-5, max_iterations=20000, check_every=256)
    a = FVSolver(name="fv", Re=100.0, **common)
    a.solve()
    b = FVFSGSolver(name="fv_fsg", Re=200.0, **common)
    b.start_from(a)
    st = b.state()
    assert np.array_equal(st["u"], a.state()["u"]) and np.array_equal(st["v"], a.state()["v"])      # the same grid: identity
    assert b.level_sizes() == [(32, 32)]
    b.solve()
    print("Re 100 from rest:", a.metrics.iterations, "iterations; Re 200 from it:", b.level_iterations)
    assert b.metrics.converged and b.level_iterations == [b.metrics.iterations]
    assert b.history[0, 0] < 0.1 and not np.array_equal(b.state()["u"], a.state()["u"])
    assert b.level_sizes() == [(16, 16), (32, 32)]        # the start is used up: the next solve is the whole sequence
    a.close(), b.close()


def test_a_nan_on_a_coarse_level_ends_the_solve(fv):
    """16 x 16, Re 1000 without under-relaxation overflows within about ten iterations (tests/test_gpu_fv_edges.py): here
    that is the COARSE level of a 32 x 32 trial.  Lone: the LdcError of a lone NaN; batched: errors[q], neighbours intact."""
    _, FVFSGSolver, Batched, _ = fv
    from solvers.spectral.ldc_lib import LdcError
    common = dict(YAML, name="fv_fsg", nx=32, ny=32, tolerance=1e-5, max_iterations=2000, check_every=256)
    bad = dict(common, Re=1000.0, alpha_uv=1.0, alpha_p=1.0)
    s = FVFSGSolver(**bad)
    with pytest.raises(LdcError, match="NaN"):
        s.solve()
    assert s.level_iterations == [] and s.metrics.iterations == 0
    s.close()
    good = dict(common, Re=100.0)
    batch = Batched([good, bad, dict(good, nx=24, ny=24)])
    metrics = batch.solve()
    assert list(batch.errors) == [1] and isinstance(batch.errors[1], LdcError) and "NaN" in str(batch.errors[1])
    assert metrics[1] is None and len(batch.solvers[1].level_iterations) == 1
    lone = FVFSGSolver(**good)
    lone.solve()
    _assert_same_trial(batch.solvers[0], lone, "neighbour of the NaN trial")
    assert batch.solvers[2].metrics.converged and batch.solvers[2].level_iterations == [batch.solvers[2].metrics.iterations]
    lone.close(), batch.close()


def test_main_runs_solver_fv_fsg(tmp_path):
    r = subprocess.run([sys.executable, str(PKG / "main.py"), "solver=fv/fsg", "N=32", "Re=100"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    res = list(tmp_path.rglob("results.json"))
    assert res, r.stderr[-3000:]
    rec = json.loads(res[0].read_text())
    assert rec["solver"] == "fv_fsg" and rec["run_name"] == "fv_fsg_N32" and rec["metrics"]["converged"] == 1
    assert len(rec["level_iterations"]) == 2 and rec["level_iterations"][1] == rec["metrics"]["iterations"]
    assert rec["params"]["n_levels"] == 2 and rec["params"]["coarsest_n"] == 16
    assert "u_L2_error" in rec["validation_errors"] and "u_rel" in rec["ghia"] and rec["metrics"]["psi_min"] < 0
    assert list(tmp_path.rglob("solution.vts"))
