"""Batched finite-volume trials on the GPU (solvers/fv/batched.py): a batch of mixed sizes and settings against lone
runs bit for bit, against the reference's trajectory fixtures (g14), over more than one launch (> 256 trials), with a
trial that goes NaN in its middle, and through the launcher end to end."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"

from conftest import PKG  # noqa: E402

pytestmark = pytest.mark.gpu

YAML = dict(name="fv", convection_scheme="TVD", alpha_uv=0.4, alpha_p=0.2, linear_solver_tol=1e-9)      # conf/solver/fv.yaml


@pytest.fixture(scope="module")
def fv():
    import __graft_entry__ as g
    g.build()
    from solvers.fv.batched import BatchedFVSolver
    from solvers.fv.solver import FVSolver
    return FVSolver, BatchedFVSolver


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def _assert_same_trial(batched, lone, what):
    """Everything a solve leaves behind, bit for bit (wall time aside)."""
    assert batched.metrics.iterations == lone.metrics.iterations, what
    assert batched.metrics.converged == lone.metrics.converged, what
    assert batched.history.shape == lone.history.shape and np.array_equal(batched.history, lone.history), what
    sb, sl = batched.state(), lone.state()
    for k in ("u", "v", "p", "mdot"):
        assert np.array_equal(sb[k], sl[k]), (what, k)
    assert batched.counters() == lone.counters(), what
    mb, ml = batched.metrics.as_dict(), lone.metrics.as_dict()
    assert set(mb) == set(ml)
    for k in ml:
        if k != "wall_time_seconds":
            assert np.array_equal(mb[k], ml[k]), (what, k, mb[k], ml[k])


def test_batch_equals_lone_runs(fv):
    """Five converging trials of different sizes, Re, lid and scheme plus one capped at 300 iterations, as ONE batch."""
    FVSolver, BatchedFVSolver = fv
    common = dict(YAML, tolerance=1e-5, max_iterations=20000, check_every=256)
    trials = [dict(common, nx=16, ny=16, Re=100.0),
              dict(common, nx=24, ny=16, Re=400.0),
              dict(common, nx=20, ny=20, Re=100.0),
              dict(common, nx=24, ny=24, Re=400.0, corner_treatment="saad"),
              dict(common, nx=16, ny=16, Re=100.0, convection_scheme="Upwind"),
              dict(common, nx=16, ny=16, Re=100.0, max_iterations=300)]
    batch = BatchedFVSolver(trials)
    batch.solve()
    assert batch.errors == {} and len(batch) == 6 and batch.batch_size == 6
    lone = [FVSolver(**t) for t in trials]
    for s in lone:
        s.solve()
    for q, (b, s) in enumerate(zip(batch.solvers, lone)):
        print(q, "iterations", b.metrics.iterations, s.metrics.iterations, "converged", b.metrics.converged)
        _assert_same_trial(b, s, q)
    assert all(s.metrics.converged for s in batch.solvers[:5])
    capped = batch.solvers[5]
    assert capped.history.shape == (300, 8) and capped.metrics.iterations == 300 and capped.metrics.converged is False
    shares = sum(s.metrics.wall_time_seconds for s in batch.solvers)
    assert shares == pytest.approx(batch.batch_seconds, rel=1e-9)
    batch.close()
    for s in lone:
        s.close()


def test_batch_matches_the_reference_trajectories(fv):
    """All Upwind trajectory cases of the reference (16 ... 48 cells and 24 x 16) as ONE batch, each capped at its K;
    bounds of the lone test (tests/test_gpu_fv.py::test_upwind_trajectories_match_reference)."""
    _, BatchedFVSolver = fv
    g = np.load(GOLD / "g14_fv_traj.npz")
    meta = json.loads((GOLD / "g14_fv_traj.json").read_text())
    tags = list(meta)
    assert len(tags) >= 7 and len({(meta[t]["nx"], meta[t]["ny"]) for t in tags}) >= 4
    batch = BatchedFVSolver([dict(name="fv", Re=m["Re"], nx=m["nx"], ny=m["ny"], corner_treatment=m.get("lid", "none"),
                                  alpha_uv=m["alpha_uv"], alpha_p=m["alpha_p"], linear_solver_tol=m["linear_solver_tol"],
                                  convection_scheme=m["convection_scheme"], tolerance=1e-30, max_iterations=m["K"],
                                  check_every=256) for m in (meta[t] for t in tags)])
    batch.solve()
    assert batch.errors == {}
    for tag, s in zip(tags, batch.solvers):
        ref = g[f"{tag}_rec"]
        assert s.history.shape == ref.shape, tag
        err = float(np.max(np.abs(s.history[:, :7] - ref[:, :7]) / np.abs(ref[:, :7])))
        print(tag, "rows", err)
        assert err <= 1e-8, tag
        st = s.state()
        for k in ("u", "v", "p", "mdot"):
            assert _rel(st[k], g[f"{tag}_{k}"]) <= 1e-8, (tag, k)
    batch.close()


def test_more_trials_than_one_launch_takes(fv):
    """260 trials of 8 x 8 cells, Re spread over 100 ... 1000, 40 iterations each: ldc_fv_batch_enqueue needs two
    launches (256 + 4).  All 260 report 40 iterations; trials 0, 255, 256 and 259 are bit-equal to lone runs.

    The relaxation is 0.05 / 0.05, not the YAML's 0.4 / 0.2: on 8 x 8 cells SIMPLE started from rest with 0.4 / 0.2
    diverges above Re ~370 in the reference itself (Re 444, Upwind: relative change 2.6e13 at iteration 13, then its
    BiCGSTAB raises), and the NumPy restatement (tests/fv_numpy.py) goes NaN within 40 iterations for 129 of these 260
    trials.  With 0.05 / 0.05 the restatement keeps all 260 bounded (max |u|, |v| 0.32 of the lid speed)."""
    FVSolver, BatchedFVSolver = fv
    from solvers.fv import ldc_fv_lib as F
    n = 260
    assert n > F.LAUNCH_MAX
    trials = [dict(YAML, alpha_uv=0.05, alpha_p=0.05, nx=8, ny=8, Re=100.0 + 900.0 * q / (n - 1), tolerance=1e-30,
                   max_iterations=40, check_every=64) for q in range(n)]
    batch = BatchedFVSolver(trials)
    batch.solve()
    print("trials stopped on a NaN:", len(batch.errors), "of", n, sorted(batch.errors)[:8])
    assert batch.errors == {}
    assert [s.metrics.iterations for s in batch.solvers] == [40] * n
    assert all(s.history.shape == (40, 8) and np.all(np.isfinite(s.history)) for s in batch.solvers)
    for q in (0, 255, 256, 259):
        lone = FVSolver(**trials[q])
        lone.solve()
        _assert_same_trial(batch.solvers[q], lone, q)
        lone.close()
    batch.close()


def test_a_nan_trial_is_reported_and_its_neighbours_are_untouched(fv):
    """Without under-relaxation the 16 x 16, Re 1000 trial overflows within about ten iterations (the NumPy restatement:
    NaN at iteration 10); the kernel's own NaN latch stops it.  The batch raises nothing."""
    FVSolver, BatchedFVSolver = fv
    from solvers.spectral.ldc_lib import LdcError
    common = dict(YAML, tolerance=1e-5, max_iterations=2000, check_every=256)
    trials = [dict(common, nx=16, ny=16, Re=100.0),
              dict(common, nx=16, ny=16, Re=1000.0, alpha_uv=1.0, alpha_p=1.0),
              dict(common, nx=24, ny=16, Re=400.0)]
    batch = BatchedFVSolver(trials)
    batch.solve()
    assert list(batch.errors) == [1], batch.errors
    assert isinstance(batch.errors[1], LdcError) and "NaN" in str(batch.errors[1])
    print("NaN trial:", batch.errors[1], batch.solvers[1].counters())
    assert batch.solvers[1].counters()["nan"] == 1
    for q in (0, 2):
        lone = FVSolver(**trials[q])
        lone.solve()
        assert lone.metrics.converged
        _assert_same_trial(batch.solvers[q], lone, q)
        lone.close()
    assert sum(batch.solvers[q].metrics.wall_time_seconds for q in (0, 2)) == pytest.approx(batch.batch_seconds, rel=1e-9)
    batch.close()


def _sweep(tmp, max_batch):
    env = {k: v for k, v in os.environ.items() if k != "LDC_MAX_BATCH"}
    if max_batch is not None:
        env["LDC_MAX_BATCH"] = str(max_batch)
    tmp.mkdir()
    r = subprocess.run([sys.executable, str(PKG / "main.py"), "-m", "solver=fv", "N=16,24", "Re=100,400", "tolerance=1e-5"],
                       cwd=tmp, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    jobs = {}
    for f in tmp.rglob("results.json"):
        assert (f.parent / "solution.vts").exists(), f.parent
        jobs[int(f.parent.name)] = json.loads(f.read_text())
    assert sorted(jobs) == [0, 1, 2, 3], (sorted(jobs), r.stderr[-3000:])
    gathered = json.loads(next(tmp.rglob("sweep_results.json")).read_text())
    assert len(gathered) == 4 and not any("error" in g for g in gathered)
    return jobs


def test_launcher_batches_an_fv_sweep_and_changes_no_result(tmp_path):
    batched = _sweep(tmp_path / "batched", None)
    lone = _sweep(tmp_path / "lone", 1)
    for j in range(4):
        b, s = batched[j], lone[j]
        assert b["solver"] == s["solver"] == "fv" and (b["N"], b["Re"]) == (s["N"], s["Re"])
        mb, ms = dict(b["metrics"]), dict(s["metrics"])
        mb.pop("wall_time_seconds"), ms.pop("wall_time_seconds")
        print(j, b["N"], b["Re"], "iterations", mb["iterations"], ms["iterations"])
        assert mb == ms and mb["converged"] == 1, j
        for k in ("validation_errors", "ghia", "objective", "validation_table"):
            assert b[k] == s[k], (j, k)
        assert b["solve_batch_size"] == 4 and "solve_batch_seconds" in b
        assert "solve_batch_size" not in s
    assert {(r["N"], r["Re"]) for r in batched.values()} == {(16, 100), (16, 400), (24, 100), (24, 400)}


def test_mixed_sweep_keeps_fv_chunks_and_co_resident_spectral_chunks_apart(tmp_path):
    """``solver=fv,spectral/sg``: four FV trials (N = 64, 96) as one batch in the same pool of streams as two spectral
    batches whose work-groups must all be resident -- N = 64 on the one-XCD-per-trial kernel (mode 3) and, with
    LDC_BATCH_WIDE=1, N = 96 on the chip-wide kernel (mode 5).  An FV work-group holds its CU for a whole chunk, so the
    chunks take turns (ldc_lib.resident_lock); a spectral launch that found CUs taken would give up its barrier wait
    and leave error records for its whole batch."""
    env = {k: v for k, v in os.environ.items() if k not in ("LDC_MAX_BATCH", "LDC_PIN_MODE")}
    env["LDC_BATCH_WIDE"] = "1"
    r = subprocess.run([sys.executable, str(PKG / "main.py"), "-m", "solver=fv,spectral/sg", "N=64,96", "Re=100,400",
                        "tolerance=1e-5"], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    recs = json.loads(next(tmp_path.rglob("sweep_results.json")).read_text())
    assert len(recs) == 8
    assert not any("error" in x for x in recs), [x.get("error") for x in recs]
    fvs = [x for x in recs if x["solver"] == "fv"]
    sgs = [x for x in recs if x["solver"] != "fv"]
    assert len(fvs) == 4 and len(sgs) == 4
    print([(x["solver"], x["N"], x["Re"], x["metrics"]["iterations"], x.get("kernel_mode"), x.get("solve_batch_size")) for x in recs])
    assert all(x["metrics"]["converged"] == 1 for x in recs)
    assert all(x["solve_batch_size"] == 4 and x["solve_streams"] >= 2 for x in fvs)
    assert {x["N"]: x["kernel_mode"] for x in sgs} == {64: 3, 96: 5}
