"""Finite-volume trials that share their launches (mapping="shared", ldc_fv_wide_batch_*) on the GPU.  The phase kernels
are the chip mapping's, so everything here is bit equality: a trial in a batch of mixed sizes against its lone
mapping="chip" run, a lone shared trial against chip, an overflow, a NaN and a quota of 0 that concern one trial only,
eager launches against the replayed graph, solves to the latch, and the launcher."""
import json
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG  # noqa: E402

pytestmark = pytest.mark.gpu

YAML = dict(name="fv", convection_scheme="TVD", alpha_uv=0.4, alpha_p=0.2, linear_solver_tol=1e-9)      # conf/solver/fv.yaml
COUNTERS = ("done", "iterations", "nan", "linear_giveups", "linear_iterations", "momentum_solves", "anderson_fallbacks")

# one work-group with fewer cells than threads; 8 work-groups; ny above 256; nx above 256; G capped at 256 (grid-stride).
# Every trial leaves the batch at another chunk: rings of 5 ... 64 rows, 6 ... 40 iterations
MIXED = [dict(YAML, nx=13, ny=17, Re=400.0, check_every=5, max_iterations=40),
         dict(YAML, nx=37, ny=50, Re=400.0, check_every=7, max_iterations=23),
         dict(YAML, nx=8, ny=300, Re=400.0, convection_scheme="Upwind", corner_treatment="saad", check_every=16,
              max_iterations=6),
         dict(YAML, nx=300, ny=9, Re=400.0, corner_treatment="saad", check_every=64, max_iterations=12),
         dict(YAML, nx=272, ny=260, Re=400.0, check_every=9, max_iterations=8)]


@pytest.fixture(scope="module")
def fv():
    import __graft_entry__ as g
    g.build()
    from solvers.fv.batched import BatchedFVSolver
    from solvers.fv.solver import FVSolver
    return FVSolver, BatchedFVSolver


def _snapshot(s):
    """Everything a solve leaves on the device and in the solver, wall time aside."""
    st = s.state()
    return dict(st, history=np.array(s.history), ctrl=s.t["ctrl"].cpu().numpy().copy(),
                rec=s.t["rec"].cpu().numpy().copy(), counters=s.counters(), iterations=int(s.metrics.iterations),
                converged=bool(s.metrics.converged))


def _same(got, want, what, rec=False):
    for k in ("u", "v", "p", "mdot", "history", "ctrl") + (("rec",) if rec else ()):
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, k)
    for k in COUNTERS:
        assert got["counters"][k] == want["counters"][k], (what, k)
    assert (got["iterations"], got["converged"]) == (want["iterations"], want["converged"]), what


_lone_cache = {}


def _lone_chip(FVSolver, trial, **change):
    """The trial's lone mapping="chip" solve, computed once per trial and shared by the tests."""
    key = json.dumps(dict(trial, **change), sort_keys=True)
    if key not in _lone_cache:
        s = FVSolver(**dict(trial, mapping="chip", **change))
        s.solve()
        _lone_cache[key] = _snapshot(s)
        s.close()
    return _lone_cache[key]


def _shared(trials, **common):
    return [dict(t, mapping="shared", **common) for t in trials]


def test_a_mixed_batch_is_its_lone_chip_runs_bit_for_bit(fv):
    FVSolver, BatchedFVSolver = fv
    trials = [dict(t, tolerance=1e-30) for t in MIXED]
    batch = BatchedFVSolver(_shared(trials))
    batch.solve()
    assert batch.errors == {} and len(batch) == 5
    for q, (s, t) in enumerate(zip(batch.solvers, trials)):
        got = _snapshot(s)
        print(q, f"{t['nx']}x{t['ny']}", got["counters"])
        assert got["iterations"] == t["max_iterations"] and got["history"].shape == (t["max_iterations"], 8)
        _same(got, _lone_chip(FVSolver, t), q)
    shares = sum(s.metrics.wall_time_seconds for s in batch.solvers)
    assert shares == pytest.approx(batch.batch_seconds, rel=1e-9)
    batch.close()


def _run37(FVSolver, mapping, chunks):
    s = FVSolver(**dict(YAML, nx=37, ny=50, Re=400.0, tolerance=1e-30, max_iterations=10**6, check_every=64,
                        mapping=mapping))
    s._begin(1e-30)
    rows = np.concatenate([s._advance(k)[0] for k in chunks], axis=0)
    out = (rows, s.state(), s.t["ctrl"].cpu().numpy().copy(), s.counters())
    s.close()
    return out


def test_a_lone_shared_trial_is_the_chip_trial(fv):
    FVSolver, _ = fv
    rows, st, ctrl, c = _run37(FVSolver, "chip", [40])
    rows2, st2, ctrl2, c2 = _run37(FVSolver, "shared", [7, 7, 7, 7, 7, 5])
    assert rows.shape == (40, 8) and np.array_equal(rows2, rows) and np.array_equal(ctrl2, ctrl)
    for k in ("u", "v", "p", "mdot"):
        assert np.array_equal(st2[k], st[k]), k
    assert {k: c2[k] for k in COUNTERS} == {k: c[k] for k in COUNTERS}


def test_an_overflow_concerns_the_trial_that_overflowed_only(fv):
    """Two BiCGSTAB iterations per SIMPLE iteration are not enough at rtol 1e-12: the tight trial is enqueued again
    with more while its neighbour, which the same launches carried, is done."""
    FVSolver, BatchedFVSolver = fv
    base = dict(YAML, nx=37, ny=50, Re=400.0, tolerance=1e-30, max_iterations=12, check_every=64)
    trials = [dict(base, linear_solver_tol=1e-3), dict(base, linear_solver_tol=1e-12)]
    batch = BatchedFVSolver(_shared(trials, linear_budget=2))
    batch.solve()
    assert batch.errors == {}
    loose, tight = batch.solvers
    print("loose", loose.counters(), "\ntight", tight.counters())
    assert tight.counters()["linear_budget_retries"] > 0
    assert loose.metrics.iterations == 12 and loose.counters()["iterations"] == 12 and loose.history.shape == (12, 8)
    for q, (s, t) in enumerate(zip(batch.solvers, trials)):
        _same(_snapshot(s), _lone_chip(FVSolver, t, linear_budget=16), q)
    batch.close()


def test_a_trial_with_quota_0_is_untouched(fv):
    import torch
    from solvers.fv import ldc_fv_lib as F
    _, BatchedFVSolver = fv
    base = dict(YAML, nx=16, ny=16, Re=100.0, tolerance=1e-30, max_iterations=100, check_every=8)
    batch = BatchedFVSolver(_shared([base, dict(base, nx=24, ny=20)]))
    a, b = batch.solvers
    for s in batch.solvers:
        s._begin(1e-30)
    assert [r[3] for r in batch.shared.advance([2, 2])] == [2, 2]        # both have a state, a record and counters
    names = ("u", "v", "p", "mdot", "rec", "ctrl")
    before = {k: b.t[k].cpu().numpy().copy() for k in names}
    stream = torch.cuda.current_stream(a.device).cuda_stream
    F.wide_batch_enqueue(batch.shared.handle, [3, 0], 12, stream)
    torch.cuda.synchronize()
    for k in names:
        assert np.array_equal(b.t[k].cpu().numpy(), before[k]), k
    assert F.lib().ldc_fv_wide_status(b._wide) == 0 and F.lib().ldc_fv_wide_status(a._wide) == 0
    assert int(a.t["ctrl"][F.CTRL_ITER].item()) == 5 and int(b.t["ctrl"][F.CTRL_ITER].item()) == 2
    batch.close()


def test_eager_launches_and_the_replayed_graph_agree(fv):
    FVSolver, BatchedFVSolver = fv
    trials = [dict(t, tolerance=1e-30) for t in MIXED[:3]]        # the three smallest
    out = {}
    for graph in (False, True):
        batch = BatchedFVSolver(_shared(trials))
        batch.set_wide_graph(graph)
        batch.solve()
        assert batch.errors == {}
        out[graph] = [_snapshot(s) for s in batch.solvers]
        batch.close()
    for q, t in enumerate(trials):
        _same(out[True][q], out[False][q], q, rec=True)
        _same(out[True][q], _lone_chip(FVSolver, t), q)


def test_a_nan_trial_between_two_healthy_ones(fv):
    """The diverging trial of tests/test_gpu_fv_batched.py (16 x 16, Re 1000, no under-relaxation): the kernel's own NaN
    latch stops it, its error is kept, and its neighbours are their lone runs.

    Chunks of 32 iterations: the iteration that meets the NaN never satisfies BiCGSTAB, so its trial is enqueued again
    with 24, 48, ... 1000 BiCGSTAB iterations, each time for the rest of the chunk, and the launches behind the NaN
    latch are empty but not free (22 x 12 600 of them here)."""
    FVSolver, BatchedFVSolver = fv
    from solvers.spectral.ldc_lib import LdcError
    common = dict(YAML, tolerance=1e-5, max_iterations=2000, check_every=32)
    trials = [dict(common, nx=16, ny=16, Re=100.0),
              dict(common, nx=16, ny=16, Re=1000.0, alpha_uv=1.0, alpha_p=1.0),
              dict(common, nx=24, ny=16, Re=400.0)]
    batch = BatchedFVSolver(_shared(trials))
    batch.solve()
    assert list(batch.errors) == [1], batch.errors
    assert isinstance(batch.errors[1], LdcError) and "NaN" in str(batch.errors[1])
    print("NaN trial:", batch.errors[1], batch.solvers[1].counters())
    assert batch.solvers[1].counters()["nan"] == 1
    for q in (0, 2):
        want = _lone_chip(FVSolver, trials[q])
        assert want["converged"]
        _same(_snapshot(batch.solvers[q]), want, q)
    assert sum(batch.solvers[q].metrics.wall_time_seconds for q in (0, 2)) == pytest.approx(batch.batch_seconds, rel=1e-9)
    batch.close()


def test_to_the_latch(fv):
    FVSolver, BatchedFVSolver = fv
    base = dict(YAML, Re=100.0, tolerance=1e-6, max_iterations=40000, check_every=256)
    trials = [dict(base, nx=16, ny=16), dict(base, nx=16, ny=16), dict(base, nx=24, ny=24)]
    batch = BatchedFVSolver(_shared(trials))
    batch.solve()
    assert batch.errors == {}
    for q, (s, t) in enumerate(zip(batch.solvers, trials)):
        want = _lone_chip(FVSolver, t)
        print(q, "iterations", s.metrics.iterations, want["iterations"])
        assert s.metrics.converged is True and want["converged"] is True
        assert s.metrics.iterations == want["iterations"] > 10
        _same(_snapshot(s), want, q)
    batch.close()


def test_the_launcher_batches_a_shared_sweep(tmp_path):
    r = subprocess.run([sys.executable, str(PKG / "main.py"), "-m", "solver=fv", "+solver.mapping=shared", "N=16,24",
                        "Re=100"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    recs = [json.loads(f.read_text()) for f in tmp_path.rglob("results.json")]
    assert sorted(x["N"] for x in recs) == [16, 24], r.stderr[-3000:]
    for x in recs:
        assert x["solver"] == "fv" and x["metrics"]["converged"] == 1 and x["metrics"]["iterations"] > 10
        assert x["solve_batch_size"] == 2
    log = r.stdout + r.stderr + "".join(f.read_text() for f in tmp_path.rglob("*.log"))
    assert "batched solve of 2 FV trials" in log, log[-3000:]
