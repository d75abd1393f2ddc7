"""Anderson acceleration of chip and shared finite-volume trials on the GPU (csrc/ldc_fv_wide_anderson.inc through
``acceleration="anderson_chip"``): the mixed iteration against the NumPy restatement (tests/fv_anderson_numpy.py) up to
300 x 260 cells, bit equality over chunks, budgets, graphs, repeats and batches of mixed and plain trials, an overflowed
iteration that is not mixed, the fallback, convergence at 16 x 16, sequencing and the launcher."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import fv_anderson_numpy as AA  # noqa: E402
from fv_numpy import FVState  # noqa: E402
from test_fv_anderson_cpu import COND_MAX, GPU_CASES, GPU_START  # noqa: E402

from conftest import PKG  # noqa: E402

pytestmark = pytest.mark.gpu

YAML = dict(name="fv", convection_scheme="TVD", alpha_uv=0.4, alpha_p=0.2, linear_solver_tol=1e-9)      # conf/solver/fv.yaml
STATE = ("u", "v", "p", "mdot")
FIXED = dict(YAML, Re=100.0, tolerance=1e-30, check_every=16)        # a fixed number of iterations, the ring of 16 rows
MIXING = dict(acceleration="anderson_chip", anderson_start=GPU_START)

# (nx, ny, Re, FVState keywords, depth, iterations): the three cases of the one-CU test, then 8 work-groups, a thin trial
# with one axis above 256, and both axes above 256 with G capped at 256 and the ring of 5 filling (6 columns in 8 iterations)
CASES = {name: (nx, ny, 100.0, kw, depth, K) for name, (nx, ny, kw, depth, K) in GPU_CASES.items()}
CASES.update({"37x50-re400": (37, 50, 400.0, {}, 3, 12),
              "8x300-thin": (8, 300, 100.0, {}, 3, 8),
              "300x260-re1000-depth5": (300, 260, 1000.0, {}, 5, 8)})


@pytest.fixture(scope="module")
def fv():
    import __graft_entry__ as g
    g.build()
    from solvers.fv.batched import BatchedFVSolver
    from solvers.fv.fsg import FVFSGSolver
    from solvers.fv.solver import FVSolver, prolong
    return FVSolver, BatchedFVSolver, FVFSGSolver, prolong


def _snapshot(s):
    """Everything a solve leaves on the device and in the solver, wall time aside."""
    return dict(s.state(), history=np.array(s.history), ctrl=s.t["ctrl"].cpu().numpy().copy(),
                astate=s.t["astate"].cpu().numpy().copy(), counters=s.counters(), iterations=int(s.metrics.iterations),
                converged=bool(s.metrics.converged))


def _same(got, want, what):
    for k in STATE + ("history", "ctrl", "astate"):
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, k)
    assert got["counters"] == want["counters"], what
    assert (got["iterations"], got["converged"]) == (want["iterations"], want["converged"]), what


# ------------------------------------------------------------------------------------------- 1. the restatement
@pytest.mark.parametrize("case", sorted(CASES))
def test_mixed_iterations_on_the_chip_agree_with_the_restatement(fv, case):
    """``anderson_start=2``: mixed from iteration 3 on.  The bound of the one-CU test: 1e-9 max(1, cond) with cond the
    largest condition number of the restatement's regularised Gram matrices -- times max|field| for the fields, and for
    every entry of the record rows times its own size."""
    nx, ny, Re, kw, depth, K = CASES[case]
    ref = FVState(nx, ny, Re, **kw)
    rows, mixer = AA.run(ref, K, depth=depth, start=GPU_START)
    assert mixer.cond <= COND_MAX and mixer.fallbacks == 0 and np.all(np.isfinite(rows))
    s = fv[0](**dict({**FIXED, **MIXING, **kw}, Re=Re, nx=nx, ny=ny, anderson_depth=depth, max_iterations=K,
                     mapping="chip"))
    s.solve()
    bound = 1e-9 * max(1.0, mixer.cond)
    st = s.state()
    want = dict(u=ref.u.ravel(), v=ref.v.ravel(), p=ref.p.ravel(), mdot=np.concatenate([ref.fx.ravel(), ref.fy.ravel()]))
    ratios = {k: float(np.max(np.abs(st[k] - want[k])) / np.max(np.abs(want[k]))) / bound for k in STATE}
    assert s.history.shape == rows.shape == (K, 8)
    ratios["rows"] = float(np.max(np.abs(s.history[:, :7] - rows[:, :7]) / np.abs(rows[:, :7]))) / bound
    print(f"{case}: cond {mixer.cond:.3e}, bound {bound:.2e}, error / bound", {k: f"{r:.2e}" for k, r in ratios.items()},
          s.counters())
    c = s.counters()
    assert c["iterations"] == K and c["nan"] == 0 and c["anderson_fallbacks"] == 0
    assert list(s.t["astate"].cpu().numpy()) == [mixer.ncol, mixer.pos, K, 0]
    assert all(np.all(np.isfinite(st[k])) for k in STATE) and st["p"][0] == 0.0
    assert all(r <= 1.0 for r in ratios.values()), ratios
    s.close()


# ------------------------------------------------------------------------------------------- 2. bit for bit
def _run37(fv, chunks, graph=None, **kw):
    s = fv[0](**dict({**YAML, **MIXING}, nx=37, ny=50, Re=400.0, anderson_depth=3, tolerance=1e-30, max_iterations=10**6,
                     check_every=64, mapping="chip", **kw))
    if graph is not None:
        s.set_wide_graph(graph)
    s._begin(1e-30)
    rows = np.concatenate([s._advance(k)[0] for k in chunks], axis=0)
    out = dict(s.state(), rows=rows, ctrl=s.t["ctrl"].cpu().numpy().copy(), astate=s.t["astate"].cpu().numpy().copy(),
               retries=s.counters()["linear_budget_retries"])
    s.close()
    return out


def test_mixed_runs_repeat_bit_for_bit_whatever_the_chunks_the_budget_and_the_graph(fv):
    """37 x 50, depth 3, 40 iterations.  The last iteration of every enqueue is mixed like any other, an iteration that
    overflowed is not mixed, and the mixing launches are part of the replayed graph."""
    base = _run37(fv, [40])
    assert base["rows"].shape == (40, 8) and list(base["astate"]) == [3, (40 - 2) % 3, 40, 0]
    plain = fv[0](**dict(YAML, nx=37, ny=50, Re=400.0, tolerance=1e-30, max_iterations=40, check_every=64, mapping="chip"))
    plain.solve()
    assert not np.array_equal(plain.state()["u"], base["u"])        # (it was mixed)
    plain.close()
    others = {"again": _run37(fv, [40]), "16-16-8": _run37(fv, [16, 16, 8]), "1 x 40": _run37(fv, [1] * 40),
              "budget 2": _run37(fv, [40], linear_budget=2), "budget 16": _run37(fv, [40], linear_budget=16),
              "eager": _run37(fv, [40], graph=False), "graph": _run37(fv, [40], graph=True),
              "graph 16-16-8 budget 2": _run37(fv, [16, 16, 8], graph=True, linear_budget=2)}
    assert others["budget 2"]["retries"] > 0
    for what, got in others.items():
        for k in STATE + ("rows", "ctrl", "astate"):
            assert got[k].shape == base[k].shape and np.array_equal(got[k], base[k]), (what, k)


# ------------------------------------------------------------------------------------------- 3. depth 0, plain neighbours
# five sizes: one work-group with fewer cells than threads, one work-group, 8, a thin trial, G capped at 256
BATCH = [dict({**FIXED, **MIXING}, nx=8, ny=8, anderson_depth=16, check_every=5, max_iterations=12),
         dict(FIXED, nx=13, ny=17, check_every=7, max_iterations=10),
         dict({**FIXED, **MIXING}, nx=37, ny=50, Re=400.0, anderson_depth=3, check_every=16, max_iterations=14),
         dict(FIXED, nx=8, ny=300, convection_scheme="Upwind", corner_treatment="saad", check_every=64, max_iterations=6),
         dict({**FIXED, **MIXING}, nx=300, ny=260, Re=1000.0, anderson_depth=5, check_every=9, max_iterations=8)]


@pytest.fixture(scope="module")
def lone_five(fv):
    """The five trials of BATCH solved alone with mapping="chip", shared and left unchanged."""
    out = []
    for t in BATCH:
        s = fv[0](**dict(t, mapping="chip"))
        s.solve()
        out.append(_snapshot(s))
        s.close()
    return out


@pytest.mark.parametrize("graph", [False, True])
def test_a_batch_of_mixed_and_plain_trials_is_its_lone_chip_runs(fv, lone_five, graph):
    batch = fv[1]([dict(t, mapping="shared") for t in BATCH])
    batch.set_wide_graph(graph)
    batch.solve()
    assert batch.errors == {}
    for q, (s, t) in enumerate(zip(batch.solvers, BATCH)):
        got = _snapshot(s)
        print(q, f"{t['nx']}x{t['ny']}", got["counters"], list(got["astate"]))
        assert got["iterations"] == t["max_iterations"]
        assert s.mixed_chip == ("acceleration" in t) and not s.accelerated
        _same(got, lone_five[q], q)
    assert list(lone_five[0]["astate"]) == [10, 10, 12, 0] and list(lone_five[1]["astate"]) == [0, 0, 0, 0]
    assert list(lone_five[4]["astate"]) == [5, 1, 8, 0]
    batch.close()


def test_a_plain_trial_beside_mixed_ones_is_the_plain_trial_of_a_plain_batch(fv, lone_five):
    from solvers.fv import ldc_fv_lib as F
    plain = fv[1]([dict({k: v for k, v in t.items() if k not in MIXING and k != "anderson_depth"}, mapping="shared")
                   for t in BATCH])
    assert plain.shared is not None and not any(s.mixed_chip for s in plain.solvers)
    assert F.lib().ldc_fv_wide_batch_launches(plain.shared.handle, 12) == 11 + 5 * 12        # today's chain
    plain.solve()
    assert plain.errors == {}
    for q in (1, 3):
        _same(_snapshot(plain.solvers[q]), lone_five[q], q)
    assert not np.array_equal(plain.solvers[2].state()["u"], lone_five[2]["u"])       # (without mixing: another run)
    plain.close()


def test_quotas_that_differ_per_trial_give_the_same_bits(fv, lone_five):
    """The batch object driven by hand: every trial reaches its count in two enqueues whose quotas differ per trial, one of
    them 0 for some.  A trial's last iteration of an enqueue is mixed although its row count has reached its quota."""
    from solvers.fv import ldc_fv_lib as F
    batch = fv[1]([dict(t, mapping="shared", check_every=16) for t in BATCH])
    assert F.lib().ldc_fv_wide_batch_launches(batch.shared.handle, 12) == 11 + 5 * 12 + F.WIDE_ANDERSON_LAUNCHES
    for s in batch.solvers:
        s._begin(1e-30)
    totals = [t["max_iterations"] for t in BATCH]
    first = [5, 10, 1, 0, 3]
    out1 = batch.shared.advance(first)
    out2 = batch.shared.advance([n - k for n, k in zip(totals, first)])
    for q, s in enumerate(batch.solvers):
        rows = np.concatenate([out1[q][0], out2[q][0]], axis=0)
        want = lone_five[q]
        assert np.array_equal(rows, want["history"]), q
        st = s.state()
        for k in STATE:
            assert np.array_equal(st[k], want[k]), (q, k)
        assert np.array_equal(s.t["ctrl"].cpu().numpy(), want["ctrl"]), q
        assert np.array_equal(s.t["astate"].cpu().numpy(), want["astate"]), q
    batch.close()


# ------------------------------------------------------------------------------------------- 4. overflow
def test_an_overflowed_iteration_is_not_mixed(fv):
    import torch
    from solvers.fv import ldc_fv_lib as F
    kw = dict({**YAML, **MIXING}, nx=37, ny=50, Re=400.0, anderson_depth=3, tolerance=1e-30, max_iterations=12,
              check_every=16, mapping="chip")
    s = fv[0](**kw)
    s._begin(1e-30)
    s._advance(5)                                            # a state, three columns, a record
    names = STATE + ("ctrl", "astate", "hist", "rec")
    before = {k: s.t[k].cpu().numpy().copy() for k in names}
    assert list(before["astate"]) == [3, 0, 5, 0]
    with torch.cuda.device(s.device):
        F.check(F.lib().ldc_fv_wide_enqueue(s._wide, 4, 1, s._stream()), "ldc_fv_wide_enqueue")      # ONE BiCGSTAB iteration
        torch.cuda.current_stream(s.device).synchronize()
    assert F.lib().ldc_fv_wide_status(s._wide) == F.E_BUDGET
    for k in names:
        assert np.array_equal(s.t[k].cpu().numpy(), before[k]), k
    s.close()
    tight, wide = fv[0](**dict(kw, linear_budget=1)), fv[0](**dict(kw, linear_budget=16))
    tight.solve(), wide.solve()
    print("budget 1:", tight.counters(), "budget 16:", wide.counters())
    assert tight.counters()["linear_budget_retries"] > 0
    a, b = _snapshot(tight), _snapshot(wide)
    a["counters"].pop("linear_budget_retries"), b["counters"].pop("linear_budget_retries")
    _same(a, b, "budget 1 against 16")
    assert np.array_equal(tight.t["hist"].cpu().numpy(), wide.t["hist"].cpu().numpy())
    tight.close(), wide.close()


# ------------------------------------------------------------------------------------------- 5. fallback
def test_a_lid_at_rest_counts_its_fallbacks_on_the_chip(fv):
    """8 x 8, depth 3 from iteration 2, the lid's profile zeroed: f = 0, so every Gram matrix is 0 and its first pivot is
    0.  As the restatement and the one-CU kernel: a fallback at iterations 3 ... 10, the latch at the warm-up (11)."""
    s = fv[0](**dict({**YAML, **MIXING}, nx=8, ny=8, Re=100.0, anderson_depth=3, tolerance=1e-6, max_iterations=200,
                     check_every=16, mapping="chip"))
    s.t["ulid"].zero_()
    s.solve()
    c, st = s.counters(), s.state()
    print("lid at rest:", c, list(s.t["astate"].cpu().numpy()))
    assert s.metrics.converged and c["iterations"] == 11 and c["nan"] == 0
    assert c["anderson_fallbacks"] == 8 and list(s.t["astate"].cpu().numpy()) == [0, 0, 11, 8]
    assert np.all(np.isfinite(s.history[:, :4])) and all(np.all(st[k] == 0.0) for k in STATE)
    s.close()


# ------------------------------------------------------------------------------------------- 6. convergence
@pytest.fixture(scope="module")
def restated_16():
    """max|du|, max|dv| between the restatement's plain and depth-5 runs at 16 x 16, Re = 100, tolerance 1e-6."""
    plain, acc = FVState(16, 16, 100.0), FVState(16, 16, 100.0)
    rp, _ = AA.run(plain, 20000, depth=0, tol=1e-6)
    ra, _ = AA.run(acc, 20000, depth=5, start=10, tol=1e-6)
    return len(rp), len(ra), float(np.max(np.abs(plain.u - acc.u))), float(np.max(np.abs(plain.v - acc.v)))


def test_acceleration_halves_the_iterations_at_16_on_the_chip(fv, restated_16):
    """The YAML's settings.  At most 0.5 x the plain chip run's iterations (the restatement: 0.23; the factor 2 is for the
    sensitivity of the mixed path to rounding), and fields within 4 x what the restatement's two runs differ by."""
    common = dict(YAML, nx=16, ny=16, Re=100.0, tolerance=1e-6, max_iterations=20000, check_every=256, mapping="chip")
    plain = fv[0](**common)
    acc = fv[0](**dict(common, acceleration="anderson_chip"))    # depth 5 from iteration 10
    plain.solve(), acc.solve()
    n_plain, n_acc, du_ref, dv_ref = restated_16
    a, b = plain.state(), acc.state()
    du, dv = float(np.max(np.abs(a["u"] - b["u"]))), float(np.max(np.abs(a["v"] - b["v"])))
    print(f"iterations: plain {plain.metrics.iterations} (restatement {n_plain}), depth 5 {acc.metrics.iterations} "
          f"({n_acc}); max|du| {du:.3e} ({du_ref:.3e}), max|dv| {dv:.3e} ({dv_ref:.3e}); counters {acc.counters()}")
    assert plain.metrics.converged and acc.metrics.converged
    assert plain.counters()["anderson_fallbacks"] == 0 and list(plain.t["astate"].cpu().numpy()) == [0, 0, 0, 0]
    assert acc.metrics.iterations <= 0.5 * plain.metrics.iterations
    assert du <= 4 * du_ref and dv <= 4 * dv_ref
    assert b["p"][0] == 0.0 and a["p"][0] == 0.0
    plain.close(), acc.close()


# ------------------------------------------------------------------------------------------- 7. sequencing
def test_an_accelerated_chip_sequence_is_the_same_steps_done_by_hand(fv):
    """solver=fv/fsg with mapping=chip and acceleration=anderson_chip, 16 -> 32: the levels inherit both."""
    FVSolver, _, FVFSGSolver, prolong = fv
    common = dict(YAML, nx=32, ny=32, Re=100.0, tolerance=1e-5, max_iterations=20000, check_every=256, mapping="chip",
                  acceleration="anderson_chip")
    seq = FVFSGSolver(**dict(common, name="fv_fsg"))
    seq.solve()
    coarse = FVSolver(**dict(common, nx=16, ny=16))
    coarse.solve()
    fine = FVSolver(**common)
    prolong([(coarse, fine)])
    fine.solve()
    print("iterations per level", seq.level_iterations, "counters", seq.counters())
    assert seq.metrics.converged and [coarse.metrics.iterations, fine.metrics.iterations] == seq.level_iterations
    assert coarse.mixed_chip and fine.mixed_chip and seq.mixed_chip
    _same(_snapshot(seq), _snapshot(fine), "by hand")
    assert fine.counters()["iterations"] > 10 and fine.t["astate"][2].item() == fine.counters()["iterations"]
    seq.close(), coarse.close(), fine.close()


# ------------------------------------------------------------------------------------------- 8. the launcher
def test_main_runs_an_accelerated_chip_trial(tmp_path):
    r = subprocess.run([sys.executable, str(PKG / "main.py"), "solver=fv", "N=16", "+solver.mapping=chip",
                        "+solver.acceleration=anderson_chip", "Re=100"], cwd=tmp_path, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    res = list(tmp_path.rglob("results.json"))
    assert res, r.stderr[-3000:]
    rec = json.loads(res[0].read_text())
    assert rec["solver"] == "fv" and rec["metrics"]["converged"] == 1
    assert rec["params"]["acceleration"] == "anderson_chip"
    assert rec["counters"]["anderson_fallbacks"] >= 0 and rec["counters"]["iterations"] == rec["metrics"]["iterations"]
