"""Anderson acceleration of the finite-volume SIMPLE iteration on the GPU (csrc/ldc_fv_anderson.hip through
``acceleration="anderson"``): depth 0 against the plain launch, the mixed iteration against the NumPy restatement
(tests/fv_anderson_numpy.py), repeats and batches bit for bit, convergence at 16 x 16, the fallback and sequencing."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import fv_anderson_numpy as AA  # noqa: E402
from fv_numpy import FVState  # noqa: E402
from test_fv_anderson_cpu import COND_MAX, GPU_CASES, GPU_START, restated  # noqa: E402

pytestmark = pytest.mark.gpu

YAML = dict(name="fv", convection_scheme="TVD", alpha_uv=0.4, alpha_p=0.2, linear_solver_tol=1e-9)      # conf/solver/fv.yaml
STATE = ("u", "v", "p", "mdot")
FIXED = dict(YAML, Re=100.0, tolerance=1e-30, check_every=16)        # a fixed number of iterations, the ring of 16 rows
ANDERSON = dict(acceleration="anderson", anderson_start=GPU_START)
# the trials of the bit-for-bit tests: 13 x 17 depth 3, 16 x 16 plain, 24 x 16 depth 5; 40 iterations in chunks of 16
TRIO = [dict({**FIXED, **ANDERSON}, nx=13, ny=17, anderson_depth=3, max_iterations=40),
        dict(FIXED, nx=16, ny=16, max_iterations=40),
        dict({**FIXED, **ANDERSON}, nx=24, ny=16, anderson_depth=5, max_iterations=40, convection_scheme="Upwind",
             corner_treatment="saad")]


@pytest.fixture(scope="module")
def fv():
    import __graft_entry__ as g
    g.build()
    from solvers.fv.batched import BatchedFVSolver
    from solvers.fv.fsg import FVFSGSolver
    from solvers.fv.solver import FVSolver, prolong
    return FVSolver, BatchedFVSolver, FVFSGSolver, prolong


@pytest.fixture(scope="module")
def lone_trio(fv):
    """The three trials of TRIO solved alone (the plain one by the plain launch), shared and left unchanged."""
    out = [fv[0](**t) for t in TRIO]
    for s in out:
        s.solve()
    yield out
    for s in out:
        s.close()


def _assert_same_trial(a, b, what):
    """Everything a solve leaves behind, bit for bit (wall time aside)."""
    assert a.metrics.iterations == b.metrics.iterations and a.metrics.converged == b.metrics.converged, what
    assert a.history.shape == b.history.shape and np.array_equal(a.history, b.history), what
    sa, sb = a.state(), b.state()
    for k in STATE:
        assert np.array_equal(sa[k], sb[k]), (what, k)
    assert a.counters() == b.counters(), what


# ------------------------------------------------------------------------------------------- (a) depth 0
def test_depth_0_through_the_mixing_path_equals_the_plain_solve(fv):
    """13 x 17 TVD, 40 iterations in chunks of 16, 16 and 8.  Beside an accelerated trial the plain one is advanced by
    launches of ONE iteration and the mixing kernel at depth 0, which only moves its record rows into place."""
    FVSolver, Batched, _, _ = fv
    plain = dict(FIXED, nx=13, ny=17, max_iterations=40)
    lone = FVSolver(**plain)
    lone.solve()
    batch = Batched([plain, dict({**plain, **ANDERSON}, anderson_depth=3)])
    batch.solve()
    assert batch.errors == {} and lone.history.shape == (40, 8)
    assert not lone.accelerated and not batch.solvers[0].accelerated and batch.solvers[1].accelerated
    _assert_same_trial(batch.solvers[0], lone, "depth 0")
    assert np.array_equal(batch.solvers[0].t["rec"].cpu().numpy()[:8], lone.t["rec"].cpu().numpy()[:8])      # the last chunk
    assert lone.counters()["iterations"] == 40 and lone.counters()["anderson_fallbacks"] == 0
    assert not np.array_equal(batch.solvers[1].state()["u"], lone.state()["u"])       # (the neighbour was mixed)
    lone.close(), batch.close()


# ------------------------------------------------------------------------------------------- (b), (c) the restatement
@pytest.mark.parametrize("case", sorted(GPU_CASES))
def test_mixed_iterations_agree_with_the_restatement(fv, case):
    """``anderson_start=2``: mixed from iteration 3 on (the first keeps x, the second gives f, the third a column).
    Depth 3 over 12 iterations wraps the ring three times; depth 16 at 8 x 8 never fills it.  Bound: 1e-9 max(1, cond)
    with cond the largest condition number of the restatement's regularised Gram matrices -- times max|field| for the
    fields, and for every entry of the record rows times its own size (no weaker: an entry is at most its column's
    maximum)."""
    nx, ny, kw, depth, K = GPU_CASES[case]
    ref, rows, mixer = restated(case)
    assert mixer.cond <= COND_MAX and mixer.fallbacks == 0
    s = fv[0](**dict({**FIXED, **ANDERSON, **kw}, nx=nx, ny=ny, anderson_depth=depth, max_iterations=K))
    s.solve()
    bound = 1e-9 * max(1.0, mixer.cond)
    st = s.state()
    want = dict(u=ref.u.ravel(), v=ref.v.ravel(), p=ref.p.ravel(), mdot=np.concatenate([ref.fx.ravel(), ref.fy.ravel()]))
    ratios = {k: float(np.max(np.abs(st[k] - want[k])) / np.max(np.abs(want[k]))) / bound for k in STATE}
    assert s.history.shape == rows.shape == (K, 8)
    ratios["rows"] = float(np.max(np.abs(s.history[:, :7] - rows[:, :7]) / np.abs(rows[:, :7]))) / bound
    print(f"{case}: cond {mixer.cond:.3e}, bound {bound:.2e}, error / bound", {k: f"{r:.2e}" for k, r in ratios.items()})
    c = s.counters()
    assert c["iterations"] == K and c["nan"] == 0 and c["anderson_fallbacks"] == 0
    a = s.t["astate"].cpu().numpy()
    assert list(a) == [mixer.ncol, mixer.pos, K, 0]
    assert all(np.all(np.isfinite(st[k])) for k in STATE) and st["p"][0] == 0.0
    assert all(r <= 1.0 for r in ratios.values()), ratios
    s.close()


# ------------------------------------------------------------------------------------------- (d) bit for bit
def test_two_identical_accelerated_runs_agree_bit_for_bit(fv, lone_trio):
    for t, first in zip(TRIO, lone_trio):
        if t.get("acceleration") == "anderson":
            again = fv[0](**t)
            again.solve()
            _assert_same_trial(again, first, (t["nx"], t["ny"]))
            again.solve()                                   # a repeat solve starts its history over: no NaN, 40 more
            assert again.counters()["iterations"] == 40 and np.all(np.isfinite(again.history))
            again.close()


def test_a_batch_of_three_equals_the_three_alone(fv, lone_trio):
    batch = fv[1](TRIO)
    batch.solve()
    assert batch.errors == {}
    for q, (b, s) in enumerate(zip(batch.solvers, lone_trio)):
        _assert_same_trial(b, s, q)
        assert not s.accelerated or np.array_equal(b.t["astate"].cpu().numpy(), s.t["astate"].cpu().numpy())
    assert list(lone_trio[0].t["astate"].cpu().numpy()) == [3, (40 - 2) % 3, 40, 0]
    assert list(lone_trio[1].t["astate"].cpu().numpy()) == [0, 0, 0, 0]            # alone: the plain launch
    assert list(batch.solvers[1].t["astate"].cpu().numpy()) == [0, 0, 40, 0]        # in the batch: depth 0
    batch.close()


# ------------------------------------------------------------------------------------------- (e) convergence
@pytest.fixture(scope="module")
def restated_16():
    """max|du|, max|dv| between the restatement's plain and depth-5 runs at 16 x 16, Re = 100, tolerance 1e-6."""
    plain, acc = FVState(16, 16, 100.0), FVState(16, 16, 100.0)
    rp, _ = AA.run(plain, 20000, depth=0, tol=1e-6)
    ra, _ = AA.run(acc, 20000, depth=5, start=10, tol=1e-6)
    return len(rp), len(ra), float(np.max(np.abs(plain.u - acc.u))), float(np.max(np.abs(plain.v - acc.v)))


def test_acceleration_halves_the_iterations_at_16(fv, restated_16):
    """The YAML's settings.  At most 0.5 x the plain run's iterations (the restatement: 0.23; the factor 2 is for the
    sensitivity of the mixed path to rounding), and fields within 4 x what the restatement's two runs differ by."""
    common = dict(YAML, nx=16, ny=16, Re=100.0, tolerance=1e-6, max_iterations=20000, check_every=256)
    plain = fv[0](**common)                                 # acceleration="none": the launch of before
    acc = fv[0](**dict(common, acceleration="anderson"))    # depth 5 from iteration 10
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


# ------------------------------------------------------------------------------------------- (f) fallback, sequencing
def test_a_lid_at_rest_counts_its_fallbacks(fv):
    """8 x 8, depth 3 from iteration 2, the lid at rest: f = 0, so every Gram matrix is 0 and its first pivot is 0.  The
    lid's PROFILE is zeroed at lid velocity 1: the viscosity rho U L / Re of a lid velocity 0 is 0, which ldc_fv_create
    refuses.  As the restatement: a fallback at iterations 3 ... 10, the latch at the warm-up (iteration 11)."""
    s = fv[0](**dict({**YAML, **ANDERSON}, nx=8, ny=8, Re=100.0, anderson_depth=3, tolerance=1e-6, max_iterations=200,
                     check_every=16))
    s.t["ulid"].zero_()
    s.solve()
    c, st = s.counters(), s.state()
    print("lid at rest:", c, list(s.t["astate"].cpu().numpy()))
    assert s.metrics.converged and c["iterations"] == 11 and c["nan"] == 0
    assert c["anderson_fallbacks"] == 8 and list(s.t["astate"].cpu().numpy()) == [0, 0, 11, 8]
    assert np.all(np.isfinite(s.history[:, :4])) and all(np.all(st[k] == 0.0) for k in STATE)
    s.close()


def test_an_accelerated_sequence_is_the_same_steps_done_by_hand(fv):
    """solver=fv/fsg with acceleration=anderson, 16 -> 32: the levels inherit the parameters."""
    FVSolver, _, FVFSGSolver, prolong = fv
    common = dict(YAML, nx=32, ny=32, Re=100.0, tolerance=1e-5, max_iterations=20000, check_every=256,
                  acceleration="anderson")
    seq = FVFSGSolver(**dict(common, name="fv_fsg"))
    seq.solve()
    coarse = FVSolver(**dict(common, nx=16, ny=16))
    coarse.solve()
    fine = FVSolver(**common)
    prolong([(coarse, fine)])
    fine.solve()
    print("iterations per level", seq.level_iterations, "counters", seq.counters())
    assert seq.metrics.converged and [coarse.metrics.iterations, fine.metrics.iterations] == seq.level_iterations
    assert coarse.accelerated and fine.accelerated
    _assert_same_trial(seq, fine, "by hand")
    seq.close(), coarse.close(), fine.close()
