"""Sequencing and continuation of wall-clustered finite-volume trials on the GPU (``grid="tanh"`` with ``transfer="tables"``
through FVFSGSolver, ``start_from`` and BatchedFVFSGSolver): the sequence 16^2 -> 32^2 against the figures of the NumPy
restatement (tests/fv_prolong_tables_numpy.py) and against the solve from rest, continuation in Re at equal grids, and a
batch that mixes such trials with uniform ones against their lone sequenced solves."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import fv_prolong_tables_numpy as T  # noqa: E402

pytestmark = pytest.mark.gpu

YAML = dict(convection_scheme="TVD", alpha_uv=0.4, alpha_p=0.2, linear_solver_tol=1e-9)      # conf/solver/fv.yaml
TANH = dict(grid="tanh", grid_stretch=1.5, transfer="tables", pressure_equation="consistent_cu",
            pressure_preconditioner="separable")
FLAGSHIP = dict(YAML, **TANH, nx=32, ny=32, Re=100.0, tolerance=1e-6, max_iterations=20000, check_every=512)
STATE = ("u", "v", "p", "mdot")


@pytest.fixture(scope="module")
def fv():
    import __graft_entry__ as g
    g.build()
    from solvers.fv.batched import BatchedFVFSGSolver
    from solvers.fv.fsg import FVFSGSolver
    from solvers.fv.solver import FVSolver
    return FVSolver, FVFSGSolver, BatchedFVFSGSolver


def _assert_same_trial(a, b, what):
    assert a.metrics.iterations == b.metrics.iterations and a.metrics.converged == b.metrics.converged, what
    assert a.history.shape == b.history.shape and np.array_equal(a.history, b.history), what
    sa, sb = a.state(), b.state()
    for k in STATE:
        assert np.array_equal(sa[k], sb[k]), (what, k)


def test_the_stretched_sequence_latches_and_ends_where_the_solve_from_rest_ends(fv):
    """n_levels = 2, coarsest_n = 16.  The level counts are the restatement's to within one iteration, and the fine fields
    differ from the lone run's by at most twice what the two runs of the restatement differ by (both stop on a rate-bound rule;
    tests/test_fv_prolong_tables_cpu.py checks those figures): the margin tests/fv_prolong_numpy.py gives SEQ_16_32_*."""
    FVSolver, FVFSGSolver, _ = fv
    s = FVFSGSolver(name="fv_fsg", n_levels=2, coarsest_n=16, **FLAGSHIP)
    assert s.level_sizes() == [(16, 16), (32, 32)]
    s.solve()
    lone = FVSolver(name="fv", **FLAGSHIP)
    lone.solve()
    a, b = s.state(), lone.state()
    duv = max(float(np.max(np.abs(a[k] - b[k]))) for k in ("u", "v"))
    dp = float(np.max(np.abs(a["p"] - b["p"])))
    print("iterations per level", s.level_iterations, "restatement", T.SEQ_16_32_ITERS, "from rest", lone.metrics.iterations,
          "restatement", T.SEQ_16_32_LONE_ITERS, " max |du|, |dv|:", duv, " max |dp|:", dp)
    assert s.metrics.converged and lone.metrics.converged and s.metrics.final_residual < 1e-6
    assert s.level_sizes() == [(16, 16), (32, 32)] and len(s.level_iterations) == 2
    assert s.metrics.iterations == s.level_iterations[1] == len(s.history)
    assert all(abs(got - want) <= 1 for got, want in zip(s.level_iterations, T.SEQ_16_32_ITERS))
    assert 0 < duv <= 2 * T.SEQ_16_32_DUV and 0 < dp <= 2 * T.SEQ_16_32_DP
    assert s.history[0, 0] < lone.history[0, 0]
    s.close(), lone.close()


def test_continuation_in_re_on_equal_stretched_grids(fv):
    FVSolver, FVFSGSolver, _ = fv
    common = dict(YAML, **TANH, nx=32, ny=32, tolerance=1e-5, max_iterations=20000, check_every=256)
    a = FVSolver(name="fv", Re=100.0, **common)
    a.solve()
    rest = FVSolver(name="fv", Re=400.0, **common)
    rest.solve()
    b = FVFSGSolver(name="fv_fsg", Re=400.0, **common)
    b.start_from(a)
    st, src = b.state(), a.state()
    assert np.array_equal(st["u"], src["u"]) and np.array_equal(st["v"], src["v"])      # equal grids: the identity
    assert np.array_equal(st["p"], src["p"] - src["p"][0]) and b.level_sizes() == [(32, 32)]
    b.solve()
    print("Re 100 from rest:", a.metrics.iterations, "; Re 400 from rest:", rest.metrics.iterations, "first residual",
          rest.history[0, 0], "; Re 400 from Re 100:", b.level_iterations, "first residual", b.history[0, 0])
    assert a.metrics.converged and rest.metrics.converged
    assert b.metrics.converged and b.level_iterations == [b.metrics.iterations]
    assert b.history[0, 0] < rest.history[0, 0]
    assert b.level_sizes() == [(16, 16), (32, 32)]        # the start is used up: the next solve is the whole sequence
    # ... and a plain FVSolver continues the same way, from a uniform source too
    u = FVSolver(name="fv", Re=100.0, **dict(YAML, nx=24, ny=24, tolerance=1e-4, max_iterations=20000, check_every=256))
    u.solve()
    d = FVSolver(name="fv", Re=100.0, **common)
    d.start_from(u)
    assert np.all(np.isfinite(d.state()["u"])) and d.state()["p"][0] == 0.0
    d.solve()
    assert d.metrics.converged and d.history[0, 0] < a.history[0, 0]
    for s in (a, rest, b, u, d):
        s.close()


def test_a_batch_of_stretched_and_uniform_sequences_equals_lone_ones(fv):
    """Two tanh trials with ``transfer="tables"`` (16 -> 32, and 13 x 17 that cannot halve) and two uniform ones with the
    default (16 -> 32, and 20 x 24 alone) in ONE batch: the stage's single ``prolong`` call splits by route."""
    _, FVFSGSolver, Batched = fv
    common = dict(YAML, name="fv_fsg", tolerance=1e-5, max_iterations=20000, check_every=256)
    trials = [dict(common, **TANH, nx=32, ny=32, Re=100.0),
              dict(common, **TANH, nx=13, ny=17, Re=100.0, corner_treatment="smoothing"),
              dict(common, nx=32, ny=32, Re=400.0),
              dict(common, nx=20, ny=24, Re=100.0)]
    batch = Batched(trials)
    assert [s.level_sizes() for s in batch.solvers] == [[(16, 16), (32, 32)], [(13, 17)], [(16, 16), (32, 32)], [(20, 24)]]
    assert [s.transfer_tables for s in batch.solvers] == [True, True, False, False]
    batch.solve()
    assert batch.errors == {}
    for q, t in enumerate(trials):
        lone = FVFSGSolver(**t)
        lone.solve()
        print(q, "iterations per level", lone.level_iterations)
        assert lone.metrics.converged and batch.solvers[q].level_iterations == lone.level_iterations
        assert len(lone.level_iterations) == (2, 1, 2, 1)[q]
        _assert_same_trial(batch.solvers[q], lone, q)
        lone.close()
    batch.close()
