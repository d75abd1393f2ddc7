"""CPU checks of the chunk driver shared by lone solvers, batches and FSG ladders (solvers/spectral/chunks.py, fsg.run_ladder):
fake trials keep ctrl / sync / rec as CPU tensors and a fake enqueue advances ctrl and writes record rows."""
from types import SimpleNamespace

import pytest
import torch

from solvers.spectral import chunks
from solvers.spectral import ldc_lib as L
from solvers.spectral.fsg import run_ladder

DONE, ITER = L.CTRL_DONE, L.CTRL_ITER


class Trial:
    """What chunks needs of an SGSolver.  ``latch``: (iteration, code) at which the fake kernel latches."""

    def __init__(self, rec_cap=8, tail=False, latch=None):
        self.rec_cap = rec_cap
        self.d = {"ctrl": torch.zeros(L.CTRL_LEN, dtype=torch.int32), "sync": torch.zeros(L.SYNC_LEN, dtype=torch.int32),
                  "rec": torch.zeros((rec_cap, L.REC_LEN), dtype=torch.float64)}
        self._edge_fix_pending = tail
        self.latch = latch
        self.edge_fixes = []                   # iteration count at each rewrite of the index-(M-1) edges

    def _sync(self):
        pass

    def _write_boundary_edges(self, names):
        assert names == ("U", "UT", "V", "VT")
        self.edge_fixes.append(int(self.d["ctrl"][ITER]))


class Handle:
    """A fake handle: ``enqueue`` advances every unlatched trial; ``calls`` keeps the n_iters of every enqueue."""

    def __init__(self, trials, mode=0, device_index=0):
        self.trials, self.mode, self.dev = trials, mode, device_index
        self.calls, self.locked = [], []

    def enqueue(self, n_iters, diagnostics):
        self.calls.append(n_iters)
        self.locked.append(L.resident_lock(self.dev).locked())
        for t in self.trials:
            ctrl = t.d["ctrl"]
            for _ in range(n_iters):
                if int(ctrl[DONE]):
                    break
                it = int(ctrl[ITER])
                t.d["rec"][it % t.rec_cap] = float(it)
                ctrl[ITER] = it + 1
                if t.latch and it + 1 == t.latch[0]:
                    ctrl[DONE] = t.latch[1]

    def step(self, k):
        return chunks.advance(self.trials, k, False, self.enqueue, self.mode, self.dev)

    def lone_step(self, k):                    # SGSolver._advance: a lone solver's chunk, unwrapped and wrapped again
        return [self.step(k)[0]]


def iterations(rows):
    return rows[:, 0].astype(int).tolist()


# ---------------------------------------------------------------------------------------------------- n_iters sequences
def test_lone_solve_carves_the_first_iteration_off_its_first_chunk():
    t = Trial(rec_cap=8, tail=True)
    h = Handle([t])
    (latch, its, rows), = chunks.run_to_tolerance([t], h.lone_step, [30], batch=False)
    assert h.calls == [1, 7, 8, 8, 6]
    assert (latch, its) == (chunks.LATCH_CAPPED, 30) and iterations(rows) == list(range(30))
    assert int(t.d["ctrl"][DONE]) == 0                         # a lone solve never writes LATCH_CAPPED
    assert t.edge_fixes == [1] and not t._edge_fix_pending


def test_lone_run_iterations_carves_the_first_iteration_off_its_first_chunk():
    t = Trial(rec_cap=8, tail=True)
    h = Handle([t])
    rows, = chunks.run_iterations([t], h.lone_step, 20, batch=False)
    assert h.calls == [1, 7, 8, 4] and iterations(rows) == list(range(20))
    h.calls.clear()
    rows, = chunks.run_iterations([t], h.lone_step, 5, batch=False)
    assert h.calls == [5] and iterations(rows) == list(range(20, 25))


def test_lone_chunk_is_cut_to_the_record_ring():
    t = Trial(rec_cap=8, tail=True)
    h = Handle([t])
    rows, latch, end = h.step(100)[0]
    assert h.calls == [1, 7] and (latch, end) == (0, 8) and iterations(rows) == list(range(8))


def test_batch_runs_the_first_iteration_as_a_chunk_of_its_own_and_latches_caps():
    ts = [Trial(tail=True) for _ in range(3)]
    h = Handle(ts, mode=3)
    out = chunks.run_to_tolerance(ts, h.step, [5, 20, 13], batch=True)
    assert h.calls == [1, 4, 8, 7]                            # each chunk shortened to the smallest live cap
    assert [(d, n) for d, n, _ in out] == [(chunks.LATCH_CAPPED, 5), (chunks.LATCH_CAPPED, 20), (chunks.LATCH_CAPPED, 13)]
    assert [iterations(r) for _, _, r in out] == [list(range(5)), list(range(20)), list(range(13))]
    assert [int(t.d["ctrl"][DONE]) for t in ts] == [chunks.LATCH_CAPPED] * 3
    assert [int(t.d["ctrl"][ITER]) for t in ts] == [5, 20, 13]
    assert all(t.edge_fixes == [1] for t in ts)


def test_batch_run_iterations_runs_the_first_iteration_alone_then_full_chunks():
    ts = [Trial(tail=True), Trial(tail=True)]
    h = Handle(ts)
    rows = chunks.run_iterations(ts, h.step, 20, batch=True)
    assert h.calls == [1, 8, 8, 3]
    assert [iterations(r) for r in rows] == [list(range(20))] * 2
    assert [int(t.d["ctrl"][DONE]) for t in ts] == [0, 0]      # run_iterations latches nothing


@pytest.mark.parametrize("batch", [False, True])
def test_without_an_edge_fix_every_loop_enqueues_plain_chunks(batch):
    ts = [Trial()] if not batch else [Trial(), Trial()]
    h = Handle(ts)
    step = h.step if batch else h.lone_step
    chunks.run_to_tolerance(ts, step, [20] * len(ts), batch=batch)
    assert h.calls == [8, 8, 4]
    for t in ts:
        t.d["ctrl"].zero_()
    h.calls.clear()
    chunks.run_iterations(ts, step, 19, batch=batch)
    assert h.calls == [8, 8, 3]
    assert all(t.edge_fixes == [] for t in ts)


# ---------------------------------------------------------------------------------------------------- latches
def test_a_latched_trial_leaves_the_batch_the_others_go_on():
    ts = [Trial(latch=(30, 1)), Trial(), Trial(latch=(3, 2))]
    h = Handle(ts)
    out = chunks.run_to_tolerance(ts, h.step, [40, 20, 40], batch=True)
    assert [(d, n) for d, n, _ in out] == [(1, 30), (chunks.LATCH_CAPPED, 20), (2, 3)]
    assert h.calls == [8, 8, 4, 8, 8]                         # up to cap 20, then chunks until the last latch
    assert [len(r) for _, _, r in out] == [30, 20, 3]
    assert [int(t.d["ctrl"][DONE]) for t in ts] == [1, chunks.LATCH_CAPPED, 2]


def test_lone_run_iterations_stops_at_the_latch():
    t = Trial(latch=(10, 2))
    h = Handle([t])
    rows, = chunks.run_iterations([t], h.lone_step, 50, batch=False)
    assert h.calls == [8, 8] and iterations(rows) == list(range(10))


def test_lone_first_iteration_that_latches_ends_the_chunk():
    t = Trial(tail=True, latch=(1, 2))
    h = Handle([t])
    rows, latch, end = h.step(8)[0]
    assert h.calls == [1] and (latch, end) == (2, 1) and t.edge_fixes == [1]


def test_a_barrier_give_up_raises():
    ts = [Trial(), Trial()]
    ts[1].d["sync"][L.SYNC_GIVEUP] = 1
    with pytest.raises(L.LdcError, match="gave up a barrier wait"):
        Handle(ts, mode=5).step(4)


# ---------------------------------------------------------------------------------------------------- lock and gathers
@pytest.mark.parametrize("mode,n,locked", [(0, 8, False), (3, 8, True), (4, 8, True), (5, 8, True), (5, 1, False)])
def test_resident_lock_around_co_resident_chunks(mode, n, locked):
    h = Handle([Trial()], mode=mode, device_index=3)
    h.step(n)
    assert h.locked == [locked] and not L.resident_lock(3).locked()


@pytest.mark.parametrize("caps,stacks", [((8, 8, 8), 4), ((8, 16, 8), 3)])
def test_one_gather_per_kind_of_word_and_chunk(monkeypatch, caps, stacks):
    """ctrl before and after, the give-up words, and the rings when every ring has the same length."""
    ts = [Trial(rec_cap=c) for c in caps]
    count = []
    real = torch.stack
    monkeypatch.setattr(torch, "stack", lambda xs, *a, **k: count.append(len(xs)) or real(xs, *a, **k))
    Handle(ts).step(8)
    assert count == [3] * stacks


# ---------------------------------------------------------------------------------------------------- FSG ladder
class Level(SimpleNamespace):
    def reset_state(self):
        self.start = "rest"

    def close(self):
        self.closed = True


class Fine(Level):
    """What run_ladder needs of an FSGSolver (trial ``q``)."""

    def __init__(self, q, nx=64, n_levels=3, factor=10.0):
        super().__init__(params=SimpleNamespace(nx=nx, n_levels=n_levels, coarse_tolerance_factor=factor), N=nx, q=q)
        self.smoother, self.levels = False, []

    def _smoother_mode(self):
        self.smoother = True

    def _make_level(self, n):
        self.levels.append(Level(N=n, q=self.q))
        return self.levels[-1]

    def _prolongate(self, coarse, fine):
        fine.start = coarse.N

    def _finish(self, tolerance, total, converged, wall):
        self.finished = (tolerance, total, converged)


def test_ladder_drops_a_diverged_trial_and_stops_when_none_is_left():
    fines = [Fine(0), Fine(1), Fine(2)]
    seen = []
    latch = {(16, 0): 1, (16, 1): 2, (16, 2): 1, (32, 0): 1, (32, 2): 2, (64, 0): chunks.LATCH_CAPPED}

    def run_level(group, tols, caps):
        seen.append(([g.N for g in group], [g.q for g in group], tols, caps))
        return [(latch[(g.N, g.q)], g.N, None) for g in group]

    run_ladder(fines, run_level, [1e-6, 1e-5, 1e-6], [100, 200, 300])
    assert [s[:2] for s in seen] == [([16, 16, 16], [0, 1, 2]), ([32, 32], [0, 2]), ([64], [0])]
    assert seen[0][2] == pytest.approx([1e-4, 1e-3, 1e-4]) and seen[1][2] == pytest.approx([1e-5, 1e-5])
    assert seen[1][3] == [100, 300] and seen[2][3] == [100]
    assert all(f.smoother for f in fines) and fines[0].levels[0].start == "rest" and fines[0].levels[1].start == 16
    assert fines[0].start == 32
    assert fines[0].finished == (1e-6, 16 + 32 + 64, False)   # capped on the fine level
    assert fines[1].finished == (1e-5, 16, False)             # diverged on the coarsest level
    assert fines[2].finished == (1e-6, 16 + 32, False)        # diverged on the middle level
    assert all(lvl.closed for f in fines for lvl in f.levels) and not hasattr(fines[0], "closed")


def test_ladder_runs_no_empty_level():
    fines = [Fine(0, nx=32, n_levels=2)]
    calls = []

    def run_level(group, tols, caps):
        calls.append(len(group))
        return [(2, 5, None)]

    run_ladder(fines, run_level, [1e-6], [50])
    assert calls == [1] and fines[0].finished == (1e-6, 5, False)


def test_ladder_converged_on_every_level():
    fines = [Fine(0, nx=32, n_levels=2)]
    run_ladder(fines, lambda g, t, c: [(1, 7, None)], [1e-6], [50])
    assert fines[0].finished == (1e-6, 14, True)
