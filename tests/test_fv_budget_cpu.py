"""The one retry loop of solvers/fv/budget.py where its four wrappers do not reach: trials that do not start at 0, a trial
that runs out of both budgets in one chunk, a waiting trial whose larger budgets stay out of the calls, and the overflow
words a loop with one cap accepts.  (The wrappers' own tests: test_fv_wide_cpu.py, test_fv_shared_cpu.py,
test_fv_pressure_cpu.py.)"""
import numpy as np
import pytest


class FakeTrial:
    """A trial at iteration ``start`` whose next iterations need ``lin[i]`` BiCGSTAB and ``cg[i]`` CG iterations.  An enqueue
    completes iterations until one needs more than a budget (overflow 1: BiCGSTAB, which comes first; 2: CG; that iteration
    has changed nothing) or all it was given.  Row i holds the iteration's number."""

    def __init__(self, start, lin, cg):
        self.start, self.total, self.lin, self.cg = start, start, list(lin), list(cg)

    def step(self, m, lin_budget, cg_budget):
        rows, overflow = [], 0
        for _ in range(m):
            i = self.total - self.start
            if lin_budget < self.lin[i]:
                overflow = 1
                break
            if cg_budget < self.cg[i]:
                overflow = 2
                break
            rows.append([float(self.total)] * 8)
            self.total += 1
        return np.array(rows).reshape(-1, 8), 0, 0, self.total, overflow


def test_three_trials_two_budgets_both_kinds_in_one_call_and_one_trial_waiting():
    from solvers.fv.budget import advance_with_retries
    trials = [FakeTrial(10, lin=[3, 20, 3], cg=[10, 10, 60]), FakeTrial(0, lin=[3, 3, 3], cg=[10, 40, 10]),
              FakeTrial(5, lin=[], cg=[])]
    calls = []

    def step(quotas, lin_budget, cg_budget):
        calls.append((list(quotas), lin_budget, cg_budget))
        return [t.step(k, lin_budget, cg_budget) for t, k in zip(trials, quotas)]

    out = advance_with_retries(step, [10, 0, 5], [3, 3, 0], [(4, 24), (4, 24), (6, 30)], (1000, 200))
    # call 1: trial 0 runs out of BiCGSTAB and trial 1 of CG, each before its second iteration; trial 1 is done in call 2;
    # trial 0 doubles the CALL's linear budget until 32, then runs out of CG before its third iteration, twice.  The
    # waiting trial's (6, 30) never enters a call's maximum
    assert calls == [([3, 3, 0], 4, 24), ([2, 2, 0], 8, 48), ([2, 0, 0], 16, 24), ([2, 0, 0], 32, 24), ([1, 0, 0], 32, 48),
                     ([1, 0, 0], 32, 96)]
    assert [o[1:4] for o in out] == [(0, 0, 13), (0, 0, 3), (0, 0, 5)]
    assert [o[4] for o in out] == [(32, 96), (4, 48), (6, 30)] and [o[5] for o in out] == [(3, 2), (0, 1), (0, 0)]
    assert out[0][0][:, 0].tolist() == [10, 11, 12] and out[1][0][:, 0].tolist() == [0, 1, 2]      # once each, in order
    assert out[2][0].shape == (0, 8)


def test_an_overflow_word_names_one_of_the_loops_own_budgets():
    from solvers.fv.budget import advance_with_budget, advance_with_retries
    none = np.zeros((0, 8))
    with pytest.raises(RuntimeError, match="overflow word 2"):       # one cap: only word 1 names a budget
        advance_with_retries(lambda quotas, b: [(none, 0, 0, 0, 2)], [0], [2], [(4,)], (10,))
    with pytest.raises(RuntimeError, match="overflow word"):
        advance_with_budget(lambda m, b: (none, 0, 0, 0, 2), 0, 2, 4, 10)
    with pytest.raises(RuntimeError, match="overflow word 3"):
        advance_with_retries(lambda quotas, a, b: [(none, 0, 0, 0, 3)], [0], [2], [(4, 4)], (10, 10))
    with pytest.raises(RuntimeError, match="linear budget 10 >= its cap 10"):
        advance_with_retries(lambda quotas, b: [(none, 0, 0, 0, 1)], [0], [2], [(10,)], (10,))
