"""The retry loop of the whole-chip mappings: iterations that carry fixed numbers of launches, enqueued again with twice the
budget when a solve needs more.

A ``mapping="chip"`` or ``"shared"`` iteration carries ``linear_budget`` BiCGSTAB iterations per momentum solve and, with
``pressure_equation="consistent"``, ``pressure_budget`` CG iterations of the pressure solve.  An iteration that needs more
changes nothing and says which budget ran out in the overflow word (include/ldc_fv.h): ``advance_with_retries`` is the one
loop that doubles that budget and enqueues what is left, for a lone trial (a batch of one) and for the trials of a shared
batch, with one budget or two.  ``advance_with_budget``, ``advance_batch_with_budget``, ``advance_with_budgets`` and
``advance_batch_with_budgets`` are that loop under the signatures it grew from."""
from __future__ import annotations

import numpy as np

from . import ldc_fv_lib as F

KINDS = ("linear", "pressure")      # overflow word w names budget w - 1: F.OVERFLOW_LINEAR = 1, F.OVERFLOW_PRESSURE = 2
assert (F.OVERFLOW_LINEAR, F.OVERFLOW_PRESSURE) == (1, 2)


def advance_with_retries(step, starts, ks, budgets, caps):
    """Trial q stands at iteration ``starts[q]`` and is to do ``ks[q]`` more (0: it is left alone), whatever budgets they
    need: ``budgets[q]`` is a tuple with one entry per cap, ``caps`` = (max_lin_iters,) or (max_lin_iters,
    pressure_max_iters), where the kernel accepts a solve that has not converged, so it cannot overflow.

    ``step(quotas, *call_budgets)`` enqueues up to ``quotas[q]`` iterations of every trial in the same launches, waits, and
    returns per trial (rows of the iterations it completed, latch, nan, iteration count, overflow).  The first call carries
    every trial with ``ks[q] > 0``, and a call carries the largest budget of each kind among its trials.  Overflow word ``w``
    in 1 ... ``len(caps)`` means: the iteration after the last completed one needs more than the call's budget ``w - 1`` and
    has changed nothing.  That trial's own budget of the kind becomes twice the CALL's, at most its cap, and it is enqueued
    again with what is left of its count, beside the others that overflowed and with quota 0 for everyone else; and so on
    until nobody overflows.  A trial that needed no more keeps its budgets.  Returns per trial (rows, latch, nan, iteration
    count, budgets now, retries per budget): no iteration is lost or counted twice."""
    n = len(starts)
    starts = [int(x) for x in starts]
    totals, budgets, retries = list(starts), [[int(b) for b in bq] for bq in budgets], [[0] * len(caps) for _ in range(n)]
    blocks, flags = [[] for _ in range(n)], [(0, 0)] * n
    todo = [q for q in range(n) if ks[q] > 0]
    while todo:
        quotas = [0] * n
        for q in todo:
            quotas[q] = int(ks[q]) - (totals[q] - starts[q])
        call = [max(budgets[q][w] for q in todo) for w in range(len(caps))]
        out = step(list(quotas), *call)
        if len(out) != n:
            raise RuntimeError("one result per trial expected")
        again = []
        for q, (rows, latch, nan, new_total, overflow) in enumerate(out):
            if len(rows) != new_total - totals[q]:
                raise RuntimeError(f"trial {q}: {len(rows)} record rows for iterations {totals[q]} ... {new_total}")
            if quotas[q] == 0:
                if new_total != totals[q]:
                    raise RuntimeError(f"trial {q} had quota 0 and went from iteration {totals[q]} to {new_total}")
                continue
            blocks[q].append(rows)
            totals[q] = int(new_total)
            flags[q] = (int(latch), int(nan))
            if latch or nan:
                continue
            if overflow:
                if not 1 <= overflow <= len(caps):
                    raise RuntimeError(f"trial {q}: overflow word {overflow}")
                which = overflow - 1
                if call[which] >= caps[which]:
                    raise RuntimeError(f"trial {q}: {KINDS[which]} budget {call[which]} >= its cap {caps[which]} reported "
                                       f"an overflow")
                budgets[q][which] = min(2 * call[which], int(caps[which]))
                retries[q][which] += 1
                again.append(q)
            elif totals[q] - starts[q] < ks[q]:
                raise RuntimeError(f"trial {q}: device loop made no progress")
        todo = again
    return [(np.concatenate(b, axis=0) if b else np.zeros((0, F.REC_LEN)), latch, nan, total, tuple(bq), tuple(r))
            for b, (latch, nan), total, bq, r in zip(blocks, flags, totals, budgets, retries)]


advance_batch_with_budgets = advance_with_retries      # budgets[q] = (BiCGSTAB, CG), caps = (max_lin_iters, pressure_max_iters)


def advance_batch_with_budget(step, starts, ks, budgets, max_lin_iters):
    """One budget per trial: ``step(quotas, budget)``; per trial (rows, latch, nan, iteration count, budget now, retries)."""
    out = advance_with_retries(step, starts, ks, [(b,) for b in budgets], (max_lin_iters,))
    return [(rows, latch, nan, total, now[0], retries[0]) for rows, latch, nan, total, now, retries in out]


def advance_with_budgets(step, start, k, budgets, caps):
    """A lone trial, a batch of one: ``step(m, linear_budget, pressure_budget)`` returns the one tuple; (rows, latch, nan,
    iteration count, budgets now, retries per budget)."""
    return advance_with_retries(lambda quotas, *call: [step(quotas[0], *call)], [start], [k], [budgets], caps)[0]


def advance_with_budget(step, start, k, budget, max_lin_iters):
    """A lone trial with one budget: ``step(m, budget)``; (rows, latch, nan, iteration count, budget now, retries)."""
    return advance_batch_with_budget(lambda quotas, b: [step(quotas[0], b)], [start], [k], [budget], max_lin_iters)[0]
