"""Batched finite-volume trials: independent FV solves advanced by the same launches, one work-group (one CU) each.

The reference's only parallel axis is the trial (conf/machine/local.yaml:5-9, scripts/hpc_submit.py:103-107).  An FV
trial is ONE work-group for its whole life (include/ldc_fv.h), so a lone trial uses 1/256 of an MI355X;
``ldc_fv_batch_enqueue`` launches up to ``LDC_FV_LAUNCH_MAX`` = 256 of them per launch, of ANY sizes and parameters.
The work-groups never wait for each other (no flags, no spins, no co-residency among them), and the kernel
keeps no state between launches other than the trial's own arrays, with reductions in a fixed order.  So every trial's
fields, record rows, iteration count, latch and counters are bit-identical to its lone ``FVSolver.solve()``, whatever
else is in the batch and wherever the chunk boundaries fall (tests/test_gpu_fv_batched.py).

An FV work-group needs nobody, but it HOLDS its CU for a whole chunk (175 VGPRs x 8 waves: nothing of the spectral
kernels' co-resident work-groups fits beside it), and the spectral kernels of modes 3, 4 and 5 need all their
work-groups resident at once and give up after a bounded spin.  So every FV chunk runs under the device's
``ldc_lib.resident_lock``, like those launches do: in a mixed sweep an FV chunk and a co-resident spectral chunk take
turns, while launch-path spectral batches of other streams still run beside either.

Trials that are all ``mapping="shared"`` are one batch object of the library instead (``solver.SharedBatch``,
``ldc_fv_wide_batch_*``): every phase of the iteration is ONE launch that carries the work-groups of all trials, min(256,
cells / 256) each, so a handful of trials already spreads over the chip where the one-CU mapping would leave it idle.
A trial is the same launches' work alone and in a batch: its results are bit-identical to its lone ``mapping="chip"``
or ``"shared"`` solve.  A chunk hands every live trial a quota of iterations and everyone else quota 0, so finished
trials stay in the batch object and cost empty work-groups; a trial whose momentum solves need more BiCGSTAB launches
than the chunk carried is enqueued again on its own with twice the budget (``budget.advance_with_retries``).

``BatchedFVFSGSolver`` is the same for coarse-to-fine sequences (solvers.fv.fsg): stage by stage, every stage a batch of
ordinary trials, one ``prolong`` call between stages, which splits its pairs by route: ``grid="tanh"`` trials with
``transfer="tables"`` ride beside uniform ones.  A trial with ``chip_transfer="tables"`` is a lone chip trial: both batch
classes refuse it by name.
"""
from __future__ import annotations

import logging
import time

import numpy as np

from ..base import WARMUP_ITERATIONS
from . import ldc_fv_lib as F
from .fsg import FVFSGSolver, level_tolerance
from .solver import WALL_RULES, FVSolver, SharedBatch, advance, device_index, postprocess, prolong

log = logging.getLogger(__name__)


def run_chunks(rec_caps, caps, step):
    """Every trial from iteration 0 to ITS latch, ITS cap or a NaN, chunk by chunk; per-trial (latch, nan, iterations,
    record rows).

    ``step(live, k)`` advances the trials ``live`` (indices, ascending) by up to ``k`` iterations in one launch and
    returns, in the same order, (rows of the new iterations, latch, nan, iteration count).  A trial that latched, went
    NaN or reached its cap leaves the live list and is never passed to ``step`` again: its work-group is not launched
    at all (the spectral batches latch such a trial on the device instead, chunks.LATCH_CAPPED).  All trials start at 0,
    so the live ones are in step, and a chunk is as long as the smallest record ring and the smallest remaining cap
    among them allow."""
    n = len(caps)
    state = [(0, 0, 0)] * n                   # (latch, nan, iterations)
    blocks = [[] for _ in range(n)]
    live = [q for q in range(n) if caps[q] > 0]
    it = 0
    while live:
        k = min(min(rec_caps[q] for q in live), min(caps[q] for q in live) - it)
        out = step(list(live), k)
        if len(out) != len(live):
            raise RuntimeError("one result per live trial expected")
        for q, (rows, latch, nan, total) in zip(live, out):
            if total == it and not (latch or nan):
                raise RuntimeError("device loop made no progress")
            blocks[q].append(rows)
            state[q] = (int(latch), int(nan), int(total))
        it += k
        live = [q for q in live if not (state[q][0] or state[q][1]) and state[q][2] < caps[q]]
    return [(latch, nan, total, np.concatenate(b, axis=0) if b else np.zeros((0, F.REC_LEN)))
            for (latch, nan, total), b in zip(state, blocks)]


class BatchedFVSolver:
    """``trials``: list of FVSolver keyword dicts, all on one device.  They need not share nx / ny, scheme,
    relaxation, lid treatment, tolerance, ``max_iterations`` or ``check_every``: the kernel takes any mix.

    ``solve()`` fills every solver's history / metrics / fields as its lone ``solve()`` would; called again, it goes
    on from the fields the trials hold, counting from 0 with a new warm-up, as a lone repeat solve does.  A trial whose
    kernel reports a NaN ends as a lone run ends -- with the ``LdcError`` of ``ldc_fv_status`` -- but here the exception
    is kept in ``errors[index]`` instead of raised, and the other trials are not disturbed."""

    Solver = FVSolver
    _shares_launches = True                   # mapping="shared" trials are taken (as one batch object of the library)

    def __init__(self, trials: list):
        if not trials:
            raise ValueError(f"{type(self).__name__} needs at least one trial")
        for t in trials:
            if t.get("chip_transfer", "uniform") != "uniform":
                raise ValueError(f"chip_transfer={t['chip_transfer']!r} inside a batch: the transfer over the whole chip "
                                 f"starts a lone mapping='chip' trial, run it on its own")
            if t.get("mapping", "cu") == "chip":
                raise ValueError("mapping='chip' inside a batch: a chip trial takes every CU, run it on its own")
        maps = {t.get("mapping", "cu") for t in trials}
        if "shared" in maps and not self._shares_launches:
            raise ValueError(f"mapping='shared' in a {type(self).__name__}: sequenced trials do not share their launches "
                             f"yet, run them one by one or with mapping='cu'")
        if "shared" in maps and maps != {"shared"}:
            raise ValueError(f"mapping='shared' beside mapping={sorted(maps - {'shared'})[0]!r} in one batch: the trials "
                             f"of a batch either share every launch or have a CU each")
        if "shared" in maps and len(trials) > F.WIDE_BATCH_MAX:
            raise ValueError(f"{len(trials)} mapping='shared' trials in one batch: at most {F.WIDE_BATCH_MAX}")
        self.solvers, self.shared = [], None
        try:
            for t in trials:
                self.solvers.append(self.Solver(**t))
        except BaseException:                 # the handles of the trials already built
            self.close()
            raise
        devs = {(s.device.type, device_index(s.device)) for s in self.solvers}
        if len(devs) != 1:
            self.close()
            raise ValueError(f"all trials of a batch must be on one device, got {sorted(devs)}")
        if maps == {"shared"}:
            try:
                self.shared = SharedBatch(self.solvers)       # one batch object for the life of this one
            except BaseException:
                self.close()
                raise
        self.errors = {}
        self.batch_seconds, self.batch_size = 0.0, len(self.solvers)

    def __len__(self):
        return len(self.solvers)

    def close(self):
        if getattr(self, "shared", None) is not None:
            self.shared.close()
            self.shared = None
        for s in self.solvers:
            s.close()

    def set_wide_graph(self, on: bool):
        """The launches of a batch of ``"shared"`` trials: one replayed hipGraph per iteration or every kernel on its own
        (``FVSolver.set_wide_graph`` for the batch object)."""
        if self.shared is None:
            raise ValueError("set_wide_graph: only a batch of mapping='shared' trials has launches to capture")
        self.shared.set_graph(on)

    def _step(self, live, k):
        """One chunk of the live trials (solver.advance: one launch, one copy of the ctrl words, one of the rows).

        ``"shared"`` trials: quota ``k`` for the live ones and 0 for the others, in the launches of the one batch object;
        back only when every live trial has done ``k`` iterations, latched or gone NaN (``SharedBatch.advance``)."""
        if self.shared is not None:
            out = self.shared.advance([k if q in live else 0 for q in range(len(self.solvers))])
            return [out[q] for q in live]
        return advance([self.solvers[q] for q in live], k)

    def solve(self, max_iter: int = None):
        """Every trial to its own tolerance or its own ``max_iterations`` (``max_iter``: one cap for all).

        Only the batch has a wall time of its own (``batch_seconds``).  A trial's ``metrics.wall_time_seconds`` is
        its share of it in proportion to its work, iterations x nx x ny; the shares of the trials that finished add
        up to ``batch_seconds``.  No live MLflow metrics per chunk, as in the spectral batches.  Returns the trials'
        metrics in order, None for a trial listed in ``errors`` (its solver keeps the metrics it was built with)."""
        ps = [s.params for s in self.solvers]
        caps = [int(p.max_iterations if max_iter is None else max_iter) for p in ps]
        for s, p in zip(self.solvers, ps):
            s._begin(p.tolerance)             # control words to zero: every trial counts from 0 on its current fields
        self.errors = {}
        t0 = time.perf_counter()
        out = run_chunks([s.rec_cap for s in self.solvers], caps, self._step)
        wall = time.perf_counter() - t0
        self.batch_seconds, self.batch_size = wall, len(self.solvers)
        self._store(out, wall)
        log.info("batched solve of %d FV trials finished in %.2f s (%d stopped on a NaN)", len(self.solvers), wall,
                 len(self.errors))
        return [None if q in self.errors else s.metrics for q, s in enumerate(self.solvers)]

    @staticmethod
    def _nan_error(s, total):
        """What a lone _advance raises for a trial whose kernel reports a NaN (ldc_fv_status -> LDC_FV_E_NAN)."""
        try:
            if s.shared:                      # (a trial above 256 cells per axis has no one-CU handle to ask)
                F.check(F.lib().ldc_fv_wide_status(s._wide), f"FV trial at iteration {total}")
            else:
                F.check(F.lib().ldc_fv_status(s.handle), f"FV trial at iteration {total}")
            raise RuntimeError(f"FV trial at iteration {total}: ctrl reports a NaN, ldc_fv_status does not")
        except Exception as exc:
            return exc

    def _store(self, out, wall, extra_work=None):
        """History, metrics and fields of every trial from ``out`` (run_chunks' rows of ``self.solvers``, in order); a
        trial that stopped on a NaN, and one already in ``errors``, gets an error instead.  ``extra_work``: per trial,
        iterations x cells spent before (coarser levels), which count in its share of the wall time."""
        for q, (s, (_, nan, total, _)) in enumerate(zip(self.solvers, out)):
            if nan and q not in self.errors:
                self.errors[q] = self._nan_error(s, total)
        work = [0 if q in self.errors else total * s.nx * s.ny + (extra_work[q] if extra_work else 0)
                for q, (s, (_, _, total, _)) in enumerate(zip(self.solvers, out))]
        work_all = max(1, sum(work))
        # the device paths of the vortex metrics ("device", "chip" and the wall rules of streamfunction): every finished trial that asks for one in one go (_store_results below
        # finds its result block); a trial in `errors` is left alone
        postprocess([s for q, s in enumerate(self.solvers)
                     if q not in self.errors and (s.params.vortex_metrics in ("device", "chip") or s.params.streamfunction in WALL_RULES)])
        for q, (s, (done, _, total, hist)) in enumerate(zip(self.solvers, out)):
            if q in self.errors:
                continue
            s.history = hist
            s._store_results(hist[WARMUP_ITERATIONS:], total, done == 1, wall * work[q] / work_all)


class BatchedFVFSGSolver(BatchedFVSolver):
    """``trials``: list of FVFSGSolver keyword dicts, all on one device; sizes, depths and parameters may differ.

    The levels are counted from the fine one DOWN, and a stage advances every trial that has a level at that depth: with
    hierarchies [16, 32, 64] and [20, 40] the stages are {16}, then {32, 20}, then {64, 40}.  So a trial joins at its own
    coarsest level, all fine levels run together in the last stage, and a stage lasts as long as its longest trial.
    Every stage is one ``run_chunks`` of ordinary FVSolvers; between stages ONE ``prolong`` call takes every state one
    level up.  A level is the same launches' work whether its trial runs alone or here, so every trial's fields, history,
    ``metrics.iterations`` and ``level_iterations`` are those of its lone ``FVFSGSolver.solve()``.  A trial that stops
    on a NaN on any level gets that level's ``LdcError`` in ``errors[index]`` and goes no further."""

    Solver = FVFSGSolver
    _shares_launches = False                  # (its stages advance ordinary one-CU trials)

    def solve(self, max_iter: int = None):
        ps = [s.params for s in self.solvers]
        caps = [int(p.max_iterations if max_iter is None else max_iter) for p in ps]
        sizes = [s.level_sizes() for s in self.solvers]
        depth = max(len(z) for z in sizes)
        self.errors = {}
        below = {}                                # trial -> its level under the one about to run
        extra = [0] * len(self.solvers)
        for s in self.solvers:
            s.level_iterations = []
        t0 = time.perf_counter()
        out = [None] * len(self.solvers)
        try:
            for above in range(depth - 1, -1, -1):        # levels above: depth - 1 ... 0 (the fine levels)
                group = [q for q in range(len(self.solvers)) if len(sizes[q]) > above and q not in self.errors]
                if not group:
                    continue
                lvls = {}
                for q in group:
                    nx, ny = sizes[q][len(sizes[q]) - 1 - above]
                    lvls[q] = self.solvers[q] if above == 0 else self.solvers[q].make_level(nx, ny)
                prolong([(below[q], lvls[q]) for q in group if q in below])
                for q in group:
                    if q in below:
                        below.pop(q).close()
                    lvls[q]._begin(level_tolerance(ps[q].tolerance, ps[q].coarse_tolerance_factor, above))
                    self.solvers[q]._started = False
                rows = run_chunks([lvls[q].rec_cap for q in group], [caps[q] for q in group],
                                  lambda live, k: advance([lvls[group[i]] for i in live], k))
                for q, row in zip(group, rows):
                    _, nan, total, _ = row
                    self.solvers[q].level_iterations.append(int(total))
                    if nan:
                        self.errors[q] = self._nan_error(lvls[q], total)
                    if above == 0:
                        out[q] = row
                    else:
                        extra[q] += total * lvls[q].nx * lvls[q].ny
                        below[q] = lvls[q]
                log.info("FV sequence, %d level(s) above the fine one: %d trials, iterations %s", above, len(group),
                         [r[2] for r in rows])
        finally:
            for lvl in below.values():
                lvl.close()
        wall = time.perf_counter() - t0
        self.batch_seconds, self.batch_size = wall, len(self.solvers)
        empty = (0, 0, 0, np.zeros((0, F.REC_LEN)))
        self._store([o if o is not None else empty for o in out], wall, extra)
        log.info("batched sequenced solve of %d FV trials finished in %.2f s (%d stopped on a NaN)", len(self.solvers),
                 wall, len(self.errors))
        return [None if q in self.errors else s.metrics for q, s in enumerate(self.solvers)]
