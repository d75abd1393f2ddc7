"""Advancing trials chunk by chunk, for lone solvers and batches alike.

The trials (SGSolvers) of one call share a handle: a lone solver's own or a batch's (batched.py).  ``advance`` runs one
chunk; ``run_iterations`` and ``run_to_tolerance`` loop over chunks.  Nothing here calls torch.cuda (waits go through the
trials' ``_sync``).  After an upload in the tail layout a lone solver runs the first iteration inside its first chunk
(1, C-1, C, ...), a batch as a chunk of its own (1, C, ...): the two orders end their chunks at different iterations.
"""
from __future__ import annotations

import contextlib

import numpy as np

from . import ldc_lib as L

LATCH_CAPPED = 3      # ctrl[DONE] code set by the host when a trial of a batch reaches its own max_iterations


def _words(tensors):
    """ONE device-to-host copy of a word of every trial (a blocking copy per trial and kind -- four of them -- was 12 ms
    of host time per chunk at 256 trials, as much as the chunk itself at N = 16)."""
    import torch
    return (tensors[0][None] if len(tensors) == 1 else torch.stack(tensors)).cpu().numpy()


def advance(trials, n_iters, diagnostics, enqueue, mode, device_index):
    """``n_iters`` iterations (at most the smallest record ring) for every trial through ``enqueue(n_iters, diagnostics)``;
    returns per-trial (records of the new iterations, latch, iteration count).  ``mode``: the handle's kernel (0, 3, 4, 5).
    The first iteration after an upload runs alone (then phi^n carries its boundary values: SGSolver.set_state)."""
    n_iters = min(int(n_iters), min(s.rec_cap for s in trials))
    if n_iters > 1 and any(s._edge_fix_pending for s in trials):
        first = advance(trials, 1, diagnostics, enqueue, mode, device_index)
        if all(latch for _, latch, _ in first):
            return first
        rest = advance(trials, n_iters - 1, diagnostics, enqueue, mode, device_index)
        return [(np.concatenate([r1, r2], axis=0), latch, end) for (r1, _, _), (r2, latch, end) in zip(first, rest)]
    starts = _words([s.d["ctrl"] for s in trials])[:, L.CTRL_ITER].tolist()
    resident = n_iters > 1 and mode in (3, 4, 5)          # work-groups that must be co-resident: see ldc_lib.resident_lock
    with L.resident_lock(device_index) if resident else contextlib.nullcontext():
        enqueue(n_iters, diagnostics)
        trials[0]._sync()
    ctrl = _words([s.d["ctrl"] for s in trials])[:, [L.CTRL_DONE, L.CTRL_ITER]].tolist()
    if _words([s.d["sync"][L.SYNC_GIVEUP] for s in trials]).any():
        raise L.LdcError("a persistent launch gave up a barrier wait (a work-group was not resident); the state is "
                         "undefined -- rerun with persistent=0")
    if len({s.rec_cap for s in trials}) == 1:
        rings = _words([s.d["rec"] for s in trials])
    else:
        rings = [s.d["rec"].cpu().numpy() for s in trials]
    out = []
    for s, start, (done, end), ring in zip(trials, starts, ctrl, rings):
        out.append((ring[np.arange(start, end) % s.rec_cap], done, end))
        if s._edge_fix_pending and end > start:
            s._write_boundary_edges(("U", "UT", "V", "VT"))
            s._edge_fix_pending = False
    return out


def _chunk(trials, k, batch):          # (module docstring: the first chunk after an upload)
    return 1 if batch and any(s._edge_fix_pending for s in trials) else k


def run_iterations(trials, step, n, batch):
    """``n`` more iterations for every trial; per-trial record arrays.  ``step(k)``: one ``advance`` of the trials' handle.
    A lone solver stops at its latch; a batch enqueues all ``n``."""
    rows = [[] for _ in trials]
    left, cap = int(n), min(s.rec_cap for s in trials)
    while left > 0:
        k = _chunk(trials, min(left, cap), batch)
        out = step(k)
        for q, (r, _, _) in enumerate(out):
            rows[q].append(r)
        left -= k
        if not batch and out[0][1]:
            break
    return [np.concatenate(r, axis=0) if r else np.zeros((0, L.REC_LEN)) for r in rows]


def run_to_tolerance(trials, step, caps, batch):
    """Every trial from iteration 0 until ITS latch fires or ITS cap is reached; per-trial (latch, iterations, records).
    In a batch a capped trial is latched on the device (LATCH_CAPPED): its work-groups leave every later launch at entry,
    like a converged trial's -- the outcome of the reference's one-process-per-trial runs with different caps.  A lone
    solver just stops (its latch reads LATCH_CAPPED in the result only)."""
    n = len(trials)
    chunk = min(s.rec_cap for s in trials)
    blocks = [[] for _ in trials]
    state = [(0, 0)] * n
    it = 0
    while True:
        live = [q for q in range(n) if not state[q][0]]
        for q in live:
            if it >= caps[q]:
                if batch:
                    trials[q].d["ctrl"][L.CTRL_DONE] = LATCH_CAPPED
                state[q] = (LATCH_CAPPED, state[q][1])
        live = [q for q in live if not state[q][0]]
        if not live:
            break
        k = _chunk(trials, min(chunk, min(caps[q] for q in live) - it), batch)
        for q, (rows, done, total) in enumerate(step(k)):
            if state[q][0] != LATCH_CAPPED:
                blocks[q].append(rows)
                state[q] = (done, total)
        it += k
    trials[0]._sync()
    return [(d, t, np.concatenate(b, axis=0) if b else np.zeros((0, L.REC_LEN))) for (d, t), b in zip(state, blocks)]
