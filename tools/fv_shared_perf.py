#!/usr/bin/env python3
"""What does ``mapping="shared"`` buy a small finite-volume sweep?  TVD, the YAML's settings, every trial from rest:

  sweep  the reference-shaped sweep N = 64, 128 x Re = 100, 400, 1000 (six trials) as ONE ``"cu"`` batch (one work-group
         per trial), as ``"chip"`` trials one after another (every kernel on its own, and one replayed hipGraph per
         iteration) and as ONE ``"shared"`` batch (likewise both); seconds inside the solves and trial-iterations/s;
  cross  T x N = 64 at Re = 1000 for T = 4, 16, 64, 256 as a ``"cu"`` batch against a ``"shared"`` batch (both launch
         forms): trial-iterations/s, which locates the T from which one CU per trial is the better use of the card.

Every step is ONE child process that alternates its forms, each ``--rounds`` (2) times, every run from rest for
``--iterations`` iterations per trial (0: to 1e-6, at most 20000; nothing latches before at a fixed count, so all forms
do the same work).  Only the chunk loop is timed (enqueue, wait, the copies of the control words and record rows), not
the construction of the trials and not the records made afterwards.

    python tools/fv_shared_perf.py [--iterations 1500] [--trials 4,16,64,256] [--out tables.md]

Every child runs under ``timeout -k 10`` with a limit of its own; after a step that fails or passes its limit nothing
more is started, the tables are written with what there is and the tool exits non-zero.  Prints Markdown (and writes it
to ``--out``) and one JSON line per step beside it.
"""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "02689-advancednumericalalgorithmp3_amd" / "src")]

YAML = dict(name="fv", convection_scheme="TVD", alpha_uv=0.4, alpha_p=0.2, linear_solver_tol=1e-9)
SWEEP = [(n, re) for n in (64, 128) for re in (100.0, 400.0, 1000.0)]


def _from_rest(solvers):
    import numpy as np
    from solvers.fv import ldc_fv_lib as F
    for s in solvers:
        n = s.n_cells
        s.set_state(np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(F.faces(s.nx, s.ny)))


def _lone(s, tol, cap):
    """One trial to its latch or the cap, chunk by chunk as solve() runs it; seconds of the loop, iterations."""
    import torch
    s._begin(tol)
    torch.cuda.synchronize()
    t0, done, total = time.perf_counter(), 0, 0
    while total < cap and not done:
        _, done, total = s._advance(min(s.rec_cap, cap - total))
    return time.perf_counter() - t0, total


def _batch(b, cap):
    b.solve(max_iter=cap)                        # batch_seconds: the chunk loop alone
    if b.errors:
        raise RuntimeError(f"trials stopped on a NaN: {b.errors}")
    return b.batch_seconds, sum(int(s.metrics.iterations) for s in b.solvers)


def child(a):
    """One step: its forms alternated round by round in this process."""
    import __graft_entry__ as g
    g.build()
    from solvers.fv.batched import BatchedFVSolver
    from solvers.fv.solver import FVSolver
    fixed = int(a.iterations) > 0
    tol, cap = (1e-30, int(a.iterations)) if fixed else (1e-6, 20000)
    if a.child == "sweep":
        cases = [dict(YAML, nx=n, ny=n, Re=re, tolerance=tol, max_iterations=cap) for n, re in SWEEP]
    else:
        cases = [dict(YAML, nx=64, ny=64, Re=1000.0, tolerance=tol, max_iterations=cap)] * int(a.child)
    forms = {"cu": BatchedFVSolver(cases)}
    if a.child == "sweep":
        for name, graph in (("chip one by one, eager", False), ("chip one by one, graph", True)):
            forms[name] = [FVSolver(**c, mapping="chip") for c in cases]
            for s in forms[name]:
                s.set_wide_graph(graph)
    for name, graph in (("shared, eager", False), ("shared, graph", True)):
        forms[name] = BatchedFVSolver([dict(c, mapping="shared") for c in cases])
        forms[name].set_wide_graph(graph)
    runs = {k: [] for k in forms}
    for _ in range(int(a.rounds)):
        for k, f in forms.items():
            if isinstance(f, list):
                _from_rest(f)
                parts = [_lone(s, tol, cap) for s in f]
                sec, its = sum(p[0] for p in parts), sum(p[1] for p in parts)
                retries = sum(s.linear_budget_retries for s in f)
            else:
                _from_rest(f.solvers)
                sec, its = _batch(f, cap)
                retries = sum(s.linear_budget_retries for s in f.solvers)
            runs[k].append(dict(seconds=round(sec, 4), trial_iterations=its, rate=round(its / sec, 1), retries=retries))
    for f in forms.values():
        for s in (f if isinstance(f, list) else [f]):
            s.close()
    print(json.dumps(dict(step=a.child, trials=len(cases), iterations=int(a.iterations), forms=runs)), flush=True)


def limit(step, iterations):
    """Seconds allowed to a child: a minute to start and build the trials, then its runs at the one-CU kernel's 2.2 ms per
    iteration at N = 128 (profiles/fv_perf.md) for every form and round, with a factor of 3."""
    its = iterations if iterations > 0 else 12000
    forms = 5 if step == "sweep" else 3
    build = 0 if step == "sweep" else int(step)          # (three batches of T trials are built first: ~0.1 s a trial)
    return int(60 + build + 3 * 2 * forms * its * 2.2e-3 * (6 if step == "sweep" else 1))


def tables(results):
    text = ""
    for r in results:
        head = ("The six-trial sweep N = 64, 128 x Re = 100, 400, 1000" if r["step"] == "sweep"
                else f"T = {r['step']} trials of N = 64, Re = 1000")
        text += f"\n{head} ({r.get('iterations') or 'to 1e-6'} iterations per trial, from rest):\n\n"
        if "error" in r:
            text += r["error"] + "\n"
            continue
        text += "| form | seconds (each run) | trial-iterations / s (each run) | budget retries |\n|---|---|---|---|\n"
        for k, runs in r["forms"].items():
            text += "| {} | {} | {} | {} |\n".format(k, ", ".join(f"{x['seconds']:.3f}" for x in runs),
                                                   ", ".join(f"{x['rate']:.0f}" for x in runs),
                                                   ", ".join(str(x["retries"]) for x in runs))
    return text


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=1500)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--trials", default="4,16,64,256")
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--out", default="")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    import __graft_entry__ as g
    g.build()                                     # once, here: the children find the library up to date
    results, failed = [], None
    steps = ([] if a.no_sweep else ["sweep"]) + [x for x in a.trials.split(",") if x]
    for step in steps:
        sec = limit(step, a.iterations)
        cmd = ["timeout", "-k", "10", str(sec), sys.executable, str(Path(__file__).resolve()), "--child", step,
               "--iterations", str(a.iterations), "--rounds", str(a.rounds)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
        if r.returncode != 0 or not lines:
            failed = f"step {step}: exit {r.returncode} (limit {sec} s)\n{r.stderr[-3000:]}"
        results.append(json.loads(lines[-1]) if lines and not failed else dict(step=step, error="failed"))
        print(json.dumps(results[-1]), flush=True)
        if a.out:
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            Path(a.out).write_text(tables(results))
            with Path(a.out).with_suffix(".jsonl").open("a") as f:
                f.write(json.dumps(results[-1]) + "\n")
        if failed:                                # nothing more is started on the card after a step that failed
            break
    print(tables(results))
    if failed:
        sys.exit(f"stopped after a failed step; the tables hold what there was.  {failed}")


if __name__ == "__main__":
    main()
