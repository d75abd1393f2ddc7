#!/usr/bin/env python3
"""What does Anderson mixing cost a chip trial, and what does it save?  ``mapping="chip"`` plain against
``acceleration="anderson_chip"``, TVD (the YAML's settings), one trial at a time alone on the card, plain and accelerated
runs alternating in ONE process.

    python tools/fv_wide_anderson_perf.py [--cost-sizes 64,256,1024] [--solves 64:400,128:1000,256:1000]
                                          [--depths 5,10] [--out profiles/fv_wide_anderson.md] [--plain-only]

(a) Cost of mixing: microseconds per iteration of a plain trial and of one mixed at depth 5 from iteration 2 on, both from
    rest at Re = 100 and tolerance 1e-30, ``--rounds`` timed chunks each, taken in turns; median and range.  The two
    trials walk different paths, so the BiCGSTAB iterations per SIMPLE iteration and the budget (which sets the number of
    launches) stand beside the times.  ``--plain-only`` times the plain trial alone: the figure to compare with the same
    tool run in a checkout of the parent commit.
(b) Iterations and wall time to tolerance 1e-6: plain, then every depth, per (N, Re); fallbacks and BiCGSTAB iterations
    too.  A solve stops at ``--max-iterations``; a case whose estimated time does not fit what is left of ``--seconds`` is
    listed as not run.

The tables go between the two marker lines of ``--out`` (the rest of that file is kept; a file without markers gets them
at its end) and one JSON line per figure beside it.
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "02689-advancednumericalalgorithmp3_amd" / "src")]

YAML = dict(name="fv", convection_scheme="TVD", alpha_uv=0.4, alpha_p=0.2, linear_solver_tol=1e-9)
BEGIN, END = "<!-- fv_wide_anderson_perf: tables -->", "<!-- fv_wide_anderson_perf: end -->"
CHUNK = {64: 256, 128: 128, 256: 64, 512: 32, 1024: 16}       # iterations per timed chunk of (a)


def cost(FVSolver, n, depth, rounds, plain_only):
    """(a) at n x n: per trial the microseconds per iteration of every timed chunk."""
    k = CHUNK.get(n, 32)
    kw = dict(YAML, nx=n, ny=n, Re=100.0, tolerance=1e-30, max_iterations=10**9, check_every=k, mapping="chip")
    trials = {"plain": FVSolver(**kw)}
    if not plain_only:
        trials["mixed"] = FVSolver(**dict(kw, acceleration="anderson_chip", anderson_depth=depth, anderson_start=2))
    times = {name: [] for name in trials}
    for s in trials.values():
        s._begin(1e-30)
        s._advance(k)                                     # (warm: the budget settles, the first launches are paid)
    lin0 = {name: s.counters()["linear_iterations"] for name, s in trials.items()}
    for _ in range(rounds):
        for name, s in trials.items():                    # in turns
            t0 = time.perf_counter()
            s._advance(k)
            times[name].append(1e6 * (time.perf_counter() - t0) / k)
    out = dict(N=n, chunk=k, rounds=rounds, depth=depth)
    for name, s in trials.items():
        c, t = s.counters(), times[name]
        assert c["iterations"] == (rounds + 1) * k and c["nan"] == 0
        out[name] = dict(us_median=round(statistics.median(t), 1), us_min=round(min(t), 1), us_max=round(max(t), 1),
                         bicgstab_per_iteration=round((c["linear_iterations"] - lin0[name]) / (rounds * k), 1),
                         budget=int(s.linear_budget), fallbacks=c["anderson_fallbacks"])
        s.close()
    return out


def solve(FVSolver, n, re, depth, cap):
    kw = dict(YAML, nx=n, ny=n, Re=re, tolerance=1e-6, max_iterations=cap, check_every=256, mapping="chip")
    if depth:
        kw.update(acceleration="anderson_chip", anderson_depth=depth)
    s = FVSolver(**kw)
    s.solve()
    m, c = s.metrics, s.counters()
    out = dict(N=n, Re=re, depth=depth, iterations=int(m.iterations), converged=bool(m.converged),
               seconds=round(m.wall_time_seconds, 3), fallbacks=c["anderson_fallbacks"],
               bicgstab=c["linear_iterations"], budget=int(s.linear_budget), retries=c["linear_budget_retries"])
    s.close()
    return out


def cost_table(costs):
    rows = ["| N | chunk x rounds | plain, us / iteration (min ... max) | BiCGSTAB / iteration, budget | depth 5, us / iteration "
            "(min ... max) | BiCGSTAB / iteration, budget | extra, us |", "|---|---|---|---|---|---|---|"]
    for r in costs:
        p, x = r["plain"], r.get("mixed")
        cell = lambda d: f"{d['us_median']} ({d['us_min']} ... {d['us_max']}) | {d['bicgstab_per_iteration']}, {d['budget']}"  # noqa: E731
        rows.append(f"| {r['N']} | {r['chunk']} x {r['rounds']} | {cell(p)} | " + (
            f"{cell(x)} | {x['us_median'] - p['us_median']:.1f} |" if x else "not run | - | - |"))
    return "\n".join(rows) + "\n"


def solve_table(solves, skipped):
    rows = ["| N | Re | acceleration | iterations | converged | seconds | fallbacks | BiCGSTAB iterations | budget (retries) | "
            "iterations / plain | seconds / plain |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    plain = {(r["N"], r["Re"]): r for r in solves if r["depth"] == 0}
    for r in solves:
        p = plain.get((r["N"], r["Re"]))
        rel = p is not None and r["depth"] > 0
        rows.append("| {N} | {Re:g} | {acc} | {iterations} | {conv} | {seconds:.2f} | {fallbacks} | {bicgstab} | {budget} ({retries}) "
                    "| {ri} | {rs} |".format(acc=f"depth {r['depth']}" if r["depth"] else "none",
                                             conv="yes" if r["converged"] else "no (cap)",
                                             ri=f"{r['iterations'] / p['iterations']:.2f}" if rel else "-",
                                             rs=f"{r['seconds'] / p['seconds']:.2f}" if rel else "-", **r))
    for n, re, depth in skipped:
        rows.append(f"| {n} | {re:g} | {'depth %d' % depth if depth else 'none'} | not run | - | - | - | - | - | - | - |")
    return "\n".join(rows) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cost-sizes", default="64,256,1024")
    ap.add_argument("--solves", default="64:400,128:1000,256:1000")
    ap.add_argument("--depths", default="5,10")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--max-iterations", type=int, default=30000)
    ap.add_argument("--seconds", type=float, default=420.0, help="(b) starts no solve it cannot expect to finish within this")
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "fv_wide_anderson.md"))
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from solvers.fv.solver import FVSolver
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    log = out.with_suffix(".jsonl")
    log.write_text("")

    def record(r):
        line = json.dumps(r)
        print(line, flush=True)
        with log.open("a") as f:
            f.write(line + "\n")

    t_start = time.perf_counter()
    costs, solves, skipped = [], [], []
    for n in [int(x) for x in a.cost_sizes.split(",") if x]:
        costs.append(cost(FVSolver, n, 5, a.rounds, a.plain_only))
        record(costs[-1])
    depths = [int(x) for x in a.depths.split(",") if x]
    per_iteration = {}                                            # seconds per iteration at N, from the solves done
    for case in ([] if a.plain_only else [x for x in a.solves.split(",") if x]):
        n, re = int(case.split(":")[0]), float(case.split(":")[1])
        for depth in [0] + depths:
            left = a.seconds - (time.perf_counter() - t_start)
            guess = per_iteration.get(n, 0.5e-3 * max(1.0, (n / 256.0) ** 2)) * a.max_iterations
            if guess > left:
                skipped.append((n, re, depth))
                record(dict(N=n, Re=re, depth=depth, not_run=f"{guess:.0f} s at the cap, {left:.0f} s left"))
                continue
            solves.append(solve(FVSolver, n, re, depth, a.max_iterations))
            record(solves[-1])
            per_iteration[n] = max(per_iteration.get(n, 0.0), solves[-1]["seconds"] / max(1, solves[-1]["iterations"]))
    text = (f"{BEGIN}\n(a) Cost of mixing, Re = 100 from rest, one trial at a time:\n\n{cost_table(costs)}\n"
            f"(b) To tolerance 1e-6 (cap {a.max_iterations} iterations):\n\n{solve_table(solves, skipped)}{END}\n")
    old = out.read_text() if out.exists() else ""
    if BEGIN in old and END in old:
        text = old[: old.index(BEGIN)] + text + old[old.index(END) + len(END):].lstrip("\n")
    else:
        text = old + ("\n" if old and not old.endswith("\n") else "") + text
    out.write_text(text)
    print(text)


if __name__ == "__main__":
    main()
