#!/usr/bin/env python3
"""What does the consistent pressure equation cost a chip trial per iteration, and what does it save to the latch?
``mapping="chip"`` with ``pressure_equation="reference"`` against ``"consistent"``, TVD (the YAML's settings), one trial at
a time alone on the card, the two modes alternating in ONE process.

    python tools/fv_pressure_perf.py [--cost-sizes 64,128,256,512] [--solve-sizes 64,128] [--out profiles/fv_pressure.md]
                                     [--reference-only]

(a) Cost: launches and milliseconds per SIMPLE iteration of both modes from rest at Re = 100 and tolerance 1e-30,
    ``--rounds`` timed chunks each, taken in turns; median and range; the BiCGSTAB and CG iterations per SIMPLE iteration
    and the budgets (which set the number of launches) beside them.  ``--reference-only`` times the reference mode alone:
    the figure to compare with tools/fv_wide_perf.py in a checkout of the parent commit.
(b) Iterations and wall time to tolerance 1e-6 at Re = 1000 with relaxation 0.4 / 0.2 and 0.7 / 0.3, both modes.  A solve
    stops at ``--max-iterations``, on a NaN, or is listed as not run when its estimated time does not fit what is left of
    ``--seconds``.

The tables go between the two marker lines of ``--out`` (the rest of that file is kept) and one JSON line per figure
beside it.
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
BEGIN, END = "<!-- fv_pressure_perf: tables -->", "<!-- fv_pressure_perf: end -->"
CHUNK = {64: 128, 128: 64, 256: 32, 512: 16, 1024: 8}         # iterations per timed chunk of (a)
MODES = ("reference", "consistent")


def cost(FVSolver, F, n, rounds, modes):
    k = CHUNK.get(n, 16)
    kw = dict(YAML, nx=n, ny=n, Re=100.0, tolerance=1e-30, max_iterations=10**9, check_every=k, mapping="chip")
    trials = {m: FVSolver(**dict(kw, pressure_equation=m)) for m in modes}
    times = {m: [] for m in trials}
    for s in trials.values():
        s._begin(1e-30)
        s._advance(k)                                     # (warm: the budgets settle, the first launches are paid)
    c0 = {m: s.counters() for m, s in trials.items()}
    for _ in range(rounds):
        for m, s in trials.items():                       # in turns
            t0 = time.perf_counter()
            s._advance(k)
            times[m].append(1e3 * (time.perf_counter() - t0) / k)
    out = dict(N=n, chunk=k, rounds=rounds)
    for m, s in trials.items():
        c, t = s.counters(), times[m]
        assert c["iterations"] == (rounds + 1) * k and c["nan"] == 0
        if s.consistent:
            F.check(F.lib().ldc_fv_wide_set_pressure_budget(s._wide, s.pressure_budget), "ldc_fv_wide_set_pressure_budget")
        out[m] = dict(ms_median=round(statistics.median(t), 4), ms_min=round(min(t), 4), ms_max=round(max(t), 4),
                      launches=F.lib().ldc_fv_wide_launches(s._wide, s.linear_budget),
                      bicgstab_per_iteration=round((c["linear_iterations"] - c0[m]["linear_iterations"]) / (rounds * k), 1),
                      linear_budget=int(s.linear_budget))
        if s.consistent:
            out[m].update(cg_per_solve=round((c["pressure_iterations"] - c0[m]["pressure_iterations"]) / (rounds * k), 1),
                          pressure_budget=int(s.pressure_budget), caps=c["pressure_caps"])
        s.close()
    return out


def solve(FVSolver, n, re, auv, ap, mode, cap):
    s = FVSolver(**dict(YAML, nx=n, ny=n, Re=re, alpha_uv=auv, alpha_p=ap, tolerance=1e-6, max_iterations=cap,
                        check_every=256, mapping="chip", pressure_equation=mode))
    out = dict(N=n, Re=re, alpha_uv=auv, alpha_p=ap, mode=mode)
    t0 = time.perf_counter()
    try:
        s.solve()
        m = s.metrics
        out.update(iterations=int(m.iterations), end="latch" if m.converged else "cap", seconds=round(m.wall_time_seconds, 3))
    except Exception as exc:                              # (a NaN ends a solve with the library's error)
        out.update(iterations=s.counters()["iterations"], end=f"error: {str(exc)[:60]}",
                   seconds=round(time.perf_counter() - t0, 3))
    c = s.counters()
    out.update(bicgstab=c["linear_iterations"], cg=c.get("pressure_iterations"), caps=c.get("pressure_caps"),
               budgets=[int(s.linear_budget), int(s.pressure_budget) if s.consistent else None])
    s.close()
    return out


def cost_table(costs):
    rows = ["| N | chunk x rounds | mode | launches / iteration | ms / iteration (min ... max) | BiCGSTAB / iteration, budget | "
            "CG / solve, budget | ms / reference |", "|---|---|---|---|---|---|---|---|"]
    for r in costs:
        for m in MODES:
            if m not in r:
                rows.append(f"| {r['N']} | {r['chunk']} x {r['rounds']} | {m} | not run | - | - | - | - |")
                continue
            d = r[m]
            cg = f"{d['cg_per_solve']}, {d['pressure_budget']}" if "cg_per_solve" in d else "-"
            ratio = f"{d['ms_median'] / r['reference']['ms_median']:.2f}" if "reference" in r else "-"
            rows.append(f"| {r['N']} | {r['chunk']} x {r['rounds']} | {m} | {d['launches']} | {d['ms_median']:.3f} "
                        f"({d['ms_min']:.3f} ... {d['ms_max']:.3f}) | {d['bicgstab_per_iteration']}, {d['linear_budget']} | {cg} | "
                        f"{ratio} |")
    return "\n".join(rows) + "\n"


def solve_table(solves, skipped):
    rows = ["| N | Re | alpha_uv / alpha_p | mode | iterations | ended at | seconds | BiCGSTAB iterations | CG iterations (caps) | "
            "budgets |", "|---|---|---|---|---|---|---|---|---|---|"]
    for r in solves:
        cg = f"{r['cg']} ({r['caps']})" if r["cg"] is not None else "-"
        rows.append(f"| {r['N']} | {r['Re']:g} | {r['alpha_uv']} / {r['alpha_p']} | {r['mode']} | {r['iterations']} | {r['end']} | "
                    f"{r['seconds']:.2f} | {r['bicgstab']} | {cg} | {r['budgets']} |")
    for n, re, auv, ap, mode in skipped:
        rows.append(f"| {n} | {re:g} | {auv} / {ap} | {mode} | not measured | - | - | - | - | - |")
    return "\n".join(rows) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cost-sizes", default="64,128,256,512")
    ap.add_argument("--solve-sizes", default="64,128")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--max-iterations", type=int, default=20000)
    ap.add_argument("--seconds", type=float, default=420.0, help="(b) starts no solve it cannot expect to finish within this")
    ap.add_argument("--reference-only", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "fv_pressure.md"))
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from solvers.fv import ldc_fv_lib as F
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

    modes = MODES[:1] if a.reference_only else MODES
    t_start = time.perf_counter()
    costs, solves, skipped = [], [], []
    for n in [int(x) for x in a.cost_sizes.split(",") if x]:
        costs.append(cost(FVSolver, F, n, a.rounds, modes))
        record(costs[-1])
    per_iteration = {(r["N"], m): 1e-3 * r[m]["ms_median"] for r in costs for m in modes}
    for n in [int(x) for x in a.solve_sizes.split(",") if x]:
        for auv, alp in ((0.4, 0.2), (0.7, 0.3)):
            for mode in modes[::-1]:                      # (the consistent solves first: they are what is new)
                left = a.seconds - (time.perf_counter() - t_start)
                guess = per_iteration.get((n, mode), 1e-3) * (a.max_iterations if mode == "reference" else 6000)
                if guess > left:
                    skipped.append((n, 1000.0, auv, alp, mode))
                    record(dict(N=n, Re=1000.0, alpha_uv=auv, mode=mode, not_run=f"{guess:.0f} s expected, {left:.0f} s left"))
                    continue
                solves.append(solve(FVSolver, n, 1000.0, auv, alp, mode, a.max_iterations))
                record(solves[-1])
    text = (f"{BEGIN}\n(a) Cost per SIMPLE iteration, Re = 100 from rest, one trial at a time:\n\n{cost_table(costs)}\n"
            f"(b) To tolerance 1e-6 at Re = 1000 (cap {a.max_iterations} iterations):\n\n{solve_table(solves, skipped)}{END}\n")
    old = out.read_text() if out.exists() else ""
    if BEGIN in old and END in old:
        text = old[: old.index(BEGIN)] + text + old[old.index(END) + len(END):].lstrip("\n")
    else:
        text = old + ("\n" if old and not old.endswith("\n") else "") + text
    out.write_text(text)
    print(text)


if __name__ == "__main__":
    main()
