#!/usr/bin/env python3
"""What does ``mapping="chip"`` buy a lone finite-volume trial?  TVD at Re = 1000 (the YAML's settings), from rest:

  rate   per size, after ``--warmup`` iterations, ``--rounds`` rounds in ONE process that alternate the mappings: the
         one-CU trial (N <= 256), the chip trial with every kernel launched on its own and the chip trial replaying one
         hipGraph per iteration; microseconds per iteration (best and worst round), launches per iteration and the mean
         BiCGSTAB iterations per momentum solve.  N = 512 and 1024: the chip trial alone;
  solve  one N = 128 solve to 1e-6 with each mapping: iterations, wall time, max-norm difference of u, v, p.

    python tools/fv_wide_perf.py [--sizes 64,128,256,512,1024] [--out profiles/fv_wide.md]

Every step is a fresh child process under a time limit of its own; after a step that fails or passes its limit nothing
more is started, the tables are written with what there is and the tool exits non-zero.  Writes Markdown to ``--out``
and one JSON line per step beside it.
"""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "02689-advancednumericalalgorithmp3_amd" / "src")]

YAML = dict(convection_scheme="TVD", alpha_uv=0.4, alpha_p=0.2, linear_solver_tol=1e-9)
CU_MAX = 256


def rate(a):
    """The child: one size, the forms alternated round by round."""
    import torch
    import __graft_entry__ as g
    g.build()
    from solvers.fv import ldc_fv_lib as F
    from solvers.fv.solver import FVSolver
    n, chunk = int(a.rate), int(a.chunk)
    kw = dict(YAML, name="fv", nx=n, ny=n, Re=1000.0, tolerance=1e-30, max_iterations=10**9, check_every=chunk)
    forms = {}
    if n <= CU_MAX:
        forms["cu"] = FVSolver(**kw)
    for name, graph in (("chip eager", False), ("chip graph", True)):
        forms[name] = FVSolver(**kw, mapping="chip")
        forms[name].set_wide_graph(graph)
    for s in forms.values():                     # the warm-up: every form reaches the same iteration count
        s._begin(1e-30)
        left = int(a.warmup)
        while left > 0:
            s._advance(min(chunk, left))
            left -= min(chunk, left)
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    before = {k: s.counters() for k, s in forms.items()}
    for _ in range(int(a.rounds)):
        for k, s in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s._advance(chunk)
            times[k].append(1e6 * (time.perf_counter() - t0) / chunk)
    out = dict(step="rate", N=n, warmup=int(a.warmup), chunk=chunk, rounds=int(a.rounds), forms={})
    for k, s in forms.items():
        c, b = s.counters(), before[k]
        solves = c["momentum_solves"] - b["momentum_solves"]
        launches = None
        if s.chip:
            launches = F.lib().ldc_fv_wide_launches(s._wide, s.linear_budget)
        out["forms"][k] = dict(us_best=round(min(times[k]), 1), us_worst=round(max(times[k]), 1),
                               launches_per_iteration=launches, linear_budget=s.linear_budget if s.chip else None,
                               retries_while_timed=c["linear_budget_retries"] - b["linear_budget_retries"],
                               mean_bicgstab=round((c["linear_iterations"] - b["linear_iterations"]) / max(1, solves), 2),
                               iterations=c["iterations"])
        s.close()
    print(json.dumps(out), flush=True)


def solve(a):
    """The child: N = 128, Re = 1000 to 1e-6, the one-CU mapping and then the chip mapping."""
    import numpy as np
    import __graft_entry__ as g
    g.build()
    from solvers.fv.solver import FVSolver
    n = int(a.solve)
    out, fields = dict(step="solve", N=n, forms={}), {}
    for mapping in ("cu", "chip"):
        s = FVSolver(**YAML, name="fv", nx=n, ny=n, Re=1000.0, tolerance=1e-6, max_iterations=200000, mapping=mapping)
        s.solve()
        m = s.metrics
        out["forms"][mapping] = dict(iterations=int(m.iterations), converged=bool(m.converged),
                                     seconds=round(m.wall_time_seconds, 3), retries=s.counters()["linear_budget_retries"])
        fields[mapping] = s.state()
        s.close()
    out["max_difference"] = {k: float(np.max(np.abs(fields["cu"][k] - fields["chip"][k]))) for k in ("u", "v", "p")}
    print(json.dumps(out), flush=True)


def limit(step, n):
    """Seconds allowed to a step: a minute to start and build the eigenvectors, then the step's iterations at the
    one-CU kernel's 15 ms x (n / 256)^2 (profiles/fv_perf.md) with a factor of 3; the N = 128 solve took 29 s there."""
    return 60.0 + (180.0 if step == "solve" else 3.0 * 1000 * 0.015 * (min(n, 512) / 256.0) ** 2 + n / 8.0)


def tables(results):
    rows = ["| N | form | us / iteration (best) | (worst round) | launches / iteration | budget | retries while timed | "
            "mean BiCGSTAB iterations | cu / this |", "|---|---|---|---|---|---|---|---|---|"]
    for r in results:
        if r.get("step") != "rate":
            continue
        if "error" in r:
            rows.append(f"| {r['N']} | {r['error']} | - | - | - | - | - | - | - |")
            continue
        cu = r["forms"].get("cu", {}).get("us_best")
        for k, f in r["forms"].items():
            rows.append("| {} | {} | {} | {} | {} | {} | {} | {} | {} |".format(
                r["N"], k, f["us_best"], f["us_worst"], f["launches_per_iteration"] or 1, f["linear_budget"] or "-",
                f["retries_while_timed"], f["mean_bicgstab"], f"{cu / f['us_best']:.2f}" if cu else "-"))
    text = "Rate (TVD, Re = 1000, from rest, after the warm-up; the forms alternate in one process):\n\n" + "\n".join(rows) + "\n"
    for r in results:
        if r.get("step") != "solve":
            continue
        text += f"\nSolve to 1e-6 at N = {r['N']}, Re = 1000:\n\n"
        if "error" in r:
            text += r["error"] + "\n"
            continue
        text += "| mapping | iterations | converged | seconds | budget retries |\n|---|---|---|---|---|\n"
        for k, f in r["forms"].items():
            text += f"| {k} | {f['iterations']} | {f['converged']} | {f['seconds']} | {f['retries']} |\n"
        text += "\nmax-norm difference of the fields: " + ", ".join(f"{k} {v:.2e}" for k, v in r["max_difference"].items()) + "\n"
    return text


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,128,256,512,1024")
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--chunk", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--solve-size", type=int, default=128)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "fv_wide.md"))
    ap.add_argument("--rate", type=int, help=argparse.SUPPRESS)
    ap.add_argument("--solve", type=int, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.rate:
        return rate(a)
    if a.solve:
        return solve(a)
    import __graft_entry__ as g
    g.build()                                     # once, here: the children find the library up to date
    out, results, failed = Path(a.out), [], None
    out.parent.mkdir(parents=True, exist_ok=True)
    log = out.with_suffix(".jsonl")
    log.write_text("")
    me = [sys.executable, str(Path(__file__).resolve()), "--warmup", str(a.warmup), "--chunk", str(a.chunk),
          "--rounds", str(a.rounds)]
    steps = [("rate", int(x)) for x in a.sizes.split(",") if x] + ([("solve", a.solve_size)] if a.solve_size else [])
    for step, n in steps:
        try:
            r = subprocess.run(me + [f"--{step}", str(n)], capture_output=True, text=True, timeout=limit(step, n))
            lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
            if r.returncode != 0 or not lines:
                failed = f"{step} at N = {n}: exit {r.returncode}\n{r.stderr[-3000:]}"
        except subprocess.TimeoutExpired:
            failed, lines = f"{step} at N = {n}: no result within {limit(step, n):.0f} s", []
        results.append(json.loads(lines[-1]) if lines and not failed else dict(step=step, N=n, error="failed"))
        print(json.dumps(results[-1]), flush=True)
        with log.open("a") as f:
            f.write(json.dumps(results[-1]) + "\n")
        out.write_text(tables(results))
        if failed:                                # nothing more is started on the card after a step that failed
            break
    print(tables(results))
    if failed:
        sys.exit(f"stopped after a failed step; the tables hold what there was.  {failed}")


if __name__ == "__main__":
    main()
