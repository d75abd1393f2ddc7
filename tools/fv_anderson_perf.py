#!/usr/bin/env python3
"""Does Anderson acceleration pay for the finite-volume solver?  ``solver=fv`` plain against ``acceleration=anderson``
at depth 5 and 10, N = 64 and 128, Re = 100, 400 and 1000, TVD (the YAML's settings), tolerance 1e-6: iterations, wall
time of the solve, microseconds per iteration and fallbacks; then what one launch per iteration costs: a plain trial
advanced by ``ldc_fv_anderson_enqueue`` at depth 0 against the same trial advanced by ``ldc_fv_batch_enqueue``.

    python tools/fv_anderson_perf.py [--sizes 64,128] [--re 100,400,1000] [--depths 5,10] [--out profiles/fv_anderson.md]

Every solve runs ONCE, in a fresh child process under an iteration cap (``--max-iterations``) and a time limit of its
own that follows from the cap (``limit``).  The sizes are taken one after another, smallest first; the solves of one
size start together and run side by side (a finite-volume trial is one work-group on one CU, so they do not compete for
CUs; at most 9 processes).  The launch-cost runs come last, one at a time, alone on the card.  After a solve that
passes its limit or exits with anything but 0, the solves already running are left to end, no further one is started,
the table is written with what there is and the tool exits non-zero.  Writes the Markdown tables to ``--out`` (again
after every size) and one JSON line per run beside it.
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


def one(a):
    """The child: one solve, one JSON line."""
    import __graft_entry__ as g
    g.build()
    from solvers.fv.solver import FVSolver
    n, re, depth = (int(a.one[0]), float(a.one[1]), int(a.one[2]))
    kw = dict(YAML, name="fv", nx=n, ny=n, Re=re, tolerance=1e-6, max_iterations=a.max_iterations,
              vortex_metrics="device")
    if depth > 0:
        kw.update(acceleration="anderson", anderson_depth=depth)
    s = FVSolver(**kw)
    s.solve()
    m, c = s.metrics, s.counters()
    print(json.dumps(dict(N=n, Re=re, depth=depth, iterations=int(m.iterations), converged=bool(m.converged),
                          seconds=round(m.wall_time_seconds, 3), us_per_iteration=round(1e6 * m.wall_time_seconds / max(1, m.iterations), 1),
                          fallbacks=c["anderson_fallbacks"], final_residual=m.final_residual, psi_min=m.psi_min)), flush=True)
    s.close()


def launch_cost(a):
    """The child: ``iters`` iterations of one plain trial from rest, in chunks of ``check_every``, by the plain launch
    and then, on a second trial, by one launch per iteration and the mixing kernel at depth 0; the states must agree
    bit for bit."""
    import numpy as np
    import torch
    import __graft_entry__ as g
    g.build()
    from solvers.fv import ldc_fv_lib as F
    from solvers.fv.solver import FVSolver, advance
    n, iters, chunk = int(a.launch_cost[0]), int(a.launch_cost[1]), 256
    kw = dict(YAML, name="fv", nx=n, ny=n, Re=100.0, tolerance=1e-30, max_iterations=iters, check_every=chunk)
    out = {}
    states = []
    for mode in ("plain", "depth0"):
        s = FVSolver(**kw)
        s._begin(1e-30)
        stream = torch.cuda.current_stream(s.device)
        advance([s], 8)                                   # (warm the launch path; counted out below)
        s._begin(1e-30)
        s.set_state(*(np.zeros(s.t[k].numel()) for k in ("u", "v", "p", "mdot")))
        stream.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters // chunk):
            if mode == "plain":
                F.batch_enqueue([s.handle], chunk, stream.cuda_stream)
            else:
                F.anderson_enqueue([s.handle], [s._anderson_block()], chunk, stream.cuda_stream)
            stream.synchronize()
        out[mode] = 1e6 * (time.perf_counter() - t0) / (iters // chunk * chunk)
        assert s.counters()["iterations"] == iters // chunk * chunk
        states.append(s.state())
        s.close()
    same = all(np.array_equal(states[0][k], states[1][k]) for k in states[0])
    print(json.dumps(dict(N=n, iterations=iters // chunk * chunk, chunk=chunk, plain_us=round(out["plain"], 1),
                          depth0_us=round(out["depth0"], 1), extra_us=round(out["depth0"] - out["plain"], 1),
                          bit_identical=bool(same))), flush=True)


def limit(n, cap):
    """Seconds allowed to one solve: the iteration cap at 15 ms x (n / 256)^2 per iteration (profiles/fv_perf.jsonl:
    15.2 ms at 256, 2.5 ms at 128, 0.65 ms at 64), twice that for the mixing launches and the neighbours, and a minute
    to start the process and load the library.  A solve that passes it does not merely need longer."""
    return 60.0 + 2.0 * cap * 0.015 * (n / 256.0) ** 2


def table(sizes, res, depths, results):
    rows = ["| N | Re | acceleration | iterations | converged | seconds | us / iteration | fallbacks | iterations / plain | seconds / plain |",
            "|---|---|---|---|---|---|---|---|---|---|"]
    for n in sizes:
        for re in res:
            plain = results.get((n, re, 0), {})
            for d in [0] + depths:
                r = results.get((n, re, d))
                if r is None:
                    continue
                ok = "error" not in r and "error" not in plain and plain.get("iterations")
                rows.append("| {} | {:g} | {} | {} | {} | {} | {} | {} | {} | {} |".format(
                    n, re, "none" if d == 0 else f"depth {d}", r.get("iterations", r.get("error", "-")),
                    {True: "yes", False: "no"}.get(r.get("converged"), "-"),
                    f"{r['seconds']:.2f}" if "seconds" in r else "-", r.get("us_per_iteration", "-"),
                    r.get("fallbacks", "-"),
                    f"{r['iterations'] / plain['iterations']:.2f}" if ok and d else "-",
                    f"{r['seconds'] / plain['seconds']:.2f}" if ok and d else "-"))
    return "\n".join(rows) + "\n"


def cost_table(costs):
    rows = ["| N | iterations | chunk | plain launch, us / iteration | depth 0, us / iteration | extra | bit-identical |",
            "|---|---|---|---|---|---|---|"]
    for r in costs:
        rows.append("| {N} | {iterations} | {chunk} | {plain_us} | {depth0_us} | {extra_us} | {bit_identical} |".format(**r)
                    if "error" not in r else f"| {r['N']} | {r['error']} | - | - | - | - | - |")
    return "\n".join(rows) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,128")
    ap.add_argument("--re", default="100,400,1000")
    ap.add_argument("--depths", default="5,10")
    ap.add_argument("--max-iterations", type=int, default=20000)
    ap.add_argument("--cost-iterations", type=int, default=2048)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "fv_anderson.md"))
    ap.add_argument("--one", nargs=3, type=float, metavar=("N", "RE", "DEPTH"), help=argparse.SUPPRESS)
    ap.add_argument("--launch-cost", nargs=2, type=int, metavar=("N", "ITERS"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        return one(a)
    if a.launch_cost:
        return launch_cost(a)
    import __graft_entry__ as g
    g.build()                                     # once, here: the children find the library up to date
    sizes = sorted(int(x) for x in a.sizes.split(","))
    res = [float(x) for x in a.re.split(",")]
    depths = [int(x) for x in a.depths.split(",")]
    if len(res) * (1 + len(depths)) > 12:
        sys.exit("at most 12 solves side by side")
    out, results, costs, failed = Path(a.out), {}, [], None
    out.parent.mkdir(parents=True, exist_ok=True)
    log = out.with_suffix(".jsonl")
    log.write_text("")
    me = [sys.executable, str(Path(__file__).resolve())]

    def record(r):
        line = json.dumps(r)
        print(line, flush=True)
        with log.open("a") as f:
            f.write(line + "\n")

    def write():
        text = ("Solves (the solves of one size ran side by side, one CU each):\n\n" + table(sizes, res, depths, results)
                + "\nOne launch per iteration (a plain trial alone on the card, Re = 100, from rest):\n\n" + cost_table(costs))
        out.write_text(text)
        return text

    t_start = time.perf_counter()
    for n in sizes:                               # one size at a time; its solves start together
        running = {}
        for c in [(n, re, d) for re in res for d in [0] + depths]:
            cmd = me + ["--one", *[str(x) for x in c], "--max-iterations", str(a.max_iterations)]
            running[c] = (subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True), time.perf_counter())
        beat = time.perf_counter()
        while running:
            time.sleep(0.5)
            for c, (proc, t0) in list(running.items()):
                if proc.poll() is None:
                    if time.perf_counter() - t0 > limit(n, a.max_iterations):     # its own time limit
                        proc.kill()
                        proc.communicate()
                        failed = failed or f"{c}: no result within {limit(n, a.max_iterations):.0f} s"
                        results[c] = dict(N=c[0], Re=c[1], depth=c[2], error="no result within its time limit")
                        record(results[c])
                        del running[c]
                    continue
                so, se = proc.communicate()
                lines = [x for x in so.splitlines() if x.startswith("{")]
                if proc.returncode == 0 and lines:
                    results[c] = json.loads(lines[-1])
                else:
                    failed = failed or f"{c}: exit {proc.returncode}\n{se[-3000:]}"
                    results[c] = dict(N=c[0], Re=c[1], depth=c[2], error=f"exit {proc.returncode}")
                record(results[c])
                del running[c]
            if time.perf_counter() - beat > 60:
                beat = time.perf_counter()
                print(f"# {time.perf_counter() - t_start:.0f} s: N = {n}, {len(running)} running", flush=True)
        write()
        if failed:                                # nothing more is started on the card after a solve that failed
            break
    for n in ([] if failed else sizes):           # alone on the card, one after another
        try:
            r = subprocess.run(me + ["--launch-cost", str(n), str(a.cost_iterations)], capture_output=True, text=True,
                               timeout=limit(n, 2 * a.cost_iterations))
            lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
            if r.returncode != 0 or not lines:
                failed = f"launch cost at N = {n}: exit {r.returncode}\n{r.stderr[-3000:]}"
        except subprocess.TimeoutExpired:
            failed, lines = f"launch cost at N = {n}: no result within its time limit", []
        costs.append(json.loads(lines[-1]) if lines and not failed else dict(N=n, error="failed"))
        record(costs[-1])
        if failed:
            break
    print(write())
    if failed:
        sys.exit(f"stopped after a failed run; the tables hold what there was.  {failed}")


if __name__ == "__main__":
    main()
