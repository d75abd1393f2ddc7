#!/usr/bin/env python3
"""Does coarse-to-fine sequencing pay for the finite-volume solver?  ``solver=fv`` against ``solver=fv/fsg`` at
N = 64, 128, 256, Re = 100 and 1000, TVD (the YAML's settings), tolerance 1e-6, ``n_levels`` 2 and 3: iterations per
level, wall time of the solve, and max|du|, max|dv| between the converged fine fields of the lone and the sequenced solve.

    python tools/fv_fsg_perf.py [--sizes 64,128,256] [--re 100,1000] [--levels 2,3] [--out profiles/fv_fsg.md]

Every solve runs ONCE, in a fresh child process under an iteration cap (``--max-iterations``, per level) and a time
limit of its own that follows from the cap (``limit``).  The sizes are taken one after another, smallest first; the
solves of one size (every Re, from rest and sequenced) start together and run side by side, so the solves that a row's
ratio compares share the card with the same neighbours from the same moment.  A finite-volume trial is one work-group on
one CU for its whole life, so they do not compete for CUs.  After a solve that passes its limit or exits with anything
but 0, the solves already running are left to end, no further one is started, the table is written with what there is
and the tool exits non-zero.  Writes the Markdown table to ``--out`` (again after every size) and one JSON line per
solve beside it.
"""
import argparse
import json
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "02689-advancednumericalalgorithmp3_amd" / "src")]


def one(a):
    """The child: one solve, one JSON line, the fine fields into ``--fields``."""
    import numpy as np
    import __graft_entry__ as g
    g.build()
    from solvers.fv.fsg import FVFSGSolver
    from solvers.fv.solver import FVSolver
    n, re, levels = a.one
    kw = dict(nx=int(n), ny=int(n), Re=float(re), convection_scheme="TVD", alpha_uv=0.4, alpha_p=0.2,
              linear_solver_tol=1e-9, tolerance=1e-6, max_iterations=a.max_iterations, vortex_metrics="device")
    if int(levels) > 1:
        s = FVFSGSolver(name="fv_fsg", n_levels=int(levels), coarsest_n=16, coarse_tolerance_factor=1.0, **kw)
        sizes = [nx for nx, _ in s.level_sizes()]
    else:
        s = FVSolver(name="fv", **kw)
        sizes = [int(n)]
    s.solve()
    its = list(getattr(s, "level_iterations", [s.metrics.iterations]))
    np.savez(a.fields, u=s.fields.u, v=s.fields.v, p=s.fields.p)
    print(json.dumps(dict(N=int(n), Re=float(re), n_levels=int(levels), sizes=sizes, iterations=its,
                          converged=bool(s.metrics.converged), seconds=round(s.metrics.wall_time_seconds, 3),
                          final_residual=s.metrics.final_residual)), flush=True)
    s.close()


def limit(case, cap):
    """Seconds allowed to one solve: every level may run to the iteration cap at 15 ms x (n / 256)^2 per iteration
    (profiles/fv_perf.jsonl: 15.2 ms at 256, 2.5 ms at 128, 0.65 ms at 64), half as much again for the neighbours,
    and a minute to start the process and load the library.  A solve that passes it does not merely need longer."""
    n, _, levels = case
    return 60.0 + 1.5 * cap * sum(0.015 * (n / 2 ** k / 256.0) ** 2 for k in range(levels))


def table(sizes, res, variants, results, np):
    def diff(n, re, lv):
        lone, seq = results.get((n, re, 1), {}), results.get((n, re, lv), {})
        if "fields" not in lone or "fields" not in seq:
            return None
        x, y = np.load(lone["fields"]), np.load(seq["fields"])
        return tuple(float(np.max(np.abs(x[k] - y[k]))) for k in ("u", "v"))

    rows = ["| N | Re | start | levels | iterations per level | converged | seconds | seconds / from rest | max \\|du\\| | max \\|dv\\| |",
            "|---|---|---|---|---|---|---|---|---|---|"]
    for n in sizes:
        for re in res:
            lone = results.get((n, re, 1), {})
            for lv in variants:
                r = results.get((n, re, lv))
                if r is None:
                    continue
                d = diff(n, re, lv) if lv > 1 else None
                ok = "error" not in r and "error" not in lone
                rows.append("| {} | {:g} | {} | {} | {} | {} | {} | {} | {} | {} |".format(
                    n, re, "from rest" if lv == 1 else f"{lv} levels",
                    " -> ".join(str(x) for x in r.get("sizes", [])) or "-",
                    " + ".join(str(x) for x in r.get("iterations", [])) or r.get("error", "-"),
                    {True: "yes", False: "no"}.get(r.get("converged"), "-"),
                    f"{r['seconds']:.2f}" if "seconds" in r else "-",
                    f"{r['seconds'] / lone['seconds']:.2f}" if ok and lv > 1 and lone.get("seconds") else "-",
                    f"{d[0]:.1e}" if d else "-", f"{d[1]:.1e}" if d else "-"))
    return "\n".join(rows) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,128,256")
    ap.add_argument("--re", default="100,1000")
    ap.add_argument("--levels", default="2,3")
    ap.add_argument("--max-iterations", type=int, default=50000)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "fv_fsg.md"))
    ap.add_argument("--one", nargs=3, type=float, metavar=("N", "RE", "LEVELS"), help=argparse.SUPPRESS)
    ap.add_argument("--fields", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        return one(a)
    import numpy as np
    import __graft_entry__ as g
    g.build()                                     # once, here: the children find the library up to date
    sizes = [int(x) for x in a.sizes.split(",")]
    res = [float(x) for x in a.re.split(",")]
    variants = [1] + [int(x) for x in a.levels.split(",")]
    out, results, failed = Path(a.out), {}, None
    out.parent.mkdir(parents=True, exist_ok=True)
    log = out.with_suffix(".jsonl")
    log.write_text("")

    def record(c, r):
        results[c] = r
        line = json.dumps({k: v for k, v in r.items() if k != "fields"})
        print(line, flush=True)
        with log.open("a") as f:
            f.write(line + "\n")

    with tempfile.TemporaryDirectory() as tmp:
        t_start = time.perf_counter()
        for n in sorted(sizes):                   # one size at a time; its solves start together
            running = {}
            for c in [(n, re, lv) for re in res for lv in variants]:
                fields = Path(tmp) / f"{c[0]}_{int(c[1])}_{c[2]}.npz"
                cmd = [sys.executable, str(Path(__file__).resolve()), "--one", *[str(x) for x in c], "--fields", str(fields),
                       "--max-iterations", str(a.max_iterations)]
                running[c] = (subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True),
                              time.perf_counter(), fields)
            beat = time.perf_counter()
            while running:
                time.sleep(0.5)
                for c, (proc, t0, fields) in list(running.items()):
                    if proc.poll() is None:
                        if time.perf_counter() - t0 > limit(c, a.max_iterations):     # its own time limit
                            proc.kill()
                            proc.communicate()
                            failed = failed or f"{c}: no result within {limit(c, a.max_iterations):.0f} s"
                            record(c, dict(N=c[0], Re=c[1], n_levels=c[2], error="no result within its time limit"))
                            del running[c]
                        continue
                    so, se = proc.communicate()
                    lines = [x for x in so.splitlines() if x.startswith("{")]
                    if proc.returncode == 0 and lines:
                        record(c, dict(json.loads(lines[-1]), fields=str(fields)))
                    else:
                        failed = failed or f"{c}: exit {proc.returncode}\n{se[-3000:]}"
                        record(c, dict(N=c[0], Re=c[1], n_levels=c[2], error=f"exit {proc.returncode}"))
                    del running[c]
                if time.perf_counter() - beat > 60:
                    beat = time.perf_counter()
                    print(f"# {time.perf_counter() - t_start:.0f} s: N = {n}, {len(running)} running", flush=True)
            text = table(sizes, res, variants, results, np)
            out.write_text(text)
            if failed:                            # nothing more is started on the card after a solve that failed
                break
    print(text)
    if failed:
        sys.exit(f"stopped after a failed solve; the table holds what there was.  {failed}")


if __name__ == "__main__":
    main()
