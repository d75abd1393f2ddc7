#!/usr/bin/env python3
"""What does the transfer over the whole chip (``chip_transfer="tables"``, ldc_fv_wide_prolong_tables_enqueue) cost, and what
do sequencing and continuation do for wall-clustered chip trials?  Records, not promises (solvers/fv/fsg.py: sequencing is
a capability, not a saving).  Stretched trials at ``grid_stretch`` 1.5 with ``chip_grid="tables"``,
``pressure_equation="consistent"`` and ``chip_preconditioner="separable"``, TVD, 0.7 / 0.3, tolerance 1e-6:

  transfer-256    one pair 128^2 -> 256^2 through ldc_fv_prolong_tables_enqueue (one work-group) and through the new entry
                  (two launches over the chip): events around the call, best of 5, and whether the bits agree;
  transfer-1024   one pair 512^2 -> 1024^2 through the new entry;
  rest-256        256^2 at Re = 1000 from rest (profiles/fv_wide_separable.md: 13.5 s, 6290 iterations);
  seq-256         the same sequenced 64 -> 128 -> 256;
  seq-512         512^2 at Re = 1000 sequenced 128 -> 256 -> 512, with its centreline errors against Botella and Peyret;
  cont-256        256^2 at Re = 1000 continued from its own Re = 400 solution (which is solved from rest first).

    python tools/fv_wide_prolong_tables_perf.py [--steps transfer-256,...] [--tolerance 1e-6] [--out profiles/fv_wide_prolong_tables.md]

One child process per step, each under its own time limit; nothing more is started on the card after a step that failed.
Writes the Markdown to ``--out`` and one JSON line per step beside it.
"""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "02689-advancednumericalalgorithmp3_amd" / "src"), str(ROOT / "tests")]

BETA = 1.5
CHIP = dict(convection_scheme="TVD", linear_solver_tol=1e-9, grid="tanh", grid_stretch=BETA, mapping="chip",
            chip_grid="tables", pressure_equation="consistent", chip_preconditioner="separable", chip_transfer="tables")
SOLVE = dict(CHIP, alpha_uv=0.7, alpha_p=0.3, pressure_max_iters=400, tolerance=1e-6, check_every=256,
             streamfunction="wall_stretched", vortex_refine="quadratic")
# step -> seconds allowed to its child (start of the process, the eigenvectors of every level, the solve)
STEPS = {"transfer-256": 120, "transfer-1024": 180, "rest-256": 240, "seq-256": 300, "seq-512": 540, "cont-256": 360}
STATE = ("u", "v", "p", "mdot")


def timed_call(torch, stream, call, repeats=5):
    times = []
    for _ in range(repeats + 1):                  # (the first call loads the code object: not counted)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e-3)
    return times[1:]


def transfer(step):
    import numpy as np
    import torch
    from solvers.fv import ldc_fv_lib as F
    from solvers.fv.solver import FVSolver
    cn, fn = (128, 256) if step == "transfer-256" else (512, 1024)
    kw = dict(CHIP, name="fv", Re=100.0, alpha_uv=0.4, alpha_p=0.2, tolerance=1e-30, check_every=8)
    rng = np.random.default_rng(3)
    c = FVSolver(**dict(kw, nx=cn, ny=cn))
    c.set_state(*(rng.standard_normal(c.t[k].numel()) for k in STATE))
    f = FVSolver(**dict(kw, nx=fn, ny=fn))
    job, stream = [f._prolong_tables_job(c)], torch.cuda.current_stream(c.device)
    row = dict(step=step, coarse=cn, fine=fn, launches=F.lib().ldc_fv_wide_prolong_tables_launches(1))
    chip = timed_call(torch, stream, lambda: F.wide_prolong_tables_enqueue(job, stream.cuda_stream))
    row.update(chip_seconds=min(chip), chip_seconds_all=chip)
    if fn <= F.MAX_N:                             # the one-CU entry takes the same job
        got = f.state()
        cu = timed_call(torch, stream, lambda: F.prolong_tables_enqueue(job, stream.cuda_stream))
        other = f.state()
        row.update(cu_seconds=min(cu), cu_seconds_all=cu, same_bits=all(np.array_equal(got[k], other[k]) for k in STATE))
    c.close(), f.close()
    return row


def solved(step, label, s, t0, **more):
    c = s.counters()
    its = list(getattr(s, "level_iterations", None) or [s.metrics.iterations])
    return dict(step=step, start=label, N=s.nx, Re=float(s.params.Re), iterations=its, converged=bool(s.metrics.converged),
                tolerance=float(s.params.tolerance), seconds=round(time.perf_counter() - t0, 2), final_residual=float(s.metrics.final_residual),
                first_residual=float(s.history[0, 0]), mean_cg=round(c["pressure_iterations"] / max(1, c["pressure_solves"]), 2),
                pressure_caps=c["pressure_caps"], **more)


def centreline(s):
    from fv_stretched_numpy import BOTELLA_RE1000, centreline_extrema
    ny, nx = s.shape_full
    xs, ys = s.fields.x.reshape(ny, nx)[0], s.fields.y.reshape(ny, nx)[:, 0]
    ext = centreline_extrema(s.fields.u.reshape(ny, nx), s.fields.v.reshape(ny, nx), xs, ys)
    return dict(extrema=ext, centreline_errors={k: abs(abs(ext[k]) - abs(BOTELLA_RE1000[k])) for k in ext})


def start(step, cap, tolerance):
    from solvers.fv.fsg import FVFSGSolver
    from solvers.fv.solver import FVSolver
    n = int(step.split("-")[1])
    kw = dict(SOLVE, nx=n, ny=n, Re=1000.0, max_iterations=cap, tolerance=tolerance)
    t0 = time.perf_counter()
    if step.startswith("rest"):
        s = FVSolver(name="fv", **kw)
        s.set_wide_graph(True)
        s.solve()
        return solved(step, "from rest", s, t0, **centreline(s))
    if step.startswith("seq"):
        s = FVFSGSolver(name="fv_fsg", n_levels=3, coarsest_n=n // 4, **kw)
        s.set_wide_graph(True)                    # (the fine level; the coarse levels run with the library's default)
        s.solve()
        return solved(step, " -> ".join(f"{a}^2" for a, _ in s.level_sizes()), s, t0, **centreline(s))
    low = FVSolver(name="fv", **dict(kw, Re=400.0))
    low.set_wide_graph(True)
    low.solve()
    source = solved(step, "Re = 400 from rest (the source)", low, t0)
    t0 = time.perf_counter()
    s = FVSolver(name="fv", **kw)
    s.set_wide_graph(True)
    s.start_from(low)
    s.solve()
    return solved(step, "continued from Re = 400", s, t0, source=source, **centreline(s))


def child(a):
    import __graft_entry__ as g
    g.build()
    row = transfer(a.child) if a.child.startswith("transfer") else start(a.child, a.max_iterations, a.tolerance)
    print(json.dumps(row), flush=True)


def markdown(rows):
    out = ["| step | case | iterations | converged | seconds | first residual | CG per solve | centreline errors (u_min, v_max, v_min) |",
           "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        if "error" in r:
            out.append(f"| {r['step']} | {r['error']} | - | - | - | - | - | - |")
        elif r["step"].startswith("transfer"):
            out.append(f"| {r['step']} | {r['coarse']}^2 -> {r['fine']}^2, the chip entry, {r['launches']} launches | - | - | "
                       f"{r['chip_seconds']:.6f} | - | - | - |")
            if "cu_seconds" in r:
                out.append(f"| {r['step']} | the same job through the one-CU entry (same bits: {r['same_bits']}) | - | - | "
                           f"{r['cu_seconds']:.6f} | - | - | - |")
        else:
            for x in ([r["source"]] if "source" in r else []) + [r]:
                err = x.get("centreline_errors")
                out.append("| {} | N = {}, Re = {:g}, {} | {} | {} | {} | {:.3g} | {} | {} |".format(
                    x["step"], x["N"], x["Re"], x["start"], " + ".join(str(i) for i in x["iterations"]),
                    "yes" if x["converged"] else "no", x["seconds"], x["first_residual"], x["mean_cg"],
                    ", ".join(f"{err[k]:.1e}" for k in ("u_min", "v_max", "v_min")) if err else "-"))
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", default=",".join(STEPS))
    ap.add_argument("--max-iterations", type=int, default=40000)
    ap.add_argument("--tolerance", type=float, default=1e-6, help="of the start rows")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "fv_wide_prolong_tables.md"))
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    import __graft_entry__ as g
    g.build()                                     # once, here: the children find the library up to date
    out, rows, failed = Path(a.out), [], None
    out.parent.mkdir(parents=True, exist_ok=True)
    log = out.with_suffix(".jsonl")
    log.write_text("")
    for step in [x for x in a.steps.split(",") if x]:
        cmd = [sys.executable, str(Path(__file__).resolve()), "--child", step, "--max-iterations", str(a.max_iterations),
               "--tolerance", str(a.tolerance)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEPS[step])
            lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
            if r.returncode != 0 or not lines:
                failed = f"{step}: exit {r.returncode}\n{r.stderr[-3000:]}"
        except subprocess.TimeoutExpired:
            failed, lines = f"{step}: no result within {STEPS[step]} s", []
        rows.append(json.loads(lines[-1]) if lines and not failed else dict(step=step, error="failed"))
        print(json.dumps(rows[-1]), flush=True)
        with log.open("a") as f:
            f.write(json.dumps(rows[-1]) + "\n")
        out.write_text(markdown(rows))
        if failed:                                # nothing more is started on the card after a step that failed
            break
    print(markdown(rows))
    if failed:
        sys.exit(f"stopped after a failed step; the table holds what there was.  {failed}")


if __name__ == "__main__":
    main()
