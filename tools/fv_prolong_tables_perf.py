#!/usr/bin/env python3
"""What does the transfer on stretched grids (``transfer="tables"``, ldc_fv_prolong_tables_enqueue) cost, and what do
sequencing and continuation do for wall-clustered trials?  Records, not promises (solvers/fv/fsg.py: sequencing is a
capability, not a saving).  At ``grid_stretch`` 1.5 with ``pressure_equation="consistent_cu"`` and
``pressure_preconditioner="separable"``, the YAML's relaxation, TVD, tolerance 1e-6:

  transfer   256 pairs of 64^2 -> 128^2 in one call: the time of the call on the card (events around it, best of 5) against
             the same transfer through the host (download of the coarse state, the NumPy restatement, upload), one pair timed
             and multiplied;
  start      a stretched 128^2 at Re = 1000 from rest, sequenced from 64^2, and continued from its own Re = 400 solution:
             iterations and seconds;
  ladder     Re = 100 -> 400 -> 1000 -> 3200 at 64^2, every rung continued from the rung below, against every rung from rest;
             a rung that does not latch within the cap is reported as such.

    python tools/fv_prolong_tables_perf.py [--parts transfer,start,ladder] [--out profiles/fv_prolong_tables.md]

One process, one solve after another, every one under the iteration cap ``--max-iterations``; a solve that raises ends the
run, and the table holds what there was.  Writes the Markdown to ``--out`` and one JSON line per row beside it.
"""
import argparse
import json
import sys
import time
from pathlib import Path
from types import SimpleNamespace

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "02689-advancednumericalalgorithmp3_amd" / "src"), str(ROOT / "tests")]

BETA = 1.5
TANH = dict(grid="tanh", grid_stretch=BETA, transfer="tables", pressure_equation="consistent_cu",
            pressure_preconditioner="separable")
YAML = dict(convection_scheme="TVD", alpha_uv=0.4, alpha_p=0.2, linear_solver_tol=1e-9)


def transfer_rows(np, torch, FVSolver, prolong, F, pairs=256, coarse_n=64, fine_n=128, repeats=5):
    import fv_prolong_tables_numpy as T
    from fv_stretched_numpy import axis_tables, tanh_vertices
    kw = dict(YAML, **TANH, name="fv", Re=100.0, tolerance=1e-30, check_every=8)
    rng = np.random.default_rng(3)
    c = FVSolver(**dict(kw, nx=coarse_n, ny=coarse_n))
    c.set_state(*(rng.standard_normal(c.t[k].numel()) for k in ("u", "v", "p", "mdot")))
    fines = [FVSolver(**dict(kw, nx=fine_n, ny=fine_n)) for _ in range(pairs)]
    jobs = [f._prolong_tables_job(c) for f in fines]
    stream = torch.cuda.current_stream(c.device)
    times = []
    for _ in range(repeats + 1):                  # (the first call loads the code object: not counted)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        F.prolong_tables_enqueue(jobs, stream.cuda_stream)
        e1.record(stream)
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e-3)
    device_s = min(times[1:])
    t0 = time.perf_counter()
    prolong([(c, f) for f in fines])              # the same through solver.prolong: jobs, lock, one wait
    call_s = time.perf_counter() - t0

    def tables(s):
        o = SimpleNamespace(nx=s.nx, ny=s.ny, rho=1.0, Lx=1.0, Ly=1.0)
        o.xc, o.hx, o.dxf, o.gxf = axis_tables(tanh_vertices(s.nx, 1.0, BETA))
        o.yc, o.hy, o.dyf, o.gyf = axis_tables(tanh_vertices(s.ny, 1.0, BETA))
        return o
    host = []
    for _ in range(3):                            # one pair through the host: download, restatement, upload
        t0 = time.perf_counter()
        st = c.state()
        a, b = tables(c), tables(fines[0])
        a.u, a.v, a.p = (st[k].reshape(c.ny, c.nx) for k in ("u", "v", "p"))
        a.ulid = c.t["ulid"].cpu().numpy()
        T.prolong(a, b)
        fines[0].set_state(b.u, b.v, b.p, T.mdot(b))
        torch.cuda.synchronize()
        host.append(time.perf_counter() - t0)
    for s in [c] + fines:
        s.close()
    return [dict(part="transfer", pairs=pairs, coarse=coarse_n, fine=fine_n, launches=F.lib().ldc_fv_prolong_tables_launches(pairs),
                 device_seconds=device_s, device_seconds_all=times[1:], prolong_call_seconds=call_s,
                 host_seconds_one_pair=min(host), host_seconds_all_pairs=min(host) * pairs)]


def solve_row(part, label, s, t0):
    its = list(getattr(s, "level_iterations", None) or [s.metrics.iterations])
    return dict(part=part, start=label, N=s.nx, Re=float(s.params.Re), iterations=its, converged=bool(s.metrics.converged),
                seconds=round(time.perf_counter() - t0, 3), final_residual=float(s.metrics.final_residual))


def start_rows(FVSolver, FVFSGSolver, cap, n=128):
    kw = dict(YAML, **TANH, nx=n, ny=n, tolerance=1e-6, max_iterations=cap, check_every=512)
    rows = []
    t0 = time.perf_counter()
    rest = FVSolver(name="fv", Re=1000.0, **kw)
    rest.solve()
    rows.append(solve_row("start", "from rest", rest, t0))
    t0 = time.perf_counter()
    seq = FVFSGSolver(name="fv_fsg", Re=1000.0, n_levels=2, coarsest_n=16, **kw)
    seq.solve()
    rows.append(solve_row("start", f"sequenced from {n // 2}^2", seq, t0))
    t0 = time.perf_counter()
    low = FVSolver(name="fv", Re=400.0, **kw)
    low.solve()
    rows.append(solve_row("start", "Re = 400 from rest (the source below)", low, t0))
    t0 = time.perf_counter()
    cont = FVSolver(name="fv", Re=1000.0, **kw)
    cont.start_from(low)
    cont.solve()
    rows.append(solve_row("start", "continued from Re = 400", cont, t0))
    for s in (rest, seq, low, cont):
        s.close()
    return rows


def ladder_rows(FVSolver, cap, n=64, rungs=(100.0, 400.0, 1000.0, 3200.0)):
    from solvers.spectral.ldc_lib import LdcError
    kw = dict(YAML, **TANH, nx=n, ny=n, tolerance=1e-6, max_iterations=cap, check_every=512)
    rows, below = [], None
    for re in rungs:
        for label in (("from rest", "continued") if below is not None else ("from rest",)):
            t0 = time.perf_counter()
            s = FVSolver(name="fv", Re=re, **kw)
            if label == "continued":
                s.start_from(below)
            try:
                s.solve()
                rows.append(solve_row("ladder", label if label == "from rest" else f"continued from Re = {below.params.Re:g}", s, t0))
            except LdcError as exc:               # a NaN: the rung fails from this start
                rows.append(dict(part="ladder", start=label, N=n, Re=re, iterations=[], converged=False,
                                 seconds=round(time.perf_counter() - t0, 3), error=str(exc)[:80]))
                s.close()
                continue
            # the next rung continues from this rung's continued solve (the first rung: from its solve from rest), if it latched
            if (label == "continued" or below is None) and s.metrics.converged:
                if below is not None:
                    below.close()
                below = s
            else:
                s.close()
    return rows


def markdown(rows):
    out = ["| part | case | iterations | converged | seconds |", "|---|---|---|---|---|"]
    for r in rows:
        if r["part"] == "transfer":
            out.append(f"| transfer | {r['pairs']} pairs {r['coarse']}^2 -> {r['fine']}^2, {r['launches']} launches: on the card | - | - | "
                       f"{r['device_seconds']:.6f} |")
            out.append(f"| transfer | the same through solver.prolong (jobs, lock, one wait) | - | - | {r['prolong_call_seconds']:.6f} |")
            out.append(f"| transfer | through the host, one pair x {r['pairs']} | - | - | {r['host_seconds_all_pairs']:.3f} "
                       f"({r['host_seconds_one_pair']:.4f} each) |")
        else:
            out.append("| {} | N = {}, Re = {:g}, {} | {} | {} | {} |".format(
                r["part"], r["N"], r["Re"], r["start"], " + ".join(str(x) for x in r["iterations"]) or r.get("error", "-"),
                "yes" if r["converged"] else "no", r["seconds"]))
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="transfer,start,ladder")
    ap.add_argument("--max-iterations", type=int, default=60000)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "fv_prolong_tables.md"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as g
    g.build()
    from solvers.fv import ldc_fv_lib as F
    from solvers.fv.fsg import FVFSGSolver
    from solvers.fv.solver import FVSolver, prolong
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    log = out.with_suffix(".jsonl")
    log.write_text("")
    rows = []

    def record(new):
        rows.extend(new)
        with log.open("a") as f:
            for r in new:
                print(json.dumps(r), flush=True)
                f.write(json.dumps(r) + "\n")
        out.write_text(markdown(rows))
    parts = a.parts.split(",")
    if "transfer" in parts:
        record(transfer_rows(np, torch, FVSolver, prolong, F))
    if "start" in parts:
        record(start_rows(FVSolver, FVFSGSolver, a.max_iterations))
    if "ladder" in parts:
        record(ladder_rows(FVSolver, a.max_iterations))
    print(markdown(rows))


if __name__ == "__main__":
    main()
