#!/usr/bin/env python3
"""What does a wall-clustered grid cost a one-CU trial per iteration, and what does it buy?  ``grid="tanh"``
(csrc/ldc_fv_stretched.hip) against the uniform kernels (fv_kernel, fv_cu_pressure_kernel: the code objects of the parent
commit, tools/fv_code_objects.py), in ONE process; every step that uses the GPU runs under a time limit of its own (a
watchdog that ends the process).

    python tools/fv_stretched_perf.py [--parts a,b,c] [--cost-sizes 32,64,128] [--out profiles/fv_stretched.md]
    python tools/fv_stretched_perf.py --cpu [--table-sizes 32,64]        (the table of (b) by the NumPy restatement, no GPU)

(a) Cost: milliseconds per SIMPLE iteration of 1 and of 256 trials of N x N cells per launch, from rest at Re = 100 with the
    YAML's settings and tolerance 1e-30, uniform and tanh (beta 1.5) in turns, both pressure equations; median and range over
    ``--rounds`` timed chunks, with the BiCGSTAB iterations per SIMPLE iteration and the CG iterations per pressure solve
    beside them (the grids differ in both, so the ratio is the cost of a trial's iteration, not of the kernel's arithmetic).
(b) The table: Re = 1000, TVD, consistent_cu, 0.7 / 0.3, linear_solver_tol 1e-9, tolerance 1e-7; cells x beta; outer
    iterations, CG iterations per solve, cap hits and the errors of the three centreline extrema against Botella & Peyret
    (a parabola through the three cells around each extremum).  All trials advance together in one batch.
(c) Wall time to the same error: a lone stretched 64 x 64 against a lone uniform 128 x 128, and 128 x 128 against 256 x 256,
    the settings of (b).

The tables go between the two marker lines of ``--out`` (the rest of that file is kept), one JSON line per figure beside it.
"""
import argparse
import faulthandler
import json
import statistics
import sys
import threading
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "02689-advancednumericalalgorithmp3_amd" / "src"), str(ROOT / "tests")]

from fv_stretched_numpy import BOTELLA_RE1000, FVStretchedState, centreline_extrema  # noqa: E402

YAML = dict(name="fv", convection_scheme="TVD", alpha_uv=0.4, alpha_p=0.2, linear_solver_tol=1e-9)
RE1000 = dict(name="fv", Re=1000.0, convection_scheme="TVD", alpha_uv=0.7, alpha_p=0.3, linear_solver_tol=1e-9,
              pressure_equation="consistent_cu", pressure_tol=1e-8, pressure_max_iters=200, tolerance=1e-7,
              max_iterations=20000, check_every=512)
BEGIN, END = "<!-- fv_stretched_perf: tables -->", "<!-- fv_stretched_perf: end -->"
CPU_BEGIN, CPU_END = "<!-- fv_stretched_perf: cpu table -->", "<!-- fv_stretched_perf: cpu end -->"
CHUNK = {32: 64, 64: 32, 128: 8}
MODES = ("reference", "consistent_cu")
GRIDS = (("uniform", {}), ("tanh 1.5", dict(grid="tanh", grid_stretch=1.5)))
BETAS = (0.0, 1.0, 1.5)


class limit:
    """A GPU step under its own time limit: past it the stacks are printed and the process ends (nothing more is started
    on the card)."""

    def __init__(self, seconds, what):
        self.seconds, self.what = seconds, what

    def __enter__(self):
        print(f"[step] {self.what} (limit {self.seconds:.0f} s)", flush=True)
        faulthandler.dump_traceback_later(self.seconds, exit=True)
        self.over, t0 = threading.Event(), time.perf_counter()

        def beat():                                # (a long lone solve says nothing by itself)
            while not self.over.wait(60.0):
                print(f"[step] {self.what}: {time.perf_counter() - t0:.0f} s", flush=True)
        threading.Thread(target=beat, daemon=True).start()

    def __exit__(self, *exc):
        self.over.set()
        faulthandler.cancel_dump_traceback_later()


def errors_of(u, v, xs, ys):
    ext = centreline_extrema(u, v, xs, ys)
    return [abs(abs(ext[k]) - abs(BOTELLA_RE1000[k])) for k in ("u_min", "v_max", "v_min")]


def cost(FVSolver, advance, n, n_trials, mode, rounds, step_limit):
    k = CHUNK.get(n, 8)
    kw = dict(YAML, nx=n, ny=n, Re=100.0, tolerance=1e-30, max_iterations=10**9, check_every=k, pressure_equation=mode)
    with limit(step_limit, f"(a) N = {n}, {mode}: {n_trials} trials per grid, set-up and warm chunk"):
        groups = {name: [FVSolver(**dict(kw, **g)) for _ in range(n_trials)] for name, g in GRIDS}
        for ss in groups.values():
            for s in ss:
                s._begin(1e-30)
            advance(ss, k)
    c0 = {name: [s.counters() for s in ss] for name, ss in groups.items()}
    times = {name: [] for name in groups}
    with limit(step_limit, f"(a) N = {n}, {mode}: {rounds} timed chunks of {k} iterations per grid"):
        for _ in range(rounds):
            for name, ss in groups.items():
                t0 = time.perf_counter()
                advance(ss, k)
                times[name].append(1e3 * (time.perf_counter() - t0) / k)
    out = dict(part="a", N=n, trials=n_trials, mode=mode, chunk=k, rounds=rounds)
    for name, ss in groups.items():
        cs, t, its = [s.counters() for s in ss], times[name], rounds * k * n_trials
        assert all(c["iterations"] == (rounds + 1) * k and c["nan"] == 0 for c in cs)
        d = dict(ms_median=round(statistics.median(t), 4), ms_min=round(min(t), 4), ms_max=round(max(t), 4),
                 bicgstab=round(sum(c["linear_iterations"] - b["linear_iterations"] for c, b in zip(cs, c0[name])) / its, 1))
        if mode == "consistent_cu":
            d["cg"] = round(sum(c["pressure_iterations"] - b["pressure_iterations"] for c, b in zip(cs, c0[name])) / its, 1)
        out[name] = d
        for s in ss:
            s.close()
    return out


def table_row(s, seconds=None):
    c = s.counters()
    ny, nx = s.shape_full
    xs, ys = s.fields.x.reshape(ny, nx)[0], s.fields.y.reshape(ny, nx)[:, 0]
    beta = float(s.params.grid_stretch) if s.params.grid == "tanh" else 0.0
    r = dict(cells=nx, beta=beta, h_wall=round(float(xs[0]) * 2 * nx, 3), converged=bool(s.metrics.converged),
             iterations=int(c["iterations"]), cg_mean=round(c["pressure_iterations"] / max(1, c["pressure_solves"]), 1),
             caps=int(c["pressure_caps"]), errors=errors_of(s.fields.u.reshape(ny, nx), s.fields.v.reshape(ny, nx), xs, ys))
    if seconds is not None:
        r["seconds"] = round(seconds, 2)
    return r


def grid_of(beta):
    return dict(grid="tanh", grid_stretch=beta) if beta else {}


def cpu_table(sizes, out):
    rows = []
    for n in sizes:
        for beta in BETAS:
            s = FVStretchedState(n, n, 1000.0, alpha_uv=0.7, alpha_p=0.3, linear_solver_tol=1e-9, convection_scheme="TVD",
                                 grid_stretch=beta, pressure_equation="consistent", pressure_tol=1e-8, pressure_max_iters=200)
            t0 = time.time()
            rec = s.run(20000, tol=1e-7)
            rows.append(dict(part="cpu", cells=n, beta=beta, h_wall=round(float(s.hx[0]) * n, 3), iterations=len(rec),
                             cg_mean=round(float(np.mean(s.cg_iters)), 1), cg_max=int(max(s.cg_iters)), caps=int(s.cg_caps),
                             errors=errors_of(s.u, s.v, s.xc, s.yc), seconds=round(time.time() - t0, 1)))
            print(json.dumps(rows[-1]), flush=True)
    text = ["| cells | beta | h_wall / h_uniform | outer its | PCG its mean / max (caps) | errors (u_min, v_max, v_min) |",
            "|---|---|---|---|---|---|"]
    for r in rows:
        text.append(f"| {r['cells']}² | {r['beta']:g} | {r['h_wall']} | {r['iterations']} | {r['cg_mean']} / {r['cg_max']} "
                    f"({r['caps']}) | " + ", ".join(f"{e:.1e}" for e in r["errors"]) + " |")
    splice(out, CPU_BEGIN, CPU_END, "The table by the NumPy restatement (tests/fv_stretched_numpy.py; beta 0 through the "
           "stretched statements), on the CPU:\n\n" + "\n".join(text) + "\n")


def splice(out, begin, end, body):
    text = f"{begin}\n{body}{end}\n"
    old = out.read_text() if out.exists() else ""
    if begin in old and end in old:
        text = old[: old.index(begin)] + text + old[old.index(end) + len(end):].lstrip("\n")
    else:
        text = old + ("\n" if old and not old.endswith("\n") else "") + text
    out.write_text(text)
    print(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--cost-sizes", default="32,64,128")
    ap.add_argument("--cost-trials", default="1,256")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--table-sizes", default="32,64")
    ap.add_argument("--parity", default="64:128,128:256", help="stretched:uniform sizes of (c)")
    ap.add_argument("--step-limit", type=float, default=300.0, help="seconds a single GPU step may take")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "fv_stretched.md"))
    a = ap.parse_args()
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    if a.cpu:
        cpu_table([int(x) for x in a.table_sizes.split(",") if x], out)
        return
    import __graft_entry__ as g
    g.build()
    from solvers.fv.batched import BatchedFVSolver
    from solvers.fv.solver import FVSolver, advance
    log = out.with_suffix(".jsonl")
    log.write_text("")

    def record(r):
        line = json.dumps(r)
        print(line, flush=True)
        with log.open("a") as f:
            f.write(line + "\n")

    parts = a.parts.split(",")
    body = ""
    if "a" in parts:
        rows = ["| N | trials per launch | equation | grid | ms / iteration (min ... max) | BiCGSTAB / iteration | CG / solve | "
                "ms / uniform |", "|---|---|---|---|---|---|---|---|"]
        for n in [int(x) for x in a.cost_sizes.split(",") if x]:
            for t in [int(x) for x in a.cost_trials.split(",") if x]:
                for mode in MODES:
                    r = cost(FVSolver, advance, n, t, mode, a.rounds, a.step_limit)
                    record(r)
                    for name, _ in GRIDS:
                        d = r[name]
                        rows.append(f"| {n} | {t} | {mode} | {name} | {d['ms_median']:.3f} ({d['ms_min']:.3f} ... {d['ms_max']:.3f}) "
                                    f"| {d['bicgstab']} | {d.get('cg', '-')} | {d['ms_median'] / r['uniform']['ms_median']:.2f} |")
        body += ("(a) Cost per SIMPLE iteration, Re = 100 from rest, YAML settings, all trials of a row in one launch:\n\n"
                 + "\n".join(rows) + "\n\n")
    if "b" in parts:
        sizes = [int(x) for x in a.table_sizes.split(",") if x]
        trials = [dict(RE1000, nx=n, ny=n, **grid_of(beta)) for n in sizes for beta in BETAS]
        with limit(a.step_limit, f"(b) {len(trials)} trials to tolerance in one batch"):
            batch = BatchedFVSolver(trials)
            t0 = time.perf_counter()
            batch.solve()
            seconds = time.perf_counter() - t0
        rows = ["| cells | beta | h_wall / h_uniform | outer its | PCG its mean (caps) | errors (u_min, v_max, v_min) |",
                "|---|---|---|---|---|---|"]
        for s in batch.solvers:
            r = dict(part="b", **table_row(s))
            record(r)
            rows.append(f"| {r['cells']}² | {r['beta']:g} | {r['h_wall']} | {r['iterations']}{'' if r['converged'] else ' (cap)'} | "
                        f"{r['cg_mean']} ({r['caps']}) | " + ", ".join(f"{e:.1e}" for e in r["errors"]) + " |")
        assert not batch.errors, batch.errors
        batch.close()
        body += (f"(b) Re = 1000, TVD, consistent_cu, 0.7 / 0.3, tolerance 1e-7, on the card (one batch of {len(trials)} trials, "
                 f"{seconds:.1f} s; beta 0 is the uniform kernel):\n\n" + "\n".join(rows) + "\n\n")
    if "c" in parts:
        rows = ["| trial | outer its | seconds | ms / iteration | PCG its mean (caps) | errors (u_min, v_max, v_min) |",
                "|---|---|---|---|---|---|"]
        for pair in a.parity.split(","):
            ns, nu = (int(x) for x in pair.split(":"))
            for n, grid, name in ((ns, grid_of(1.5), f"tanh 1.5, {ns}²"), (nu, {}, f"uniform, {nu}²")):
                with limit(a.step_limit, f"(c) {name} to tolerance, alone"):
                    s = FVSolver(**dict(RE1000, nx=n, ny=n, **grid))
                    t0 = time.perf_counter()
                    s.solve()
                    r = dict(part="c", name=name, **table_row(s, time.perf_counter() - t0))
                    s.close()
                record(r)
                rows.append(f"| {name} | {r['iterations']}{'' if r['converged'] else ' (cap)'} | {r['seconds']:.2f} | "
                            f"{1e3 * r['seconds'] / r['iterations']:.2f} | {r['cg_mean']} ({r['caps']}) | "
                            + ", ".join(f"{e:.1e}" for e in r["errors"]) + " |")
        body += "(c) Wall time of lone trials to tolerance 1e-7, the settings of (b):\n\n" + "\n".join(rows) + "\n\n"
    splice(out, BEGIN, END, body)


if __name__ == "__main__":
    main()
