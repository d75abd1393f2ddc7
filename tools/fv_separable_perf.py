#!/usr/bin/env python3
"""What does the separable scaled preconditioner (``pressure_preconditioner="separable"``, csrc/ldc_fv_stretched_sep.hip) buy a
stretched one-CU trial per SIMPLE iteration and to convergence?  Against the constant-coefficient preconditioner of the same
build (fv_stretched_kernel<true>: the code object of the parent commit, tools/fv_code_objects.py) and beside the uniform
kernel, in ONE process; every step that uses the GPU runs under a time limit of its own (the watchdog of
tools/fv_stretched_perf.py, whose method this follows).

    python tools/fv_separable_perf.py [--parts a,c] [--cost-sizes 32,64,128] [--out profiles/fv_separable.md]

(a) Cost: milliseconds per SIMPLE iteration of 1 and of 256 trials of N x N cells per launch, from rest at Re = 100 with the
    YAML's settings, consistent_cu and tolerance 1e-30: the uniform grid, tanh 1.5 with "laplacian" and tanh 1.5 with
    "separable" in turns within every round; median and range over ``--rounds`` timed chunks (wall clock around the launch and
    its wait; the first chunk of every group is not timed), with the CG iterations per pressure solve beside them.
(c) Wall time of lone trials to tolerance 1e-7: Re = 1000, TVD, 0.7 / 0.3, tanh 1.5, both preconditioners, 64 x 64 and 128 x 128.

The tables go between the two marker lines of ``--out`` (the rest of that file is kept), one JSON line per figure beside it.
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "02689-advancednumericalalgorithmp3_amd" / "src"), str(ROOT / "tests"),
                str(ROOT / "tools")]

from fv_stretched_perf import RE1000, YAML, limit, splice, table_row  # noqa: E402

BEGIN, END = "<!-- fv_separable_perf: tables -->", "<!-- fv_separable_perf: end -->"
CHUNK = {32: 256, 64: 64, 128: 16}
TANH = dict(grid="tanh", grid_stretch=1.5)
GRIDS = (("uniform", {}), ("tanh 1.5, laplacian", dict(TANH, pressure_preconditioner="laplacian")),
         ("tanh 1.5, separable", dict(TANH, pressure_preconditioner="separable")))


def cost(FVSolver, advance, n, n_trials, rounds, step_limit):
    k = CHUNK.get(n, 8)
    kw = dict(YAML, nx=n, ny=n, Re=100.0, tolerance=1e-30, max_iterations=10**9, check_every=k,
              pressure_equation="consistent_cu")
    with limit(step_limit, f"(a) N = {n}: {n_trials} trials per row, set-up and warm chunk"):
        groups = {name: [FVSolver(**dict(kw, **g)) for _ in range(n_trials)] for name, g in GRIDS}
        for ss in groups.values():
            for s in ss:
                s._begin(1e-30)
            advance(ss, k)
    c0 = {name: [s.counters() for s in ss] for name, ss in groups.items()}
    times = {name: [] for name in groups}
    with limit(step_limit, f"(a) N = {n}, {n_trials} trials: {rounds} timed chunks of {k} iterations per row"):
        for _ in range(rounds):
            for name, ss in groups.items():
                t0 = time.perf_counter()
                advance(ss, k)
                times[name].append(1e3 * (time.perf_counter() - t0) / k)
    out = dict(part="a", N=n, trials=n_trials, chunk=k, rounds=rounds)
    for name, ss in groups.items():
        cs, t, its = [s.counters() for s in ss], times[name], rounds * k * n_trials
        assert all(c["iterations"] == (rounds + 1) * k and c["nan"] == 0 and c["pressure_caps"] == 0 for c in cs)
        out[name] = dict(ms_median=round(statistics.median(t), 4), ms_min=round(min(t), 4), ms_max=round(max(t), 4),
                         bicgstab=round(sum(c["linear_iterations"] - b["linear_iterations"] for c, b in zip(cs, c0[name])) / its, 1),
                         cg=round(sum(c["pressure_iterations"] - b["pressure_iterations"] for c, b in zip(cs, c0[name])) / its, 1))
        for s in ss:
            s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="a,c")
    ap.add_argument("--cost-sizes", default="32,64,128")
    ap.add_argument("--cost-trials", default="1,256")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--lone-sizes", default="64,128")
    ap.add_argument("--step-limit", type=float, default=300.0, help="seconds a single GPU step may take")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "fv_separable.md"))
    a = ap.parse_args()
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    import __graft_entry__ as g
    g.build()
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
        rows = ["| N | trials per launch | grid, preconditioner | ms / iteration (min ... max) | BiCGSTAB / iteration | CG / solve | "
                "ms / uniform | ms / laplacian |", "|---|---|---|---|---|---|---|---|"]
        for n in [int(x) for x in a.cost_sizes.split(",") if x]:
            for t in [int(x) for x in a.cost_trials.split(",") if x]:
                r = cost(FVSolver, advance, n, t, a.rounds, a.step_limit)
                record(r)
                for name, _ in GRIDS:
                    d = r[name]
                    rows.append(f"| {n} | {t} | {name} | {d['ms_median']:.3f} ({d['ms_min']:.3f} ... {d['ms_max']:.3f}) | "
                                f"{d['bicgstab']} | {d['cg']} | {d['ms_median'] / r['uniform']['ms_median']:.2f} | "
                                f"{d['ms_median'] / r['tanh 1.5, laplacian']['ms_median']:.2f} |")
        body += ("(a) Cost per SIMPLE iteration, Re = 100 from rest, YAML settings, consistent_cu, all trials of a row in one "
                 "launch:\n\n" + "\n".join(rows) + "\n\n")
    if "c" in parts:
        rows = ["| trial | preconditioner | outer its | seconds | ms / iteration | PCG its mean (caps) | errors (u_min, v_max, v_min) |",
                "|---|---|---|---|---|---|---|"]
        for n in [int(x) for x in a.lone_sizes.split(",") if x]:
            for pre in ("laplacian", "separable"):
                with limit(a.step_limit, f"(c) tanh 1.5, {n}², {pre}, to tolerance, alone"):
                    s = FVSolver(**dict(RE1000, nx=n, ny=n, **TANH, pressure_preconditioner=pre))
                    t0 = time.perf_counter()
                    s.solve()
                    r = dict(part="c", preconditioner=pre, **table_row(s, time.perf_counter() - t0))
                    s.close()
                record(r)
                rows.append(f"| tanh 1.5, {n}² | {pre} | {r['iterations']}{'' if r['converged'] else ' (cap)'} | {r['seconds']:.2f} | "
                            f"{1e3 * r['seconds'] / r['iterations']:.2f} | {r['cg_mean']} ({r['caps']}) | "
                            + ", ".join(f"{e:.1e}" for e in r["errors"]) + " |")
        body += ("(c) Wall time of lone trials to tolerance 1e-7 (Re = 1000, TVD, consistent_cu, 0.7 / 0.3, pressure_tol 1e-8):\n\n"
                 + "\n".join(rows) + "\n\n")
    splice(out, BEGIN, END, body)


if __name__ == "__main__":
    main()
