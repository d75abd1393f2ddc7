#!/usr/bin/env python3
"""What does the consistent pressure equation cost a one-CU trial per iteration, and what does a sweep gain from it?
``mapping="cu"`` with ``pressure_equation="reference"`` against ``"consistent_cu"``, TVD (the YAML's settings), in ONE
process; every step that uses the GPU runs under a time limit of its own (a watchdog that ends the process).

    python tools/fv_cu_pressure_perf.py [--cost-sizes 32,64,128] [--trials 256] [--sweep-trials 64,256]
                                        [--out profiles/fv_cu_pressure.md]

(a) Cost: milliseconds per launch-iteration of ``--trials`` trials of N x N cells from rest at Re = 100 and tolerance
    1e-30, one work-group each in one launch, both modes in turns, ``--rounds`` timed chunks each; median and range; the
    BiCGSTAB iterations per SIMPLE iteration and the CG iterations per pressure solve beside them (means over the trials).
    The reference rows are the path of the parent commit (fv_kernel<false>, whose code object has not changed).
(b) The sweep: T trials of N = 64 with Re = 100, 400, 1000 in turns (relaxation 0.7 / 0.3, tolerance 1e-6, cap
    ``--max-iterations``) to tolerance, three ways: ``cu`` + ``consistent_cu``, ``cu`` + ``reference``, and
    ``shared`` + ``consistent`` in batches of ``--shared-batch`` trials one after the other.  Seconds, how many trials
    latched, hit the cap or stopped on a NaN, and their iterations.  A way that cannot be expected to fit what is left of
    ``--seconds`` is listed as not measured.

The tables go between the two marker lines of ``--out`` (the rest of that file is kept) and one JSON line per figure
beside it.
"""
import argparse
import faulthandler
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "02689-advancednumericalalgorithmp3_amd" / "src")]

YAML = dict(name="fv", convection_scheme="TVD", alpha_uv=0.4, alpha_p=0.2, linear_solver_tol=1e-9)
BEGIN, END = "<!-- fv_cu_pressure_perf: tables -->", "<!-- fv_cu_pressure_perf: end -->"
CHUNK = {32: 64, 64: 32, 128: 8}                  # iterations per timed chunk of (a)
MODES = ("reference", "consistent_cu")
SWEEP_RE = (100.0, 400.0, 1000.0)
WAYS = (("cu", "consistent_cu"), ("cu", "reference"), ("shared", "consistent"))


class limit:
    """A GPU step under its own time limit: past it the stacks are printed and the process ends (nothing more is started
    on the card)."""

    def __init__(self, seconds, what):
        self.seconds, self.what = seconds, what

    def __enter__(self):
        print(f"[step] {self.what} (limit {self.seconds:.0f} s)", flush=True)
        faulthandler.dump_traceback_later(self.seconds, exit=True)

    def __exit__(self, *exc):
        faulthandler.cancel_dump_traceback_later()


def cost(FVSolver, advance, n, n_trials, rounds, step_limit):
    k = CHUNK.get(n, 8)
    kw = dict(YAML, nx=n, ny=n, Re=100.0, tolerance=1e-30, max_iterations=10**9, check_every=k, mapping="cu")
    with limit(step_limit, f"(a) N = {n}: {n_trials} trials per mode, set-up and warm chunk"):
        groups = {m: [FVSolver(**dict(kw, pressure_equation=m)) for _ in range(n_trials)] for m in MODES}
        for ss in groups.values():
            for s in ss:
                s._begin(1e-30)
            advance(ss, k)                                 # (warm: the first launch of each kernel is paid)
    c0 = {m: [s.counters() for s in ss] for m, ss in groups.items()}
    times = {m: [] for m in MODES}
    with limit(step_limit, f"(a) N = {n}: {rounds} timed chunks of {k} iterations per mode"):
        for _ in range(rounds):
            for m, ss in groups.items():                   # in turns
                t0 = time.perf_counter()
                advance(ss, k)                             # (one launch, then the copy of ctrl: a synchronise)
                times[m].append(1e3 * (time.perf_counter() - t0) / k)
    out = dict(N=n, trials=n_trials, chunk=k, rounds=rounds)
    for m, ss in groups.items():
        cs, t = [s.counters() for s in ss], times[m]
        assert all(c["iterations"] == (rounds + 1) * k and c["nan"] == 0 for c in cs)
        its = rounds * k * n_trials
        d = dict(ms_median=round(statistics.median(t), 4), ms_min=round(min(t), 4), ms_max=round(max(t), 4),
                 bicgstab_per_iteration=round(sum(c["linear_iterations"] - b["linear_iterations"]
                                                  for c, b in zip(cs, c0[m])) / its, 1))
        if m == "consistent_cu":
            d.update(cg_per_solve=round(sum(c["pressure_iterations"] - b["pressure_iterations"]
                                            for c, b in zip(cs, c0[m])) / its, 1),
                     caps=sum(c["pressure_caps"] for c in cs))
        out[m] = d
        for s in ss:
            s.close()
    return out


def sweep(Batched, n, n_trials, mapping, mode, cap, shared_batch, step_limit):
    trials = [dict(YAML, nx=n, ny=n, Re=SWEEP_RE[q % len(SWEEP_RE)], alpha_uv=0.7, alpha_p=0.3, tolerance=1e-6,
                   max_iterations=cap, check_every=256, mapping=mapping, pressure_equation=mode)
              for q in range(n_trials)]
    size = shared_batch if mapping == "shared" else n_trials
    out = dict(N=n, trials=n_trials, mapping=mapping, mode=mode, batches=0, seconds=0.0, latched=0, capped=0, nan=0,
               iterations=0, iterations_max=0, per_re={})
    for lo in range(0, n_trials, size):
        part = trials[lo: lo + size]
        with limit(step_limit, f"(b) {n_trials} trials, {mapping} + {mode}: batch of {len(part)} from trial {lo}"):
            batch = Batched(part)
            t0 = time.perf_counter()
            batch.solve()
            out["seconds"] += time.perf_counter() - t0
            out["batches"] += 1
            for q, s in enumerate(batch.solvers):
                its = int(s.counters()["iterations"])
                end = "nan" if q in batch.errors else "latched" if s.metrics.converged else "capped"
                out[end] += 1
                out["iterations"] += its
                out["iterations_max"] = max(out["iterations_max"], its)
                r = out["per_re"].setdefault(f"{s.params.Re:g}", dict(latched=0, capped=0, nan=0, iterations=[]))
                r[end] += 1
                r["iterations"].append(its)
            batch.close()
    for r in out["per_re"].values():
        r["iterations"] = [min(r["iterations"]), max(r["iterations"])]
    out["seconds"] = round(out["seconds"], 3)
    return out


def cost_table(costs):
    rows = ["| N | trials | chunk x rounds | mode | ms / launch-iteration (min ... max) | BiCGSTAB / iteration | CG / solve "
            "(caps) | ms / reference |", "|---|---|---|---|---|---|---|---|"]
    for r in costs:
        for m in MODES:
            d = r[m]
            cg = f"{d['cg_per_solve']} ({d['caps']})" if "cg_per_solve" in d else "-"
            rows.append(f"| {r['N']} | {r['trials']} | {r['chunk']} x {r['rounds']} | {m} | {d['ms_median']:.3f} "
                        f"({d['ms_min']:.3f} ... {d['ms_max']:.3f}) | {d['bicgstab_per_iteration']} | {cg} | "
                        f"{d['ms_median'] / r['reference']['ms_median']:.2f} |")
    return "\n".join(rows) + "\n"


def sweep_table(sweeps, skipped):
    rows = ["| trials | mapping + equation | batches | seconds | latched / capped / NaN | iterations in all (most of one "
            "trial) | per Re: latched / capped / NaN, iterations min ... max |", "|---|---|---|---|---|---|---|"]
    for r in sweeps:
        per = "; ".join(f"Re {re}: {d['latched']} / {d['capped']} / {d['nan']}, {d['iterations'][0]} ... {d['iterations'][1]}"
                        for re, d in sorted(r["per_re"].items(), key=lambda kv: float(kv[0])))
        rows.append(f"| {r['trials']} | {r['mapping']} + {r['mode']} | {r['batches']} | {r['seconds']:.2f} | {r['latched']} / "
                    f"{r['capped']} / {r['nan']} | {r['iterations']} ({r['iterations_max']}) | {per} |")
    for t, mapping, mode, why in skipped:
        rows.append(f"| {t} | {mapping} + {mode} | - | not measured ({why}) | - | - | - |")
    return "\n".join(rows) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cost-sizes", default="32,64,128")
    ap.add_argument("--trials", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sweep-trials", default="64,256")
    ap.add_argument("--sweep-n", type=int, default=64)
    ap.add_argument("--shared-batch", type=int, default=64)
    ap.add_argument("--max-iterations", type=int, default=20000)
    ap.add_argument("--step-limit", type=float, default=240.0, help="seconds a single GPU step may take")
    ap.add_argument("--seconds", type=float, default=600.0, help="(b) starts no way it cannot expect to finish within this")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "fv_cu_pressure.md"))
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from solvers.fv.batched import BatchedFVSolver
    from solvers.fv.solver import FVSolver, advance
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
    costs, sweeps, skipped = [], [], []
    for n in [int(x) for x in a.cost_sizes.split(",") if x]:
        costs.append(cost(FVSolver, advance, n, a.trials, a.rounds, a.step_limit))
        record(costs[-1])
    # seconds per launch-iteration of N = sweep_n on cu, from (a) where it was run: what a way of (b) may be expected to take
    per_it = {m: 1e-3 * r[m]["ms_median"] for r in costs if r["N"] == a.sweep_n for m in MODES}
    for t in [int(x) for x in a.sweep_trials.split(",") if x]:
        for mapping, mode in WAYS:
            left = a.seconds - (time.perf_counter() - t_start)
            rounds = -(-t // 256)                          # launches of 256 work-groups: one CU each
            guess = (per_it.get(mode, 1e-3) * rounds * (a.max_iterations if mode == "reference" else 3000)
                     if mapping == "cu" else 30.0 * -(-t // a.shared_batch))
            if guess > left:
                skipped.append((t, mapping, mode, f"{guess:.0f} s expected, {left:.0f} s left"))
                record(dict(trials=t, mapping=mapping, mode=mode, not_run=skipped[-1][3]))
                continue
            sweeps.append(sweep(BatchedFVSolver, a.sweep_n, t, mapping, mode, a.max_iterations, a.shared_batch, a.step_limit))
            record(sweeps[-1])
    text = (f"{BEGIN}\n(a) Cost per SIMPLE iteration on `cu`, Re = 100 from rest, all trials of a row in one launch:\n\n"
            f"{cost_table(costs)}\n(b) The sweep: N = {a.sweep_n}, Re = 100, 400, 1000 in turns, 0.7 / 0.3, to tolerance 1e-6 "
            f"(cap {a.max_iterations} iterations; `shared` in batches of {a.shared_batch}):\n\n{sweep_table(sweeps, skipped)}{END}\n")
    old = out.read_text() if out.exists() else ""
    if BEGIN in old and END in old:
        text = old[: old.index(BEGIN)] + text + old[old.index(END) + len(END):].lstrip("\n")
    else:
        text = old + ("\n" if old and not old.endswith("\n") else "") + text
    out.write_text(text)
    print(text)


if __name__ == "__main__":
    main()
