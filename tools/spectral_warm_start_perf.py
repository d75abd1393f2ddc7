#!/usr/bin/env python3
"""What does ``initial_guess="fv"`` buy a spectral solve?  ONE process, per (N, Re):

  rest     ``SGSolver.solve()`` with the default keys -- the code path of the parent commit, the baseline of every time;
  fv       the same trial with ``initial_guess="fv"`` at seed tolerances 1e-4 (the default) and 1e-6: spectral iterations,
           the seed's cells, iterations and wall time, the wall time of the spectral part, and the maximum-norm distance
           of the converged u, v from the from-rest fields.

    python tools/spectral_warm_start_perf.py [--sizes 32,64,128] [--re 100,400,1000] [--tolerance 1e-6]
                                             [--budget-seconds 600] [--max-iterations 5000000] [--out FILE.md]
                                             [--reference-tolerance 1e-9]

Cases run in order of size; a case is started only while the budget lasts, and every case that did not run is named.
A solve that goes NaN stops early (``nan_guard``) and is reported as such.  With ``--reference-tolerance`` every case
is also solved (seeded) to that tolerance, and the distances of the from-rest and the seeded fields from it are listed:
which of the two paths the stop rule ends nearer to the fixed point.  Appends Markdown to ``--out``.
"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "02689-advancednumericalalgorithmp3_amd" / "src")]

YAML = dict(name="spectral", basis_type="chebyshev", CFL=1.5, beta_squared=5.0, corner_treatment="smoothing",
            corner_smoothing=0.15, multigrid="none", nan_guard=True)
SEED_TOLERANCES = (1e-4, 1e-6)


def solve(SGSolver, kw):
    s = SGSolver(**kw)
    t0 = time.perf_counter()
    s.solve()
    wall = time.perf_counter() - t0
    m, info = s.metrics, s.initial_guess_info
    out = dict(iterations=int(m.iterations), converged=bool(m.converged), wall=wall, metrics_wall=float(m.wall_time_seconds),
               finite=bool(np.all(np.isfinite(s.fields.u))), u=s.fields.u.copy(), v=s.fields.v.copy(), info=info,
               mode=int(s.kernel_mode))
    s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="32,64,128")
    ap.add_argument("--re", default="100,400,1000")
    ap.add_argument("--tolerance", type=float, default=1e-6)
    ap.add_argument("--budget-seconds", type=float, default=600.0)
    ap.add_argument("--max-iterations", type=int, default=5_000_000)
    ap.add_argument("--reference-tolerance", type=float, default=0.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import __graft_entry__ as g
    g.build()
    from solvers.spectral.sg import SGSolver

    cases = [(n, re) for n in (int(v) for v in a.sizes.split(",")) for re in (float(v) for v in a.re.split(","))]
    lines = ["", f"### `tools/spectral_warm_start_perf.py` (tolerance {a.tolerance:g}, cap {a.max_iterations} iterations)", "",
             "| N | Re | kernel | from rest: iterations | s | seed tol | seed cells | seed iterations | seed s | "
             "spectral iterations | spectral s | total s | ratio (iterations) | ratio (time) | max distance u, v |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    skipped, refs, t_start = [], [], time.perf_counter()
    solve(SGSolver, dict(YAML, Re=100.0, nx=16, ny=16, tolerance=1e-3, max_iterations=2000, initial_guess="fv"))      # warm both paths
    for q, (n, re) in enumerate(cases):
        if time.perf_counter() - t_start > a.budget_seconds:
            skipped = cases[q:]
            break
        kw = dict(YAML, Re=re, nx=n, ny=n, tolerance=a.tolerance, max_iterations=a.max_iterations)
        rest = solve(SGSolver, kw)
        state = "" if rest["converged"] else (" (NaN)" if not rest["finite"] else " (not converged)")
        seeded = {}
        print(f"N={n} Re={re:g} rest: {rest['iterations']}{state} in {rest['wall']:.2f} s", flush=True)
        for tol in SEED_TOLERANCES:
            if time.perf_counter() - t_start > a.budget_seconds:
                skipped.append((n, re, tol))
                continue
            fv = solve(SGSolver, dict(kw, initial_guess="fv", initial_guess_tolerance=tol))
            info = fv["info"]
            both = rest["converged"] and fv["converged"]
            dist = max(float(np.max(np.abs(fv["u"] - rest["u"]))), float(np.max(np.abs(fv["v"] - rest["v"])))) if both else float("nan")
            fstate = "" if fv["converged"] else (" (NaN)" if not fv["finite"] else " (not converged)")
            seeded[tol] = fv
            used = "" if info["used"] else " (failed: from rest)"
            print(f"N={n} Re={re:g} fv {tol:g}: seed {info['iterations']}{used} in {info['wall_time_seconds']:.2f} s, spectral "
                  f"{fv['iterations']}{fstate}, total {fv['wall']:.2f} s, distance {dist:.2e}", flush=True)
            lines.append(f"| {n} | {re:g} | {rest['mode']} | {rest['iterations']}{state} | {rest['wall']:.2f} | {tol:g} | "
                         f"{info['cells'][0]} x {info['cells'][1]} | {info['iterations']}{used} | {info['wall_time_seconds']:.2f} | "
                         f"{fv['iterations']}{fstate} | {fv['metrics_wall'] - info['wall_time_seconds']:.2f} | {fv['wall']:.2f} | "
                         f"{fv['iterations'] / max(1, rest['iterations']):.2f} | {fv['wall'] / rest['wall']:.2f} | {dist:.1e} |")
        if a.reference_tolerance > 0 and rest["converged"] and time.perf_counter() - t_start <= a.budget_seconds:
            ref = solve(SGSolver, dict(kw, tolerance=a.reference_tolerance, initial_guess="fv"))
            far = lambda r: max(float(np.max(np.abs(r["u"] - ref["u"]))), float(np.max(np.abs(r["v"] - ref["v"]))))      # noqa: E731
            row = (f"| {n} | {re:g} | {ref['iterations']}{'' if ref['converged'] else ' (not converged)'} | {ref['wall']:.2f} | "
                   f"{far(rest):.1e} | " + " | ".join(f"{far(seeded[t]):.1e}" if t in seeded and seeded[t]["converged"] else "-"
                                                      for t in SEED_TOLERANCES) + " |")
            print("reference", row, flush=True)
            refs.append(row)
    if refs:
        lines += ["", f"Maximum-norm distance (u, v) from the seeded solve to tolerance {a.reference_tolerance:g}:", "",
                  "| N | Re | reference: iterations | s | from rest | " + " | ".join(f"seed to {t:g}" for t in SEED_TOLERANCES) + " |",
                  "|---|---|---|---|---|" + "---|" * len(SEED_TOLERANCES)] + refs
    lines += ["", "Did not run (budget): " + (", ".join(str(c) for c in skipped) if skipped else "nothing."), ""]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
