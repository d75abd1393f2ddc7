#!/usr/bin/env python3
"""FV-Q1: which value of the TVD limiter psi did the reference's compiled code use on faces with
mdot >= 0?  Each candidate is run to convergence with the NumPy restatement (tests/fv_numpy.py) at N = 128,
tolerance 1e-6, the YAML's TVD settings, and its u, v are compared with the stored converged FV solutions that
the reference produced (data/validation/fv/Re*/solution.npz).  Prints one JSON line per (Re, candidate).

    python tools/fv_q1_table.py [--N 128] [--re 100,1000] [--cand zero,muscl,one]
"""
import argparse
import json
import sys
import time
from concurrent.futures import ProcessPoolExecutor
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
DATA = ROOT / "02689-advancednumericalalgorithmp3_amd" / "data" / "validation" / "fv"


def run(args):
    N, Re, cand, max_it = args
    from fv_numpy import FVState
    s = FVState(N, N, Re, alpha_uv=0.4, alpha_p=0.2, linear_solver_tol=1e-9, convection_scheme="TVD", psi_up=cand)
    t0 = time.perf_counter()
    rec = s.run(max_it, tol=1e-6)
    wall = time.perf_counter() - t0
    g = np.load(DATA / f"Re{Re}" / "solution.npz")
    order = np.lexsort((g["y"], g["x"]))                  # stored points: x slow, y fast
    x = (np.arange(N) + 0.5) / N
    ok = np.allclose(g["x"][order].reshape(N, N)[:, 0], x) and np.allclose(g["y"][order].reshape(N, N)[0, :], x)
    ru, rv = g["u"][order].reshape(N, N).T, g["v"][order].reshape(N, N).T      # -> [j, i]
    eu = float(np.linalg.norm(s.u - ru) / np.linalg.norm(ru))
    ev = float(np.linalg.norm(s.v - rv) / np.linalg.norm(rv))
    return dict(N=N, Re=Re, psi_for_mdot_ge_0=cand, iterations=len(rec), converged=bool(rec[-1, 0] < 1e-6),
                u_rel_L2=eu, v_rel_L2=ev, grid_ok=bool(ok), mean_bicgstab_iterations=float(np.mean(s.iters)),
                host_seconds=round(wall, 1), host_iterations_per_s=round(len(rec) / wall, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=128)
    ap.add_argument("--re", default="100,1000")
    ap.add_argument("--cand", default="zero,muscl,one")
    ap.add_argument("--max-it", type=int, default=40000)
    a = ap.parse_args()
    jobs = [(a.N, int(re), c, a.max_it) for re in a.re.split(",") for c in a.cand.split(",")]
    with ProcessPoolExecutor(max_workers=len(jobs)) as ex:
        for r in ex.map(run, jobs):
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
