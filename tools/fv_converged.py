#!/usr/bin/env python3
"""Converged finite-volume fields at N = 128 (TVD, the YAML's settings, tolerance 1e-6) against the reference's stored
solutions: lid "none" vs data/validation/fv/Re*, lid "saad" vs data/validation/fv-regu/Re*.  One JSON line per case.

    python tools/fv_converged.py [--cases 100:none,1000:none,400:saad,1000:saad]
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "02689-advancednumericalalgorithmp3_amd" / "src")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="100:none,1000:none,400:saad,1000:saad")
    ap.add_argument("--N", type=int, default=128)
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from solvers.fv.solver import FVSolver
    for case in a.cases.split(","):
        re_, lid = case.split(":")
        s = FVSolver(name="fv", Re=float(re_), nx=a.N, ny=a.N, convection_scheme="TVD", alpha_uv=0.4, alpha_p=0.2,
                     linear_solver_tol=1e-9, tolerance=1e-6, max_iterations=60000, corner_treatment=lid)
        t0 = time.perf_counter()
        s.solve()
        wall = time.perf_counter() - t0
        c = s.counters()
        print(json.dumps(dict(N=a.N, Re=int(float(re_)), lid=lid, converged=s.metrics.converged,
                              iterations=s.metrics.iterations, wall_s=round(wall, 2),
                              us_per_iteration=round(wall / s.metrics.iterations * 1e6, 1),
                              mean_bicgstab_iterations=round(c["linear_iterations"] / c["momentum_solves"], 2),
                              linear_giveups=c["linear_giveups"], validation_errors=s.compute_validation_errors(),
                              psi_min=s.metrics.psi_min, ghia=s.ghia_error() if int(float(re_)) in (100, 400, 1000) else None)),
              flush=True)
        s.close()


if __name__ == "__main__":
    main()
