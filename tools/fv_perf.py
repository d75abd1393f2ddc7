#!/usr/bin/env python3
"""Finite-volume kernel timings (include/ldc_fv.h): microseconds per SIMPLE iteration of a lone trial at N = 64, 128,
256 (TVD, the YAML's settings, from a developed state), trial-iterations/s of B trials in one launch, and the mean
BiCGSTAB iterations per momentum solve.  Prints one JSON line per measurement.

    python tools/fv_perf.py [--iters 200] [--batch 256] [--batch-n 64]
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
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warm", type=int, default=300)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--batch-n", type=int, default=64)
    ap.add_argument("--sizes", default="64,128,256")
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    from solvers.fv import ldc_fv_lib as F
    from solvers.fv.solver import FVSolver
    kw = dict(name="fv", Re=1000.0, convection_scheme="TVD", alpha_uv=0.4, alpha_p=0.2, linear_solver_tol=1e-9,
              tolerance=1e-30, check_every=max(a.iters, a.warm))
    stream = torch.cuda.current_stream().cuda_stream
    for n in [int(x) for x in a.sizes.split(",")]:
        s = FVSolver(nx=n, ny=n, **kw)
        s._begin(1e-30)
        s._advance(a.warm)
        c0 = s.counters()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        F.check(F.lib().ldc_fv_enqueue(s.handle, a.iters, stream))
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        c1 = s.counters()
        print(json.dumps(dict(what="lone", N=n, iterations=a.iters, us_per_iteration=round(dt / a.iters * 1e6, 1),
                              mean_bicgstab_iterations=round((c1["linear_iterations"] - c0["linear_iterations"])
                                                             / (c1["momentum_solves"] - c0["momentum_solves"]), 2))),
              flush=True)
        s.close()
    trials = [FVSolver(nx=a.batch_n, ny=a.batch_n, **dict(kw, Re=100.0 + 900.0 * q / max(1, a.batch - 1)))
              for q in range(a.batch)]
    for s in trials:
        s._begin(1e-30)
    hs = [s.handle for s in trials]
    F.batch_enqueue(hs, a.warm, stream)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    F.batch_enqueue(hs, a.iters, stream)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps(dict(what="batch", N=a.batch_n, trials=a.batch, iterations=a.iters,
                          trial_iterations_per_s=round(a.batch * a.iters / dt, 1),
                          us_per_launch_iteration=round(dt / a.iters * 1e6, 1))), flush=True)
    for s in trials:
        s.close()


if __name__ == "__main__":
    main()
