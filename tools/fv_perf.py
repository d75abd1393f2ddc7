#!/usr/bin/env python3
"""Finite-volume kernel timings (include/ldc_fv.h): microseconds per SIMPLE iteration of a lone trial at N = 64, 128,
256 (TVD, the YAML's settings, from a developed state), trial-iterations/s of B trials in one launch, and the mean
BiCGSTAB iterations per momentum solve.  Prints one JSON line per measurement.

    python tools/fv_perf.py [--iters 200] [--batch 256] [--batch-n 64]

``--sweep`` times a whole finite-volume sweep through the launcher instead: the grid N = 64, 128 x Re = 100, 400, 1000
(TVD, tolerance 1e-6, max_iterations 20000 so that no trial can run away) in a fresh child process, and prints one line
with the wall time of the process, the launcher's own time inside the solves and every trial's iterations and time.
``--main`` points at the main.py of another checkout (a worktree of the parent commit, built there) for an A/B on one
card; ``--max-batch 1`` runs this checkout's trials one by one.

``--post`` times the post-processing of a finished batch (streamfunction and vortex metrics, copies included): 256 trials
at N = 64 and 64 at N = 128, each after ``--iters`` iterations from rest, on the host path (SciPy's sparse solve, one
trial after another) and on the device path (ldc_fv_post_enqueue), in one process, alternated twice.

    python tools/fv_perf.py --post [--iters 200] [--post-cases 256x64,64x128]

    python tools/fv_perf.py --sweep [--label head] [--main /path/to/other/checkout/02689-.../main.py] [--max-batch 1]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "02689-advancednumericalalgorithmp3_amd" / "src")]


SWEEP = ["-m", "solver=fv", "N=64,128", "Re=100,400,1000", "tolerance=1e-6", "max_iterations=20000"]


def sweep(a):
    main_py = Path(a.main).resolve() if a.main else ROOT / "02689-advancednumericalalgorithmp3_amd" / "main.py"
    env = {k: v for k, v in os.environ.items() if k != "LDC_MAX_BATCH"}
    if a.max_batch is not None:
        env["LDC_MAX_BATCH"] = str(a.max_batch)
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        r = subprocess.run([sys.executable, str(main_py)] + SWEEP, cwd=tmp, env=env, capture_output=True, text=True,
                           timeout=a.timeout)
        wall = time.perf_counter() - t0
        if r.returncode != 0:
            sys.exit(f"the sweep failed ({r.returncode}):\n{r.stderr[-3000:]}")
        recs = json.loads(next(Path(tmp).rglob("sweep_results.json")).read_text())
    trials = [dict(N=x["N"], Re=x["Re"], iterations=x["metrics"]["iterations"], converged=x["metrics"]["converged"],
                   seconds=round(x["metrics"]["wall_time_seconds"], 3), batch_size=x.get("solve_batch_size", 1),
                   record_seconds=round(x["total_seconds"], 3)) for x in recs]
    print(json.dumps(dict(what="sweep", label=a.label, max_batch=a.max_batch, trials=len(trials),
                          wall_seconds=round(wall, 2),
                          # inside the solves: the batch's own wall time, or the sum of the lone solves
                          solve_seconds=round(max((x.get("solve_batch_seconds", 0.0) for x in recs), default=0.0)
                                              or sum(t["seconds"] for t in trials), 2),
                          slowest_trial_seconds=max(t["seconds"] for t in trials) if all(t["batch_size"] == 1 for t in trials) else None,
                          per_trial=trials)), flush=True)


def post(a):
    import numpy as np
    import torch
    import __graft_entry__ as g
    g.build()
    from solvers.fv.batched import BatchedFVSolver
    from solvers.fv.solver import postprocess
    kw = dict(name="fv", convection_scheme="TVD", alpha_uv=0.4, alpha_p=0.2, linear_solver_tol=1e-9, tolerance=1e-30,
              check_every=a.iters, max_iterations=a.iters)
    for case in a.post_cases.split(","):
        b, n = (int(x) for x in case.split("x"))
        batch = BatchedFVSolver([dict(kw, nx=n, ny=n, Re=100.0 + 900.0 * q / max(1, b - 1)) for q in range(b)])
        for s in batch.solvers:
            s._begin(1e-30)
        batch._step(list(range(b)), a.iters)
        for s in batch.solvers:
            s._finalize_fields()

        def run(mode):
            for s in batch.solvers:
                s.params.vortex_metrics = mode
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if mode == "device":
                postprocess(batch.solvers)
            out = [s.compute_vortex_metrics() for s in batch.solvers]
            return time.perf_counter() - t0, out
        run("device")                                         # (first launch, sine tables, output tensors)
        times = {"host": [], "device": []}
        for _ in range(2):
            for mode in ("host", "device"):
                dt, out = run(mode)
                times[mode].append(dt)
                times[mode + "_psi_min"] = float(np.mean([m["psi_min"] for m in out]))
        host, dev = min(times["host"]), min(times["device"])
        print(json.dumps(dict(what="post", N=n, trials=b, iterations=a.iters,
                              host_seconds=[round(t, 4) for t in times["host"]],
                              device_seconds=[round(t, 5) for t in times["device"]],
                              host_ms_per_trial=round(host / b * 1e3, 3), device_ms_per_trial=round(dev / b * 1e3, 4),
                              host_over_device=round(host / dev, 1),
                              mean_psi_min=dict(host=times["host_psi_min"], device=times["device_psi_min"]))), flush=True)
        batch.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--post", action="store_true", help="time host and device post-processing of finished batches")
    ap.add_argument("--post-cases", default="256x64,64x128", help="trials x N, comma-separated")
    ap.add_argument("--sweep", action="store_true", help="time the N = 64, 128 x Re = 100, 400, 1000 sweep through main.py")
    ap.add_argument("--label", default="head")
    ap.add_argument("--main", default=None, help="main.py of another (built) checkout")
    ap.add_argument("--max-batch", type=int, default=None, help="LDC_MAX_BATCH of the child process")
    ap.add_argument("--timeout", type=float, default=900.0)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warm", type=int, default=300)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--batch-n", type=int, default=64)
    ap.add_argument("--sizes", default="64,128,256")
    a = ap.parse_args()
    if a.sweep:
        return sweep(a)
    if a.post:
        return post(a)
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
