"""A/B of the chip-wide kernel's batch form (ldc_batch_mode 5) against what a sweep gets without it, one card, one process,
the forms measured one after another: trial-iterations per second, diagnostics off, chunks of 512 iterations.

  (a) launch path: two halves of the batch on two HIP streams (persistent=0), as bench.py's farm leg and main.py advance
      an equal-N group today;
  (b) batch mode 5: one batch, every trial persistent=5, launch groups of ldc_wide_trials_per_launch trials;
  (c) lone mode-5 trials one after another (one launch per trial and chunk).

Batches run the tiles layout only (the lone trials of (c) too); (b) is skipped where the size has no batch form (N=256).
Three timed windows per form, the median reported.
Usage: python tools/ab_wide_batch.py [N:B ...]   (default 96:14 128:8 160:4 256:2)"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "02689-advancednumericalalgorithmp3_amd", "src"))

import torch  # noqa: E402

from solvers.spectral import ldc_lib as L  # noqa: E402
from solvers.spectral.batched import BatchedSGSolver, run_concurrently  # noqa: E402
from solvers.spectral.sg import SGSolver  # noqa: E402

K = 512          # iterations per chunk
CHUNKS = 2       # chunks per timed window
WINDOWS = 3


def trials(N, B, persistent):
    kw = dict(name="spectral", lid_velocity=1.0, Lx=1.0, Ly=1.0, nx=N, ny=N, tolerance=0.0, max_iterations=10**9,
              basis_type="chebyshev", CFL=1.5, beta_squared=5.0, corner_treatment="smoothing", multigrid="none",
              check_every=4096, graph_iters=64, persistent=persistent)
    return [dict(kw, Re=1000.0, corner_smoothing=0.02 + 0.01 * q) for q in range(B)]


def windows(step, n_trials):
    rates = []
    for _ in range(WINDOWS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step()
        torch.cuda.synchronize()
        rates.append(n_trials * K * CHUNKS / (time.perf_counter() - t0))
    return statistics.median(rates), min(rates), max(rates)


def launch_path_halves(N, B):
    ts = trials(N, B, 0)
    halves = [BatchedSGSolver(ts[: B // 2]), BatchedSGSolver(ts[B // 2:])]
    run_concurrently(halves, lambda b: b.run_iterations(64, diagnostics=False))       # edge fix, graph build
    assert all(b.kernel_mode == 0 for b in halves)

    def advance(b):
        for _ in range(CHUNKS):
            b.run_iterations(K, diagnostics=False)
    out = windows(lambda: run_concurrently(halves, advance), B)
    for b in halves:
        b.close()
    return out


def batch_mode5(N, B):
    b = BatchedSGSolver(trials(N, B, 5))
    b.run_iterations(K + 1, diagnostics=False)        # edge fix + the chunk graph of length K
    assert b.kernel_mode == 5, b.kernel_mode

    def step():
        for _ in range(CHUNKS):
            b.run_iterations(K, diagnostics=False)
    out = windows(step, B)
    b.close()
    return out


def lone_mode5(N, B):
    ss = [SGSolver(**t) for t in trials(N, B, 5)]
    for s in ss:
        s.run_iterations(K + 1, diagnostics=False)
        assert s.kernel_mode == 5

    def step():
        for _ in range(CHUNKS):
            for s in ss:
                s.run_iterations(K, diagnostics=False)
    out = windows(step, B)
    for s in ss:
        s.close()
    return out


def main(argv):
    import ctypes as C
    cases = [tuple(int(x) for x in a.split(":")) for a in argv] or [(96, 14), (128, 8), (160, 4), (256, 2)]
    cus, xcds = C.c_int(), C.c_int()
    L.check(L.lib().ldc_device_info(C.byref(cus), C.byref(xcds)), "ldc_device_info")
    print(f"# device {torch.cuda.get_device_name(0)}, {cus.value} CUs; K={K} x {CHUNKS} per window, {WINDOWS} windows, "
          "rates in k trial-iterations/s (median [min, max])", flush=True)
    for N, B in cases:
        layouts = ["tiles"] if N < 256 else [None]
        rate_a = None
        for layout in layouts:
            if layout is None:
                os.environ.pop("LDC_WIDE_LAYOUT", None)
            else:
                os.environ["LDC_WIDE_LAYOUT"] = layout
            G = int(L.lib().ldc_wide_trials_per_launch(N, N, 0, cus.value))
            if rate_a is None:                  # (the launch path has no layout switch)
                rate_a = launch_path_halves(N, B)
            rb = batch_mode5(N, B) if G >= 1 else (0.0, 0.0, 0.0)
            rc = lone_mode5(N, B)
            rec = dict(N=N, B=B, layout=layout or "default", trials_per_launch=G,
                       launch_path_halves=round(rate_a[0] / 1e3, 1), batch_mode5=round(rb[0] / 1e3, 1),
                       lone_mode5=round(rc[0] / 1e3, 1), spread=dict(a=[round(x / 1e3, 1) for x in rate_a[1:]],
                                                                     b=[round(x / 1e3, 1) for x in rb[1:]],
                                                                     c=[round(x / 1e3, 1) for x in rc[1:]]))
            print(f"N={N:3d} B={B:2d} layout={rec['layout']:7s} G={G}:  (a) launch path, halves {rec['launch_path_halves']:7.1f}"
                  f"   (b) batch mode 5 {rec['batch_mode5']:7.1f}   (c) lone mode 5 {rec['lone_mode5']:7.1f}"
                  f"   b/a {rb[0] / rate_a[0]:.2f}   c/a {rc[0] / rate_a[0]:.2f}", flush=True)
            print(json.dumps(rec), flush=True)
    os.environ.pop("LDC_WIDE_LAYOUT", None)


if __name__ == "__main__":
    main(sys.argv[1:])
