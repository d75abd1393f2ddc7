#!/usr/bin/env python3
"""The converged stretched-grid case the GPU suite pins (tests/test_gpu_fv_stretched.py): the NumPy restatement
(tests/fv_stretched_numpy.py) to its latch at 32 x 32, Re 1000, beta 1.5, TVD, the consistent pressure equation, relaxation
0.7 / 0.3, linear_solver_tol 1e-9.  Written to tests/golden/g17_fv_stretched_converged.json: the iteration count, rel at the
stop and one iteration before with their relative distances to the tolerance (the count is a fair demand on the kernel only
if rounding cannot move it: both must be >= 1e-4, as for g15_fv_converged; otherwise choose another tolerance), the centreline
extrema and the CG statistics.

Usage:  python tools/fv_stretched_converged.py [--tolerance 1e-7] [--n 32] [--beta 1.5]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

from fv_stretched_numpy import BOTELLA_RE1000, FVStretchedState, centreline_extrema  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tolerance", type=float, default=1e-7)
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--beta", type=float, default=1.5)
    ap.add_argument("--max-iterations", type=int, default=20000)
    ap.add_argument("--out", default=str(ROOT / "tests" / "golden" / "g17_fv_stretched_converged.json"))
    a = ap.parse_args()
    params = dict(alpha_uv=0.7, alpha_p=0.3, linear_solver_tol=1e-9, convection_scheme="TVD", grid_stretch=a.beta,
                  pressure_equation="consistent", pressure_tol=1e-8, pressure_max_iters=200)
    s = FVStretchedState(a.n, a.n, 1000.0, **params)
    t0 = time.time()
    rec = s.run(a.max_iterations, tol=a.tolerance)
    rel = rec[:, 0]
    assert rel[-1] < a.tolerance <= rel[-2], "not converged"
    margins = dict(at_stop=(a.tolerance - rel[-1]) / a.tolerance, before_stop=(rel[-2] - a.tolerance) / a.tolerance)
    ext = centreline_extrema(s.u, s.v, s.xc, s.yc)
    out = dict(nx=a.n, ny=a.n, Re=1000.0, tolerance=a.tolerance, **params, iterations=len(rel), rel_at_stop=float(rel[-1]),
               rel_before_stop=float(rel[-2]), margins=margins, extrema=ext,
               errors={k: abs(abs(ext[k]) - abs(BOTELLA_RE1000[k])) for k in ext},
               cg_iterations_mean=float(np.mean(s.cg_iters)), cg_iterations_max=int(max(s.cg_iters)), cg_caps=int(s.cg_caps),
               record_last=[float(x) for x in rec[-1]])
    print(json.dumps(out, indent=1), f"\n{time.time() - t0:.1f} s")
    assert min(margins.values()) >= 1e-4, "rounding could move the count: choose another tolerance"
    Path(a.out).write_text(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
