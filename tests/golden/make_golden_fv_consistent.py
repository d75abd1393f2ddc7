"""Writes tests/golden/g16_fv_consistent.npz: the converged fields and the iteration counts of the NumPy restatement of the
SIMPLE iteration with the consistent pressure equation (tests/fv_consistent_numpy.py; TVD, tolerance 1e-6,
linear_solver_tol 1e-9, pressure_tol 1e-8), which tests/test_gpu_fv_pressure.py compares the device's solves with.
Minutes of NumPy at 32 x 32, so it is recorded once:  python tests/golden/make_golden_fv_consistent.py"""
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
from fv_consistent_numpy import FVConsistentState  # noqa: E402

CASES = {"N16_Re100_04_02": dict(nx=16, ny=16, Re=100.0, alpha_uv=0.4, alpha_p=0.2),
         "N32_Re1000_07_03": dict(nx=32, ny=32, Re=1000.0, alpha_uv=0.7, alpha_p=0.3)}

if __name__ == "__main__":
    out = {}
    for tag, c in CASES.items():
        o = FVConsistentState(c["nx"], c["ny"], c["Re"], alpha_uv=c["alpha_uv"], alpha_p=c["alpha_p"],
                              linear_solver_tol=1e-9, convection_scheme="TVD")
        rec = o.run(20000, tol=1e-6)
        print(tag, len(rec), "iterations, CG at most", max(o.cg_iters))
        out.update({f"{tag}_iterations": np.int64(len(rec)), f"{tag}_u": o.u.ravel(), f"{tag}_v": o.v.ravel(),
                    f"{tag}_p": o.p.ravel()})
    np.savez_compressed(HERE / "g16_fv_consistent.npz", **out)
