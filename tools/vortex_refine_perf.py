#!/usr/bin/env python3
"""What does ``vortex_refine="newton"`` cost, and what does it change in the Botella comparison?  ONE process:

  time     per size, on ONE seeded developed state: seconds per ``compute_vortex_metrics()`` with ``"none"`` and with
           ``"newton"``, alternated, ``--rounds`` runs each, wait included; both run once before the clock starts (the
           eigenbasis and the barycentric weights are uploaded at the first call).  The spread of the ``none`` runs is the
           margin below which a difference says nothing;
  botella  one FSG trial per N (Re = 1000, corner_smoothing 0.15, to the tolerance of
           conf/experiment/optimization/corner_smoothing.yaml): the ``botella_vortex`` objective and the rows of the Botella
           table from the SAME converged state with both settings, and the statuses of the refinement.

    python tools/vortex_refine_perf.py [--sizes 32,50,128,256] [--botella 30,40,50] [--out profiles/spectral_refine.md]

Appends Markdown to ``--out``.  Run it under a time limit: a step that raises ends the tool, nothing is started after it.
"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "02689-advancednumericalalgorithmp3_amd" / "src")]

YAML = dict(basis_type="chebyshev", CFL=1.5, beta_squared=5.0, corner_treatment="smoothing", corner_smoothing=0.15)


def seed(s):
    """A developed flow: a primary vortex off the centre and an eddy in each of three corners, u = psi_y, v = -psi_x."""
    X, Y = s.x_full, s.y_full

    def eddy(x0, x1, y0, y1):
        inside = (X > x0) & (X < x1) & (Y > y0) & (Y < y1)
        return np.where(inside, (np.sin(np.pi * (X - x0) / (x1 - x0)) * np.sin(np.pi * (Y - y0) / (y1 - y0))) ** 2, 0.0)
    psi = -0.1 * (np.sin(np.pi * X ** 1.3) * np.sin(np.pi * Y ** 1.6)) ** 2
    psi += 0.005 * (eddy(0.7, 1.0, 0.0, 0.3) + eddy(0.0, 0.25, 0.0, 0.25)) + 0.02 * eddy(0.0, 0.3, 0.6, 0.9)
    u, v = psi @ s.Dy_1d.T, -(s.Dx_1d @ psi)
    u[0, :] = u[-1, :] = v[0, :] = v[-1, :] = 0.0
    u[:, 0] = v[:, 0] = v[:, -1] = 0.0
    u[:, -1] = s.u_lid
    s.set_state(u=u, v=v, p=np.zeros(s.shape_inner))


def timing(SGSolver, n, rounds):
    import torch
    s = SGSolver(**YAML, name="spectral", Re=1000.0, nx=n, ny=n)
    seed(s)

    def call(mode):
        s.params.vortex_refine = mode
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = s.compute_vortex_metrics()
        return time.perf_counter() - t0, out
    for mode in ("none", "newton"):
        call(mode)
    times = {"none": [], "newton": []}
    for _ in range(rounds):
        for mode in times:
            times[mode].append(call(mode)[0])
    status = s.vortex_refine_status
    s.close()
    return times, status


def botella(FSGSolver, n, tolerance, cap):
    from solvers import validation as V
    from solvers.base import _VORTEX_KEYS
    from solvers.datastructures import Metrics
    s = FSGSolver(**YAML, name="spectral_fsg", Re=1000.0, nx=n, ny=n, multigrid="fsg", n_levels=2, coarse_tolerance_factor=1.0,
                  tolerance=tolerance, max_iterations=cap)          # (conf/solver/spectral/fsg.yaml)
    s.solve()
    out = {}
    for mode in ("none", "newton"):
        s.params.vortex_refine = mode
        vm = s.compute_vortex_metrics()
        m = Metrics(**{k: float(vm.get(k, 0.0)) for k in _VORTEX_KEYS})
        out[mode] = (V.compute_botella_vortex_objective(m, 1000), V.botella_table(m, 1000))
    info = (int(s.metrics.iterations), bool(s.metrics.converged), s.vortex_refine_status)
    s.close()
    return out, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="32,50,128,256")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--botella", default="30,40,50")
    ap.add_argument("--tolerance", type=float, default=1e-6)
    ap.add_argument("--max-iterations", type=int, default=500000)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "spectral_refine.md"))
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from solvers.spectral.fsg import FSGSolver
    from solvers.spectral.sg import SGSolver
    fmt = lambda ts: " / ".join(f"{t:.4g}" for t in ts)        # noqa: E731
    text = ["", "### Cost of `vortex_refine=\"newton\"` (tools/vortex_refine_perf.py)", "",
            f"Seconds per `compute_vortex_metrics()` on one seeded state, {a.rounds} runs per setting, alternated in one process:", "",
            "| N | none | newton | spread of none | newton (mean) - none (mean) | statuses |", "|---|---|---|---|---|---|"]
    for n in [int(x) for x in a.sizes.split(",") if x]:
        t, status = timing(SGSolver, n, a.rounds)
        text.append("| {} | {} | {} | {:.4g} | {:.4g} | {} |".format(
            n, fmt(t["none"]), fmt(t["newton"]), max(t["none"]) - min(t["none"]),
            float(np.mean(t["newton"]) - np.mean(t["none"])), list(status)))
        print(text[-1], flush=True)
    sizes = [int(x) for x in a.botella.split(",") if x]
    if sizes:
        text += ["", f"Botella comparison at Re = 1000 (FSG, corner_smoothing 0.15, tolerance {a.tolerance:g}), both settings on the same "
                 "converged state:", "", "| N | iterations | converged | objective none | objective newton | statuses |", "|---|---|---|---|---|---|"]
        tables = []
        for n in sizes:
            out, (its, conv, status) = botella(FSGSolver, n, a.tolerance, a.max_iterations)
            text.append(f"| {n} | {its} | {conv} | {out['none'][0]:.4e} | {out['newton'][0]:.4e} | {list(status)} |")
            print(text[-1], flush=True)
            tables.append((n, out))
        for n, out in tables:
            text += ["", f"N = {n}:", "", "| vortex | metric | Botella | none | error % | newton | error % |", "|---|---|---|---|---|---|---|"]
            for r0, r1 in zip(out["none"][1], out["newton"][1]):
                text.append(f"| {r0['Vortex']} | {r0['Metric']} | {r0['Botella']} | {r0['Computed']} | {r0['Error (%)']} | "
                            f"{r1['Computed']} | {r1['Error (%)']} |")
    with Path(a.out).open("a") as f:
        f.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
