#!/usr/bin/env python3
"""What does the separable scaled preconditioner buy a chip trial on a wall-clustered grid (grid="tanh", mapping="chip",
chip_grid="tables", pressure_equation="consistent", chip_preconditioner laplacian | separable)?  TVD at Re = 1000 (the YAML's
settings), beta = 1.5, graph replay:

  rate      per size, ``--rounds`` rounds in ONE process that alternate the two preconditioners from the SAME developed state:
            a separable trial is advanced ``--warmup`` iterations from rest, its u, v, p, mdot are copied into both trials,
            both run one untimed chunk (the budgets settle), then the timed chunks alternate; microseconds per SIMPLE iteration
            (best, median and worst round), launches per iteration, the budgets a converging run settled on, and the mean
            BiCGSTAB and CG iterations per solve while timed.
  converge  one trial (``--converge N``) with streamfunction="wall_stretched", vortex_refine="quadratic", 0.7 / 0.3 to
            ``--tolerance``: wall time, iterations, the centreline extrema against Botella and Peyret, the ``botella_vortex``
            objective.

    python tools/fv_wide_separable_perf.py [--sizes 64,128,256,512,1024] [--converge 256] [--converge-with separable]
                                           [--out profiles/fv_wide_separable.md]

Every step is a fresh child process under a time limit of its own; after a step that fails or passes its limit nothing more
is started, the tables are written with what there is and the tool exits non-zero.  Writes Markdown to ``--out`` and one JSON
line per step beside it.
"""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path
from types import SimpleNamespace

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "02689-advancednumericalalgorithmp3_amd" / "src"), str(ROOT / "tests")]

YAML = dict(convection_scheme="TVD", linear_solver_tol=1e-9)
BETA = 1.5
CHIP = dict(grid="tanh", grid_stretch=BETA, mapping="chip", chip_grid="tables", pressure_equation="consistent")
KINDS = ("laplacian", "separable")


def rate(a):
    """The child: one size, the two preconditioners alternated round by round from one developed state."""
    import torch
    import __graft_entry__ as g
    g.build()
    from solvers.fv import ldc_fv_lib as F
    from solvers.fv.solver import FVSolver
    n, chunk = int(a.rate), int(a.chunk)
    kw = dict(YAML, name="fv", nx=n, ny=n, Re=1000.0, alpha_uv=0.4, alpha_p=0.2, tolerance=1e-30, max_iterations=10**9,
              check_every=chunk, **CHIP)
    forms = {k: FVSolver(**kw, chip_preconditioner=k) for k in KINDS}
    for s in forms.values():
        s.set_wide_graph(True)
    lead = forms["separable"]                     # the developed state, by the cheaper of the two
    lead._begin(1e-30)
    left = int(a.warmup)
    while left > 0:
        lead._advance(min(chunk, left))
        left -= min(chunk, left)
    st = lead.state()
    for s in forms.values():
        s.set_state(st["u"], st["v"], st["p"], st["mdot"])
        s._begin(1e-30)
        s._advance(chunk)                         # untimed: graphs are captured and the budgets settle
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    before = {k: s.counters() for k, s in forms.items()}
    for _ in range(int(a.rounds)):
        for k, s in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s._advance(chunk)
            times[k].append(1e6 * (time.perf_counter() - t0) / chunk)
    out = dict(step="rate", N=n, beta=BETA, warmup=int(a.warmup), chunk=chunk, rounds=int(a.rounds), forms={})
    for k, s in forms.items():
        c, b = s.counters(), before[k]
        d = lambda key: c.get(key, 0) - b.get(key, 0)        # noqa: E731
        out["forms"][k] = dict(
            us_best=round(min(times[k]), 1), us_median=round(statistics.median(times[k]), 1), us_worst=round(max(times[k]), 1),
            launches_per_iteration=F.lib().ldc_fv_wide_launches(s._wide, s.linear_budget),
            linear_budget=s.linear_budget, pressure_budget=s.pressure_budget,
            retries_while_timed=d("linear_budget_retries") + d("pressure_budget_retries"),
            mean_bicgstab=round(d("linear_iterations") / max(1, d("momentum_solves")), 2),
            mean_cg=round(d("pressure_iterations") / max(1, d("pressure_solves")), 2),
            pressure_caps=d("pressure_caps"), iterations=c["iterations"], nan=c["nan"])
        s.close()
    print(json.dumps(out), flush=True)


def converge(a):
    """The child: one trial to the latch, its centreline extrema and vortex objective."""
    import __graft_entry__ as g
    g.build()
    from fv_stretched_numpy import BOTELLA_RE1000, centreline_extrema
    from solvers import validation as V
    from solvers.datastructures import _VORTEX_KEYS
    from solvers.fv.solver import FVSolver
    n = int(a.converge)
    s = FVSolver(**dict(YAML, name="fv", nx=n, ny=n, Re=1000.0, alpha_uv=0.7, alpha_p=0.3, pressure_tol=float(a.pressure_tol),
                        pressure_max_iters=400, tolerance=float(a.tolerance), max_iterations=int(a.max_iterations),
                        check_every=256, streamfunction="wall_stretched", vortex_refine="quadratic",
                        chip_preconditioner=a.converge_with, **CHIP))
    s.set_wide_graph(True)
    t0 = time.perf_counter()
    s.solve()
    wall = time.perf_counter() - t0
    c = s.counters()
    ny, nx = s.shape_full
    xs, ys = s.fields.x.reshape(ny, nx)[0], s.fields.y.reshape(ny, nx)[:, 0]
    ext = centreline_extrema(s.fields.u.reshape(ny, nx), s.fields.v.reshape(ny, nx), xs, ys)
    err = {k: abs(abs(ext[k]) - abs(BOTELLA_RE1000[k])) for k in ext}
    vortex = s.compute_vortex_metrics()
    m = SimpleNamespace(**{k: float(vortex.get(k, 0.0)) for k in _VORTEX_KEYS})
    out = dict(step="converge", N=n, beta=BETA, preconditioner=a.converge_with, tolerance=float(a.tolerance),
               pressure_tol=float(a.pressure_tol), wall_seconds=round(wall, 2), iterations=int(s.metrics.iterations),
               converged=bool(s.metrics.converged), ms_per_iteration=round(1e3 * wall / max(1, int(s.metrics.iterations)), 3),
               mean_cg=round(c["pressure_iterations"] / max(1, c["pressure_solves"]), 2), pressure_caps=c["pressure_caps"],
               pressure_budget=s.pressure_budget, linear_budget=s.linear_budget,
               retries=c["linear_budget_retries"] + c["pressure_budget_retries"], linear_giveups=c["linear_giveups"],
               extrema=ext, centreline_errors=err, objective=V.compute_botella_vortex_objective(m, 1000),
               refine_status=[int(x) for x in s.vortex_refine_status] if s.vortex_refine_status is not None else None,
               psi_min=m.psi_min, psi_min_x=m.psi_min_x, psi_min_y=m.psi_min_y, omega_center=m.omega_center)
    s.close()
    print(json.dumps(out), flush=True)


def limit(n):
    """Seconds allowed to a rate step: a minute to start and build the eigenvectors, then its iterations at the laplacian
    chain's 44 ms x (n / 1024)^2 with a floor of 0.5 ms and a factor of 3 (profiles/fv_wide_stretched.md)."""
    return 60.0 + n / 4.0 + 3.0 * 1500 * max(0.0005, 0.044 * (n / 1024.0) ** 2)


def tables(results):
    rows = ["| N | preconditioner | us / iteration (best) | (median) | (worst round) | launches / iteration | budgets (linear, "
            "pressure) | retries while timed | mean BiCGSTAB | mean CG | laplacian / this |",
            "|---|---|---|---|---|---|---|---|---|---|---|"]
    text = []
    for r in results:
        if "error" in r:
            rows.append(f"| {r['N']} | {r['error']} | - | - | - | - | - | - | - | - | - |")
            continue
        if r["step"] == "converge":
            text += ["", f"Converged {r['N']} x {r['N']}, Re = 1000, beta = {r['beta']}, `chip_preconditioner={r['preconditioner']}`, "
                     f"0.7 / 0.3, tolerance {r['tolerance']:g}, pressure_tol {r['pressure_tol']:g}, `wall_stretched` + `quadratic`:",
                     "", "```json", json.dumps(r, indent=1), "```"]
            continue
        lap = r["forms"]["laplacian"]["us_best"]
        for k, f in r["forms"].items():
            rows.append("| {} | {} | {} | {} | {} | {} | {}, {} | {} | {} | {} | {:.2f} |".format(
                r["N"], k, f["us_best"], f["us_median"], f["us_worst"], f["launches_per_iteration"], f["linear_budget"],
                f["pressure_budget"], f["retries_while_timed"], f["mean_bicgstab"], f["mean_cg"], lap / f["us_best"]))
    return ("Rate (TVD, Re = 1000, 0.4 / 0.2, beta = 1.5, consistent, graph replay, from the developed state of the warm-up; the "
            "two preconditioners alternate in one process):\n\n" + "\n".join(rows) + "\n" + "\n".join(text) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,128,256,512,1024")
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--chunk", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--converge", type=int, default=0)
    ap.add_argument("--converge-with", default="separable", choices=KINDS)
    ap.add_argument("--tolerance", type=float, default=1e-6)
    ap.add_argument("--pressure-tol", type=float, default=1e-8)
    ap.add_argument("--max-iterations", type=int, default=40000)
    ap.add_argument("--converge-limit", type=float, default=540.0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "fv_wide_separable.md"))
    ap.add_argument("--rate", type=int, help=argparse.SUPPRESS)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.rate:
        return rate(a)
    if a.child:
        return converge(a)
    import __graft_entry__ as g
    g.build()                                     # once, here: the children find the library up to date
    out, results, failed = Path(a.out), [], None
    out.parent.mkdir(parents=True, exist_ok=True)
    log = out.with_suffix(".jsonl")
    log.write_text("")
    me = [sys.executable, str(Path(__file__).resolve()), "--warmup", str(a.warmup), "--chunk", str(a.chunk),
          "--rounds", str(a.rounds)]
    steps = [(int(x), me + ["--rate", x], limit(int(x))) for x in a.sizes.split(",") if x]
    if a.converge:
        steps.append((a.converge, me + ["--child", "--converge", str(a.converge), "--converge-with", a.converge_with,
                                        "--tolerance", str(a.tolerance), "--pressure-tol", str(a.pressure_tol),
                                        "--max-iterations", str(a.max_iterations)], a.converge_limit))
    for n, cmd, seconds in steps:
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=seconds)
            lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
            if r.returncode != 0 or not lines:
                failed = f"N = {n}: exit {r.returncode}\n{r.stderr[-3000:]}"
        except subprocess.TimeoutExpired:
            failed, lines = f"N = {n}: no result within {seconds:.0f} s", []
        results.append(json.loads(lines[-1]) if lines and not failed else dict(step="rate", N=n, error="failed"))
        print(json.dumps(results[-1]), flush=True)
        with log.open("a") as f:
            f.write(json.dumps(results[-1]) + "\n")
        out.write_text(tables(results))
        if failed:                                # nothing more is started on the card after a step that failed
            break
    print(tables(results))
    if failed:
        sys.exit(f"stopped after a failed step; the tables hold what there was.  {failed}")


if __name__ == "__main__":
    main()
