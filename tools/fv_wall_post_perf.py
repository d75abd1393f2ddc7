#!/usr/bin/env python3
"""What do ``streamfunction="wall"`` and ``vortex_refine="quadratic"`` change in the Botella comparison, and what does
the chain of ``ldc_fv_wall_post_enqueue`` cost?  ONE process:

  botella  ONE batch of converged trials (``--sizes`` x ``--res``, conf/solver/fv.yaml's scheme and relaxation), then on
           every final state the vortex metrics by three rules: ``device`` (the reference's ring rule), ``wall`` and
           ``wall`` + ``quadratic``; per rule the rows of ``validation_table`` and ``compute_botella_vortex_objective``;
  chain    seconds per ``ldc_fv_wall_post_enqueue`` call with its wait (enqueue, then a stream synchronise), for one job at
           each of ``--chain-sizes`` and for ``--jobs`` jobs of ``--jobs-size`` cells per axis, on seeded states: every
           case runs once before the clock starts, then ``--rounds`` rounds of ``--calls`` calls, the cases alternating
           round by round;
  hashes   with ``--parent-tree DIR`` (a checkout of the parent commit; needs hipcc, no GPU) the device code of the eight
           units from before is compiled from both trees at one path, disassembled and hashed, by the method of
           profiles/fv_cu_pressure.md.  ``--skip botella,chain`` makes that the whole run.

    python tools/fv_wall_post_perf.py [--out profiles/fv_wall_post.md] [--jsonl profiles/fv_wall_post.jsonl]

Appends Markdown to ``--out`` and one JSON line per row to ``--jsonl``.  Run it under a time limit: a step that raises ends
the tool, nothing is started after it."""
import argparse
import json
import sys
import time
from pathlib import Path
from types import SimpleNamespace

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "02689-advancednumericalalgorithmp3_amd" / "src")]

YAML = dict(name="fv", convection_scheme="TVD", alpha_uv=0.4, alpha_p=0.2, linear_solver_tol=1e-9)
RULES = (("device", dict(streamfunction="reference", vortex_refine="none")),
         ("wall", dict(streamfunction="wall", vortex_refine="none")),
         ("wall + quadratic", dict(streamfunction="wall", vortex_refine="quadratic")))


def metrics_by(s, rule):
    """The vortex metrics of the solver's final state by one of RULES, as an object with the keys of ``Metrics``."""
    from solvers.datastructures import _VORTEX_KEYS
    s.params.vortex_metrics = "device"
    s.params.streamfunction, s.params.vortex_refine = rule["streamfunction"], rule["vortex_refine"]
    s._post = None
    vortex = s.compute_vortex_metrics()
    return SimpleNamespace(**{k: float(vortex.get(k, 0.0)) for k in _VORTEX_KEYS}), s.vortex_refine_status


def botella(sizes, res, tolerance, cap, emit):
    from solvers import validation as V
    from solvers.fv.batched import BatchedFVSolver
    trials = [dict(YAML, nx=n, ny=n, Re=float(re), tolerance=tolerance, max_iterations=cap, check_every=256,
                   vortex_metrics="device") for n in sizes for re in res]
    batch = BatchedFVSolver(trials)
    t0 = time.perf_counter()
    batch.solve()
    wall = time.perf_counter() - t0
    text = ["", "## Botella rows of converged trials by the three rules (tools/fv_wall_post_perf.py)", "",
            f"One batch of {len(trials)} `mapping=\"cu\"` trials (TVD, 0.4 / 0.2, tolerance {tolerance:g}, at most {cap} "
            f"iterations), {wall:.1f} s; the rules are applied to the same final state.  Errors in per cent of Botella's "
            f"value as `validation_table` prints them (x and y as relative errors too); the objective is "
            f"`compute_botella_vortex_objective`.", "",
            "| N | Re | iterations | converged | rule | psi_min | err | omega_center err | x err | y err | BR psi err | BR omega err "
            "| BL psi err | BL omega err | objective | status |", "|" + "---|" * 16]
    for s, t in zip(batch.solvers, trials):
        for name, rule in RULES:
            m, status = metrics_by(s, rule)
            rows = {(r["Vortex"], r["Metric"]): r["Error (%)"] for r in V.botella_table(m, int(t["Re"]))}
            obj = V.compute_botella_vortex_objective(m, int(t["Re"]))
            rec = dict(kind="botella", N=t["nx"], Re=t["Re"], iterations=int(s.metrics.iterations),
                       converged=bool(s.metrics.converged), rule=name, objective=obj, status=status,
                       metrics=vars(m), errors_percent={f"{a} {b}": e for (a, b), e in rows.items()})
            emit(rec)
            g = lambda a, b: rows.get((a, b), "-")        # noqa: E731
            text.append(f"| {t['nx']} | {t['Re']:g} | {rec['iterations']} | {rec['converged']} | {name} | {m.psi_min:.6f} | "
                        f"{g('Primary', '|ψ|')} | {g('Primary', '|ω|')} | {g('Primary', 'x')} | {g('Primary', 'y')} | "
                        f"{g('BR', '|ψ|')} | {g('BR', '|ω|')} | {g('BL', '|ψ|')} | {g('BL', '|ω|')} | {obj:.3e} | "
                        f"{status if status is not None else '-'} |")
            print(text[-1], flush=True)
    batch.close()
    return text


def chain(chain_sizes, jobs, jobs_size, rounds, calls, emit):
    import torch
    from solvers.fv import ldc_fv_lib as F
    from solvers.fv.solver import wall_eig
    dev = torch.device("cuda:0")
    f64 = dict(dtype=torch.float64, device=dev)
    keep = []

    def job(n, seed):
        rng = np.random.default_rng(seed)
        lam, Cm = wall_eig(n, dev)
        t = dict(u=torch.tensor(rng.normal(size=n * n), **f64), v=torch.tensor(rng.normal(size=n * n), **f64),
                 ulid=torch.ones(n, **f64), psi=torch.zeros(n * n, **f64), omega=torch.zeros(n * n, **f64),
                 scratch=torch.zeros(F.wall_scratch_len(n, n), **f64), result=torch.zeros(F.WALL_RESULT_LEN, **f64))
        keep.append(t)
        return F.WallJob(u=t["u"].data_ptr(), v=t["v"].data_ptr(), ulid=t["ulid"].data_ptr(), Cx=Cm.data_ptr(),
                         lamx=lam.data_ptr(), Cy=Cm.data_ptr(), lamy=lam.data_ptr(), psi=t["psi"].data_ptr(),
                         omega=t["omega"].data_ptr(), scratch=t["scratch"].data_ptr(), result=t["result"].data_ptr(),
                         dx=1.0 / n, dy=1.0 / n, nx=n, ny=n, ix_lt=n // 2, ix_gt=n - n // 2, jy_lt=n // 2, jy_gt=n - n // 2,
                         refine=1, pad=0)

    cases = {f"1 job of {n}^2": [job(n, n)] for n in chain_sizes}
    cases[f"{jobs} jobs of {jobs_size}^2"] = [job(jobs_size, 7000 + q) for q in range(jobs)]
    stream = torch.cuda.current_stream(dev).cuda_stream

    def call(js):
        t0 = time.perf_counter()
        F.wall_post_enqueue(js, stream)
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0

    for js in cases.values():
        call(js)
    times = {k: [] for k in cases}
    for _ in range(rounds):
        for k, js in cases.items():
            times[k].append(sum(call(js) for _ in range(calls)) / calls)
    text = ["", "## The chain's time (tools/fv_wall_post_perf.py)", "",
            f"Seconds per `ldc_fv_wall_post_enqueue` call, wait included (host clock around enqueue + synchronise), seeded "
            f"states, `refine = 1`; {rounds} rounds of {calls} calls, the cases alternating round by round; each case ran "
            f"once before the clock started.", "", "| case | launches | mean of each round (s) | best | worst |", "|---|---|---|---|---|"]
    for k, ts in times.items():
        launches = F.lib().ldc_fv_wall_post_launches(len(cases[k]))
        emit(dict(kind="chain", case=k, launches=launches, seconds=ts))
        text.append(f"| {k} | {launches} | {' / '.join(f'{t:.3e}' for t in ts)} | {min(ts):.3e} | {max(ts):.3e} |")
        print(text[-1], flush=True)
    return text


UNITS = ("ldc_kernels", "ldc_fv_post", "ldc_fv_prolong", "ldc_fv_anderson", "ldc_fv_wide", "ldc_vortex_refine",
         "ldc_fv_sample", "ldc_fv_cu_pressure")


def device_code_hashes(tree):
    """{unit: sha256 of the disassembly of its gfx950 code object} for the eight units from before, from the sources of
    ``tree`` (a checkout of this repository).  csrc/ and include/ are copied to ONE scratch directory first, so that two
    trees are compiled at the same path (a path in the code object would otherwise differ).  Needs hipcc, no GPU."""
    import hashlib
    import os
    import shutil
    import subprocess
    import tempfile
    from concurrent.futures import ThreadPoolExecutor
    tree = Path(tree)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objdump = os.environ.get("LLVM_OBJDUMP", "/opt/rocm/llvm/bin/llvm-objdump")
    work = Path(tempfile.gettempdir()) / "ldc_fv_wall_post_hashes"
    shutil.rmtree(work, ignore_errors=True)
    shutil.copytree(tree / "02689-advancednumericalalgorithmp3_amd" / "csrc", work / "csrc")
    shutil.copytree(tree / "include", work / "include")

    def one(unit):
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "--no-gpu-bundle-output",
                        "-c", "-I", "include", f"csrc/{unit}.hip", "-o", f"{unit}.co"], cwd=work, check=True)
        dis = subprocess.run([objdump, "-d", f"{unit}.co"], cwd=work, check=True, capture_output=True, text=True).stdout
        kept = "".join(line + "\n" for line in dis.split("\n")[:-1] if "file format" not in line)
        return hashlib.sha256(kept.encode()).hexdigest()

    with ThreadPoolExecutor(max_workers=len(UNITS)) as ex:
        out = dict(zip(UNITS, ex.map(one, UNITS)))
    shutil.rmtree(work, ignore_errors=True)
    return out


def hashes(parent_tree, emit):
    """The table of device-code hashes, the parent's checkout at ``parent_tree`` against this tree."""
    parent, this = device_code_hashes(parent_tree), device_code_hashes(ROOT)
    text = ["", "## The device code of the eight units from before", "",
            "`hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only --no-gpu-bundle-output -c -I include csrc/X.hip -o "
            "X.co`, then `llvm-objdump -d X.co | grep -v 'file format' | sha256sum`, both trees built at the same path (the "
            "method of profiles/fv_cu_pressure.md; `tools/fv_wall_post_perf.py --parent-tree DIR` runs it), parent against "
            "this commit:", "", "| unit | parent | this commit |", "|---|---|---|"]
    for unit in UNITS:
        emit(dict(kind="hash", unit=unit, parent=parent[unit], this=this[unit]))
        text.append(f"| `{unit}.hip` | {parent[unit]} | {'the same' if this[unit] == parent[unit] else this[unit]} |")
        print(text[-1], flush=True)
    return text


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,128")
    ap.add_argument("--res", default="100,400,1000")
    ap.add_argument("--tolerance", type=float, default=1e-6)
    ap.add_argument("--max-iterations", type=int, default=20000)
    ap.add_argument("--chain-sizes", default="64,256,1024")
    ap.add_argument("--jobs", type=int, default=256)
    ap.add_argument("--jobs-size", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit: hash the device code of both")
    ap.add_argument("--skip", default="", help="comma list of: botella, chain")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "fv_wall_post.md"))
    ap.add_argument("--jsonl", default=str(ROOT / "profiles" / "fv_wall_post.jsonl"))
    a = ap.parse_args()
    ints = lambda s: [int(x) for x in s.split(",") if x]          # noqa: E731
    skip = set(a.skip.split(","))
    records = []
    text = []
    if a.parent_tree:
        text += hashes(a.parent_tree, records.append)
    if not {"botella", "chain"} <= skip:
        import __graft_entry__ as g
        g.build()
    if "botella" not in skip:
        text += botella(ints(a.sizes), ints(a.res), a.tolerance, a.max_iterations, records.append)
    if "chain" not in skip:
        text += chain(ints(a.chain_sizes), a.jobs, a.jobs_size, a.rounds, a.calls, records.append)
    with Path(a.out).open("a") as f:
        f.write("\n".join(text) + "\n")
    with Path(a.jsonl).open("a") as f:
        for r in records:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
