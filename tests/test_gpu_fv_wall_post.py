"""The wall-anchored finite-volume post-processing on the GPU (ldc_fv_wall_post_enqueue, ``streamfunction="wall"``,
``vortex_refine="quadratic"``).  The yardstick is the NumPy statement of tests/fv_wall_post_numpy.py: omega in fp64, psi by
its long-double solve, the extrema and the refinement applied to the device's own psi and omega; and, for the mapping,
the same job alone."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import fv_wall_post_numpy as W  # noqa: E402
from fv_wall_post_numpy import EPS, LD  # noqa: E402

from conftest import PKG  # noqa: E402

pytestmark = pytest.mark.gpu

YAML = dict(name="fv", convection_scheme="TVD", alpha_uv=0.4, alpha_p=0.2, linear_solver_tol=1e-9)      # conf/solver/fv.yaml
REFINED_TOL = 1e-13          # a kernel without contraction against its NumPy statement (the prolongation test's tolerance)


@pytest.fixture(scope="module")
def fv():
    import __graft_entry__ as g
    g.build()
    from solvers.fv.batched import BatchedFVSolver
    from solvers.fv.solver import FVSolver
    return FVSolver, BatchedFVSolver


def _state(kind, nx, ny, Lx, Ly):
    if kind == "manufactured":
        return W.manufactured(nx, ny, Lx, Ly)[:3]
    return W.smooth_state(nx, ny)


def _run(cases, refine=1):
    """ONE ldc_fv_wall_post_enqueue call for ``cases`` = [(nx, ny, Lx, Ly, u, v, ulid)]: per case (psi, omega, block)."""
    import torch
    from solvers.fv import ldc_fv_lib as F
    from solvers.fv.solver import wall_eig
    dev = torch.device("cuda:0")
    f64 = dict(dtype=torch.float64, device=dev)
    keep, jobs = [], []
    for nx, ny, Lx, Ly, u, v, ulid in cases:
        xs, ys = W.cell_centres(nx, ny, Lx, Ly)
        ix_lt, ix_gt, jy_lt, jy_gt = W.mask_bounds(xs, ys)
        lamx, Cx = wall_eig(nx, dev)
        lamy, Cy = wall_eig(ny, dev)
        t = dict(u=torch.tensor(np.ascontiguousarray(u).ravel(), **f64), v=torch.tensor(np.ascontiguousarray(v).ravel(), **f64),
                 ulid=torch.tensor(np.ascontiguousarray(ulid), **f64), psi=torch.full((nx * ny,), np.nan, **f64),
                 omega=torch.full((nx * ny,), np.nan, **f64), scratch=torch.full((F.wall_scratch_len(nx, ny),), np.nan, **f64),
                 result=torch.full((F.WALL_RESULT_LEN,), np.nan, **f64))
        keep.append(t)
        jobs.append(F.WallJob(u=t["u"].data_ptr(), v=t["v"].data_ptr(), ulid=t["ulid"].data_ptr(), Cx=Cx.data_ptr(),
                              lamx=lamx.data_ptr(), Cy=Cy.data_ptr(), lamy=lamy.data_ptr(), psi=t["psi"].data_ptr(),
                              omega=t["omega"].data_ptr(), scratch=t["scratch"].data_ptr(), result=t["result"].data_ptr(),
                              dx=Lx / nx, dy=Ly / ny, nx=nx, ny=ny, ix_lt=ix_lt, ix_gt=ix_gt, jy_lt=jy_lt, jy_gt=jy_gt,
                              refine=refine, pad=0))
    F.wall_post_enqueue(jobs, torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    return [(t["psi"].cpu().numpy().reshape(c[1], c[0]), t["omega"].cpu().numpy().reshape(c[1], c[0]),
             t["result"].cpu().numpy()) for t, c in zip(keep, cases)]


def _assert_block_is_the_statement(block, psi, om, nx, ny, Lx, Ly, refine=1, what=""):
    """Slots 0 .. 15 exactly (cells and values are picks of the device's own fields); the groups' statuses exactly and
    their values within REFINED_TOL max(1, |value|).  Returns the largest scaled difference."""
    xs, ys = W.cell_centres(nx, ny, Lx, Ly)
    want = W.result_block(psi, om, W.mask_bounds(xs, ys), Lx / nx, Ly / ny, refine=refine)
    assert np.array_equal(block[:W.POST_LEN], want[:W.POST_LEN]), (what, block[:W.POST_LEN], want[:W.POST_LEN])
    worst = 0.0
    for name, got in W.block_groups(block).items():
        ref = W.block_groups(want)[name]
        assert got[W.G_STATUS] == ref[W.G_STATUS], (what, name, got, ref)
        scaled = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
        worst = max(worst, float(scaled.max()))
        assert np.all(scaled <= REFINED_TOL), (what, name, got, ref)
        if got[W.G_STATUS] != 0:                    # the cell's own values, bit for bit
            assert np.array_equal(got, ref), (what, name, got, ref)
    return worst


# ------------------------------------------------------------------------------------------- 1. the entry, job by job
@pytest.mark.parametrize("shape", W.GPU_SHAPES, ids=W.shape_id)
def test_entry_against_the_statement(fv, shape):
    """omega within 4 eps max(|u|, |v|, lid)(1/dx + 1/dy) of the statement, psi within 4 eps kappa max|psi| of its
    long-double solve, the extremum cells the statement's on the device's fields, the groups within 1e-13."""
    nx, ny, Lx, Ly = shape
    dx, dy = Lx / nx, Ly / ny
    states = {kind: _state(kind, nx, ny, Lx, Ly) for kind in ("seeded", "manufactured")}
    out = _run([(nx, ny, Lx, Ly, *st) for st in states.values()])
    for (kind, (u, v, ulid)), (psi, om, block) in zip(states.items(), out):
        om_ref = W.omega(u, v, ulid, dx, dy)
        psi_ld = W.psi_solve(om_ref, dx, dy, LD)
        bw, bp = W.omega_bound(u, v, ulid, dx, dy), W.psi_bound(psi_ld, nx, ny, dx, dy)
        ew, ep = float(np.max(np.abs(om - om_ref))), float(np.max(np.abs(psi.astype(LD) - psi_ld)))
        assert np.all(np.isfinite(om)) and np.all(np.isfinite(psi)) and block[W.NONFINITE] == 0
        worst = _assert_block_is_the_statement(block, psi, om, nx, ny, Lx, Ly, what=(shape, kind))
        k = W.kappa(nx, ny, dx, dy)
        print(f"FVWALL {nx}x{ny} {kind}: omega err {ew:.2e} (bound {bw:.2e}); psi err {ep:.2e}, kappa {k:.2e}, share of eps "
              f"kappa max|psi| {ep / (EPS * k * float(np.max(np.abs(psi_ld)))):.3f} (bound 4); groups {worst:.2e} (bound 1e-13); "
              f"status {[int(g[W.G_STATUS]) for g in W.block_groups(block).values()]}")
        assert ew <= bw
        assert ep <= bp
    # refine = 0: the same fields and slots, the cells' own values with status -1
    (psi0, om0, block0), = _run([(nx, ny, Lx, Ly, *states["manufactured"])], refine=0)
    assert np.array_equal(psi0, out[1][0]) and np.array_equal(om0, out[1][1])
    assert np.array_equal(block0[:W.POST_LEN], out[1][2][:W.POST_LEN])
    _assert_block_is_the_statement(block0, psi0, om0, nx, ny, Lx, Ly, refine=0, what=(shape, "refine=0"))
    assert all(g[W.G_STATUS] == -1 for g in W.block_groups(block0).values())


def test_manufactured_centre_on_the_device(fv):
    """The refined primary centre of the 16 x 16 manufactured field is a quarter as far from the exact one as the snapped."""
    u, v, ulid, _ = W.manufactured(16, 16)
    (_, _, block), = _run([(16, 16, 1.0, 1.0, u, v, ulid)])
    (_, _, snapped), = _run([(16, 16, 1.0, 1.0, u, v, ulid)], refine=0)
    dist = lambda b: float(np.hypot(b[W.POST_LEN + W.G_X] - W.EXACT_CENTRE[0], b[W.POST_LEN + W.G_Y] - W.EXACT_CENTRE[1]))   # noqa: E731
    print(f"16x16: snapped {dist(snapped):.3e}, refined {dist(block):.3e}")
    assert block[W.POST_LEN + W.G_STATUS] == 0 and dist(block) <= dist(snapped) / 4


def test_status_codes(fv):
    """The status cases of the CPU test through the whole chain, all in one call: the device's statuses are the
    statement's on the device's own psi, and the ones the fields were built for."""
    nx, ny = 12, 10
    dx, dy = 1.0 / nx, 1.0 / ny
    fields = W.status_fields(nx, ny)
    cases = [(nx, ny, 1.0, 1.0, *W.state_for_psi(target, dx, dy)) for target, _ in fields.values()]
    u, v, ulid = W.state_for_psi(fields["corner"][0], dx, dy)
    u = u.copy()
    u[7, 7] = np.nan
    cases.append((nx, ny, 1.0, 1.0, u, v, ulid))
    out = _run(cases)
    seen = set()
    for (name, (target, want)), (psi, om, block) in zip(fields.items(), out):
        _assert_block_is_the_statement(block, psi, om, nx, ny, 1.0, 1.0, what=name)
        got = [int(g[W.G_STATUS]) for g in W.block_groups(block).values()]
        print(name, got, "max|psi - target|", float(np.max(np.abs(psi - target))))
        assert all(w is None or g == w for g, w in zip(got, want)), (name, got, want)
        seen.update(got)
    assert {0, 1, 2, 3} <= seen
    psi, om, block = out[-1]                          # the NaN: the flag, status 1 four times
    assert block[W.NONFINITE] == 1 and np.isnan(om).any()
    assert [int(g[W.G_STATUS]) for g in W.block_groups(block).values()] == [1, 1, 1, 1]


# ------------------------------------------------------------------------------------------- 2. jobs share launches
def test_26_jobs_in_one_call_are_the_jobs_alone(fv):
    from solvers.fv import ldc_fv_lib as F
    shapes = [(8, 8, 1.0, 1.0), (13, 17, 1.0, 1.0), (24, 16, 2.0, 0.5), (33, 20, 1.0, 1.0), (260, 9, 1.0, 1.0),
              (9, 260, 1.0, 1.0), (40, 40, 1.0, 1.0)]
    cases = []
    for q in range(26):
        nx, ny, Lx, Ly = shapes[q % len(shapes)] if q != 11 else (1024, 8, 1.0, 1.0)
        cases.append((nx, ny, Lx, Ly, *W.smooth_state(nx, ny, seed=100 + q)))
    assert F.lib().ldc_fv_wall_post_launches(len(cases)) >= 14          # at least two launch groups
    together, again = _run(cases), _run(cases)
    for q in range(len(cases)):                       # every job, alone in a call of its own
        alone, = _run([cases[q]])
        for a, b, c in zip(alone, together[q], again[q]):
            assert np.array_equal(a, b, equal_nan=True) and np.array_equal(b, c, equal_nan=True), q
    for q, ((psi, om, block), case) in enumerate(zip(together, cases)):
        assert np.array_equal(block, again[q][2]) and np.array_equal(psi, again[q][0]), q
        _assert_block_is_the_statement(block, psi, om, *case[:4], what=q)


# ------------------------------------------------------------------------------------------- 3. solvers
def _wall(**kw):
    return dict(YAML, Re=100.0, nx=16, ny=16, max_iterations=200, tolerance=1e-30, check_every=64, streamfunction="wall",
                vortex_refine="quadratic", **kw)


def _statement_metrics(s):
    psi, om = s.streamfunction(), s.vorticity()
    block = W.result_block(psi, om, s._mask_bounds, s.dx_min, s.dy_min, refine=int(s.params.vortex_refine == "quadratic"))
    return W.metrics(block, s.nx, s.dx_min, s.dy_min), block, psi, om


def _assert_metrics_are_the_statement(s, got):
    want, block, psi, om = _statement_metrics(s)
    for k, v in want.items():
        assert abs(got[k] - v) <= REFINED_TOL * max(1.0, abs(v)), (k, got[k], v)
    st = s.state()
    om_ref = W.omega(st["u"].reshape(s.ny, s.nx), st["v"].reshape(s.ny, s.nx), s.t["ulid"].cpu().numpy(), s.dx_min, s.dy_min)
    assert float(np.max(np.abs(om - om_ref))) <= W.omega_bound(st["u"], st["v"], s.t["ulid"].cpu().numpy(), s.dx_min, s.dy_min)
    psi_ld = W.psi_solve(om_ref, s.dx_min, s.dy_min, LD)
    assert float(np.max(np.abs(psi.astype(LD) - psi_ld))) <= W.psi_bound(psi_ld, s.nx, s.ny, s.dx_min, s.dy_min)
    return want, block


@pytest.mark.parametrize("mapping", ["cu", "chip"])
def test_solver_metrics_are_the_statement_on_the_final_state(fv, mapping):
    FVSolver, _ = fv
    s = FVSolver(**_wall(mapping=mapping))
    s.solve()
    m = s.metrics.as_dict()
    assert s.metrics.iterations == 200 and m["psi_min"] < 0
    want, block = _assert_metrics_are_the_statement(s, m)
    assert s.vortex_refine_status == tuple(int(g[W.G_STATUS]) for g in W.block_groups(block).values())
    assert s.vortex_refine_status[0] == 0
    xs, ys = W.cell_centres(16, 16)
    assert m["psi_min_x"] not in xs and m["psi_min_y"] not in ys                  # a sub-cell centre
    print(mapping, {k: m[k] for k in ("psi_min", "psi_min_x", "psi_min_y", "omega_center", "psi_BR", "omega_BR")},
          s.vortex_refine_status)
    plain = FVSolver(**dict(_wall(mapping=mapping), vortex_refine="none"))
    plain.set_state(**s.state())
    plain._finalize_fields()
    snapped = plain.compute_vortex_metrics()
    assert plain.vortex_refine_status is None and snapped["psi_min_x"] in xs and snapped["psi_min_y"] in ys
    assert snapped["psi_min"] >= m["psi_min"] and snapped["omega_max"] == m["omega_max"]
    _assert_metrics_are_the_statement(plain, snapped)
    s.close()
    plain.close()


@pytest.mark.parametrize("mapping", ["cu", "chip"])
def test_a_solve_goes_on_after_the_post_processing_as_if_nothing_had_happened(fv, mapping):
    FVSolver, _ = fv
    from solvers.fv.solver import postprocess
    a, b = (FVSolver(**_wall(mapping=mapping)) for _ in range(2))
    rows = {}
    for s in (a, b):
        s._begin(1e-30)
        rows[s] = [s._advance(20)[0]]
    postprocess([a])
    assert a._post is not None and len(a._post) == W.RESULT_LEN and a._post[0] < 0 and b._post is None
    for s in (a, b):
        rows[s].append(s._advance(20)[0])
    sa, sb = a.state(), b.state()
    for k in ("u", "v", "p", "mdot"):
        assert np.array_equal(sa[k], sb[k]), k
    assert np.array_equal(np.concatenate(rows[a]), np.concatenate(rows[b])) and np.concatenate(rows[a]).shape == (40, 8)
    assert a.counters() == b.counters() and a.counters()["iterations"] == 40
    a.close()
    b.close()


def _solve_metrics(s):
    m = s.metrics.as_dict()
    m.pop("wall_time_seconds")
    return m


def _assert_batch_is_its_lone_runs(FVSolver, BatchedFVSolver, trials):
    batch = BatchedFVSolver(trials)
    batch.solve()
    assert batch.errors == {}
    out = []
    for q, (b, t) in enumerate(zip(batch.solvers, trials)):
        lone = FVSolver(**t)
        lone.solve()
        sb, sl = b.state(), lone.state()
        for k in ("u", "v", "p", "mdot"):
            assert np.array_equal(sb[k], sl[k]), (q, k)
        assert _solve_metrics(b) == _solve_metrics(lone), q                 # bit for bit, vortex metrics included
        out.append((_solve_metrics(b), lone))
    return batch, out


def test_a_wall_trial_and_a_reference_trial_in_one_batch(fv):
    FVSolver, BatchedFVSolver = fv
    trials = [dict(_wall(), nx=24, ny=16, corner_treatment="saad"),
              dict(YAML, Re=100.0, nx=8, ny=8, max_iterations=200, tolerance=1e-30, check_every=64, vortex_metrics="device")]
    batch, out = _assert_batch_is_its_lone_runs(FVSolver, BatchedFVSolver, trials)
    (mw, lone_w), (mr, lone_r) = out
    _assert_metrics_are_the_statement(batch.solvers[0], mw)
    assert mw["psi_min"] < 0 and batch.solvers[0].vortex_refine_status[0] == 0
    # the reference trial: the parent's rule, read off a device post-processing of its own
    from solvers.fv.solver import postprocess
    postprocess([lone_r])
    assert len(lone_r._post) == 16
    ref = lone_r._device_vortex_metrics()
    assert {k: mr[k] for k in ref} == ref and mr["omega_BR"] == 0.0 and batch.solvers[1].vortex_refine_status is None
    psi = lone_r.streamfunction()
    assert np.all(psi[0] == 0.0) and np.all(psi[:, 0] == 0.0)                     # the ring rule's psi
    for _, lone in out:
        lone.close()
    batch.close()


def test_a_shared_batch_of_two_wall_trials(fv):
    FVSolver, BatchedFVSolver = fv
    trials = [dict(_wall(mapping="shared")), dict(_wall(mapping="shared"), nx=24, ny=20, Re=400.0)]
    batch, out = _assert_batch_is_its_lone_runs(FVSolver, BatchedFVSolver, trials)
    for s, (m, lone) in zip(batch.solvers, out):
        _assert_metrics_are_the_statement(s, m)
        assert m["psi_min"] < 0 and s.vortex_refine_status[0] == 0
        lone.close()
    batch.close()


def test_the_launcher_takes_the_two_options(tmp_path):
    r = subprocess.run([sys.executable, str(PKG / "main.py"), "solver=fv", "N=16", "Re=100", "max_iterations=200",
                        "+solver.streamfunction=wall", "+solver.vortex_refine=quadratic"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = json.loads(next(tmp_path.rglob("results.json")).read_text())
    assert rec["params"]["streamfunction"] == "wall" and rec["params"]["vortex_refine"] == "quadratic"
    m = rec["metrics"]
    print({k: m.get(k) for k in ("psi_min", "psi_min_x", "psi_BR", "omega_BR", "psi_BL", "omega_BL")})
    assert m["psi_min"] < 0 and m["psi_BR"] > 0 and m["omega_BR"] != 0.0
