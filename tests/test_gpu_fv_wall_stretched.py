"""The wall-anchored finite-volume post-processing on stretched grids on the GPU (ldc_fv_wall_stretched_post_enqueue,
``grid="tanh"`` with ``streamfunction="wall_stretched"``, ``vortex_refine="quadratic"``).  The yardstick is the NumPy statement of
tests/fv_wall_stretched_numpy.py: omega in fp64, psi by a long-double direct solve of the same operator, the extrema and the
refinement applied to the device's own psi and omega; at beta = 0 the uniform entry; and, for the mapping, the same job alone."""
import functools
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import fv_wall_post_numpy as W  # noqa: E402
import fv_wall_stretched_numpy as S  # noqa: E402
from fv_wall_stretched_numpy import EPS, LD  # noqa: E402

from conftest import PKG  # noqa: E402

pytestmark = pytest.mark.gpu

YAML = dict(name="fv", convection_scheme="TVD", alpha_uv=0.4, alpha_p=0.2, linear_solver_tol=1e-9)      # conf/solver/fv.yaml
REFINED_TOL = 1e-13          # the value of tests/test_gpu_fv_wall_post.py: a kernel without contraction against its NumPy statement


@pytest.fixture(scope="module")
def fv():
    import __graft_entry__ as g
    g.build()
    from solvers.fv.batched import BatchedFVSolver
    from solvers.fv.solver import FVSolver
    return FVSolver, BatchedFVSolver


@functools.lru_cache(maxsize=None)
def _axis(n, beta):
    """(axis, (lam, Q)) of n cells on the unit interval: computed once, shared by every test."""
    ax = S.axis(n, 1.0, beta)
    return ax, S.dirichlet_eig(ax, tridiagonal=n > 256)


@functools.lru_cache(maxsize=None)
def _tables(n, beta):
    """The two device tables of an axis, uploaded once."""
    import torch
    ax, eig = _axis(n, beta)
    f64 = dict(dtype=torch.float64, device=torch.device("cuda:0"))
    return torch.tensor(S.grid_table(ax), **f64), torch.tensor(S.post_table(ax, eig), **f64)


@functools.lru_cache(maxsize=None)
def _manufactured(nx, ny, beta):
    """(u, v, ulid), the statement's omega and the long-double psi of the manufactured field: computed once."""
    (ax, _), (ay, _) = _axis(nx, beta), _axis(ny, beta)
    u, v, ulid, _ = S.manufactured(ax, ay)
    om = S.omega(u, v, ulid, ax, ay)
    return (u, v, ulid), om, S.psi_solve_ld(om, ax, ay)


def _run(cases):
    """ONE ldc_fv_wall_stretched_post_enqueue call for ``cases`` = [(nx, ny, beta, refine, u, v, ulid)]: per case
    (psi, omega, block).  Jobs of equal axes share their tables."""
    import torch
    from solvers.fv import ldc_fv_lib as F
    dev = torch.device("cuda:0")
    f64 = dict(dtype=torch.float64, device=dev)
    keep, jobs = [], []
    for nx, ny, beta, refine, u, v, ulid in cases:
        (ax, _), (ay, _) = _axis(nx, beta), _axis(ny, beta)
        ix_lt, ix_gt, jy_lt, jy_gt = S.mask_bounds(ax, ay)
        (gx, px), (gy, py) = _tables(nx, beta), _tables(ny, beta)
        assert gx.numel() == F.grid_table_len(nx) and px.numel() == F.wall_stretched_table_len(nx)
        assert gy.numel() == F.grid_table_len(ny) and py.numel() == F.wall_stretched_table_len(ny)
        t = dict(u=torch.tensor(np.ascontiguousarray(u).ravel(), **f64), v=torch.tensor(np.ascontiguousarray(v).ravel(), **f64),
                 ulid=torch.tensor(np.ascontiguousarray(ulid), **f64), psi=torch.full((nx * ny,), np.nan, **f64),
                 omega=torch.full((nx * ny,), np.nan, **f64), scratch=torch.full((F.wall_scratch_len(nx, ny),), np.nan, **f64),
                 result=torch.full((F.WALL_RESULT_LEN,), np.nan, **f64))
        assert t["u"].numel() == t["v"].numel() == nx * ny and t["ulid"].numel() == nx
        keep.append(t)
        jobs.append(F.WallStretchedJob(u=t["u"].data_ptr(), v=t["v"].data_ptr(), ulid=t["ulid"].data_ptr(),
                                       x_grid=gx.data_ptr(), y_grid=gy.data_ptr(), x_post=px.data_ptr(), y_post=py.data_ptr(),
                                       psi=t["psi"].data_ptr(), omega=t["omega"].data_ptr(), scratch=t["scratch"].data_ptr(),
                                       result=t["result"].data_ptr(), nx=nx, ny=ny, ix_lt=ix_lt, ix_gt=ix_gt, jy_lt=jy_lt,
                                       jy_gt=jy_gt, refine=refine, pad=0))
    F.wall_stretched_post_enqueue(jobs, torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    return [(t["psi"].cpu().numpy().reshape(c[1], c[0]), t["omega"].cpu().numpy().reshape(c[1], c[0]),
             t["result"].cpu().numpy()) for t, c in zip(keep, cases)]


def _assert_block_is_the_statement(block, psi, om, nx, ny, beta, refine=1, what=""):
    """Slots 0 .. 15 exactly (cells and values are picks of the device's own fields); the groups' statuses exactly and
    their values within REFINED_TOL max(1, |value|).  Returns the largest scaled difference."""
    (ax, _), (ay, _) = _axis(nx, beta), _axis(ny, beta)
    want = S.result_block(psi, om, S.mask_bounds(ax, ay), ax, ay, refine=refine)
    assert np.array_equal(block[:S.POST_LEN], want[:S.POST_LEN]), (what, block[:S.POST_LEN], want[:S.POST_LEN])
    worst = 0.0
    for name, got in S.block_groups(block).items():
        ref = S.block_groups(want)[name]
        assert got[S.G_STATUS] == ref[S.G_STATUS], (what, name, got, ref)
        scaled = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
        worst = max(worst, float(scaled.max()))
        assert np.all(scaled <= REFINED_TOL), (what, name, got, ref)
        if got[S.G_STATUS] != 0:                    # the cell's own values, bit for bit
            assert np.array_equal(got, ref), (what, name, got, ref)
    return worst


# ------------------------------------------------------------------------------------------- 1. the entry, job by job
@pytest.mark.parametrize("beta", S.BETAS)
@pytest.mark.parametrize("shape", S.GPU_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_entry_against_the_statement(fv, shape, beta):
    """omega within the statement's rounding bound, psi within 4 eps kappa max|psi| of the long-double solve, the extremum
    cells the statement's on the device's fields, the groups within 1e-13; both refine values, two jobs of one call."""
    nx, ny = shape
    (ax, ex), (ay, ey) = _axis(nx, beta), _axis(ny, beta)
    (u, v, ulid), om_ref, psi_ld = _manufactured(nx, ny, beta)
    (psi, om, block), (psi0, om0, block0) = _run([(nx, ny, beta, 1, u, v, ulid), (nx, ny, beta, 0, u, v, ulid)])
    bw, bp = S.omega_bound(u, v, ulid, ax, ay), S.psi_bound(psi_ld, ax, ay, (ex, ey))
    ew, ep = float(np.max(np.abs(om - om_ref))), float(np.max(np.abs(psi.astype(LD) - psi_ld)))
    assert np.all(np.isfinite(om)) and np.all(np.isfinite(psi)) and block[W.NONFINITE] == 0
    worst = _assert_block_is_the_statement(block, psi, om, nx, ny, beta, what=(shape, beta))
    k = S.kappa(ax, ay, (ex, ey))
    print(f"FVWS {nx}x{ny} beta {beta}: omega err {ew:.2e} (bound {bw:.2e}); psi err {ep:.2e}, kappa {k:.2e}, share of eps kappa "
          f"max|psi| {ep / (EPS * k * float(np.max(np.abs(psi_ld)))):.3f} (bound 4); groups {worst:.2e} (bound 1e-13); status "
          f"{S.statuses(block)}")
    assert ew <= bw
    assert ep <= bp
    assert S.statuses(block)[0] == 0
    # refine = 0: the same fields and slots, the cells' own values with status -1
    assert np.array_equal(psi0, psi) and np.array_equal(om0, om)
    assert np.array_equal(block0[:S.POST_LEN], block[:S.POST_LEN])
    _assert_block_is_the_statement(block0, psi0, om0, nx, ny, beta, refine=0, what=(shape, beta, "refine=0"))
    assert S.statuses(block0) == (-1, -1, -1, -1)


@pytest.mark.parametrize("shape", [(13, 17), (37, 50), (64, 16)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_beta_zero_is_the_uniform_entry(fv, shape):
    """The same state through the new entry and through ldc_fv_wall_post_enqueue: psi within the sum of the two entries'
    bounds, the cells and statuses identical."""
    import torch
    from solvers.fv import ldc_fv_lib as F
    from solvers.fv.solver import wall_eig
    nx, ny = shape
    dx, dy = 1.0 / nx, 1.0 / ny
    (ax, ex), (ay, ey) = _axis(nx, 0.0), _axis(ny, 0.0)
    (u, v, ulid), _, psi_ld = _manufactured(nx, ny, 0.0)
    out = []
    for refine in (1, 0):
        (psi_s, om_s, block_s), = _run([(nx, ny, 0.0, refine, u, v, ulid)])
        dev = torch.device("cuda:0")
        f64 = dict(dtype=torch.float64, device=dev)
        (lamx, Cx), (lamy, Cy) = wall_eig(nx, dev), wall_eig(ny, dev)
        t = dict(u=torch.tensor(u.ravel(), **f64), v=torch.tensor(v.ravel(), **f64), ulid=torch.tensor(ulid, **f64),
                 psi=torch.zeros(nx * ny, **f64), omega=torch.zeros(nx * ny, **f64),
                 scratch=torch.zeros(F.wall_scratch_len(nx, ny), **f64), result=torch.zeros(F.WALL_RESULT_LEN, **f64))
        ix_lt, ix_gt, jy_lt, jy_gt = S.mask_bounds(ax, ay)
        job = F.WallJob(u=t["u"].data_ptr(), v=t["v"].data_ptr(), ulid=t["ulid"].data_ptr(), Cx=Cx.data_ptr(),
                        lamx=lamx.data_ptr(), Cy=Cy.data_ptr(), lamy=lamy.data_ptr(), psi=t["psi"].data_ptr(),
                        omega=t["omega"].data_ptr(), scratch=t["scratch"].data_ptr(), result=t["result"].data_ptr(), dx=dx, dy=dy,
                        nx=nx, ny=ny, ix_lt=ix_lt, ix_gt=ix_gt, jy_lt=jy_lt, jy_gt=jy_gt, refine=refine, pad=0)
        F.wall_post_enqueue([job], torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize(dev)
        psi_u, block_u = t["psi"].cpu().numpy().reshape(ny, nx), t["result"].cpu().numpy()
        both = S.psi_bound(psi_ld, ax, ay, (ex, ey)) + W.psi_bound(psi_ld, nx, ny, dx, dy)
        diff = float(np.max(np.abs(psi_s - psi_u)))
        print(f"{nx}x{ny} refine {refine}: |psi_stretched - psi_uniform| {diff:.2e} (bound {both:.2e})")
        assert diff <= both
        cells = [W.PSI_MIN_CELL, W.OMEGA_MAX_CELL, W.PSI_BR_CELL, W.PSI_BR_CELL + 1, W.PSI_BR_CELL + 2, W.NONFINITE]
        assert np.array_equal(block_s[cells], block_u[cells])
        assert S.statuses(block_s) == S.statuses(block_u)
        out.append(S.statuses(block_s))
    assert out[0][0] == 0 and out[1] == (-1, -1, -1, -1)


def _status_cases():
    cases, names = [], []
    for beta in (1.5, 2.5):
        (ax, _), (ay, _) = _axis(12, beta), _axis(10, beta)
        for name, (target, want) in S.status_fields(ax, ay).items():
            cases.append((12, 10, beta, 1, *S.state_for_psi(target, ax, ay)))
            names.append((name, beta, target, want))
    return cases, names


def _nan_case():
    (ax, _), (ay, _) = _axis(12, 1.5), _axis(10, 1.5)
    u, v, ulid = S.state_for_psi(S.status_fields(ax, ay)["corner"][0], ax, ay)
    u = u.copy()
    u[7, 7] = np.nan
    return (12, 10, 1.5, 1, u, v, ulid)


def test_status_codes(fv):
    """The status cases of the CPU test through the whole chain, all in one call with a job that carries a NaN: the device's
    statuses are the statement's on the device's own psi, and the primary ones those the fields were built for; the NaN job
    is flagged and the others are what they are without it."""
    cases, names = _status_cases()
    out = _run(cases + [_nan_case()])
    seen = set()
    for (name, beta, target, want), (psi, om, block) in zip(names, out):
        _assert_block_is_the_statement(block, psi, om, 12, 10, beta, what=(name, beta))
        got = S.statuses(block)
        print(name, beta, got, "max|psi - target|", float(np.max(np.abs(psi - target))))
        assert got[0] == want[0], (name, beta, got, want)      # (a corner of a field that is 0 there is decided by rounding)
        seen.update(got)
    assert {0, 1, 2, 3} <= seen
    psi, om, block = out[-1]                          # the NaN: the flag, status 1 four times
    assert block[W.NONFINITE] == 1 and np.isnan(om).any()
    assert S.statuses(block) == (1, 1, 1, 1)
    without = _run(cases)                             # the other jobs are unaffected, bit for bit
    for a, b in zip(without, out):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_a_nan_alone(fv):
    (psi, om, block), = _run([_nan_case()])
    assert block[W.NONFINITE] == 1 and np.isnan(om).any() and np.isnan(psi).any()
    assert S.statuses(block) == (1, 1, 1, 1)
    (_, _, block0), = _run([_nan_case()[:3] + (0,) + _nan_case()[4:]])
    assert block0[W.NONFINITE] == 1 and S.statuses(block0) == (-1, -1, -1, -1)


# ------------------------------------------------------------------------------------------- 2. jobs share launches
def test_34_jobs_in_one_call_are_the_jobs_alone(fv):
    from solvers.fv import ldc_fv_lib as F
    shapes = [(8, 8), (13, 17), (37, 50), (64, 16), (16, 64), (257, 24), (40, 40)]
    cases = []
    for q in range(F.WALL_STRETCHED_LAUNCH_MAX + 2):
        nx, ny = shapes[q % len(shapes)] if q != 11 else (1024, 9)
        beta = S.BETAS[q % 3] if (nx, ny) != (40, 40) else 1.5
        u, v, ulid = W.smooth_state(nx, ny, seed=100 + q)
        cases.append((nx, ny, beta, q % 2, u, v, ulid))
    assert F.lib().ldc_fv_wall_stretched_post_launches(len(cases)) == 14          # two launch groups
    together, again = _run(cases), _run(cases)
    for q in range(len(cases)):                       # every job, alone in a call of its own
        alone, = _run([cases[q]])
        for a, b, c in zip(alone, together[q], again[q]):
            assert np.array_equal(a, b, equal_nan=True) and np.array_equal(b, c, equal_nan=True), q
    for q, ((psi, om, block), case) in enumerate(zip(together, cases)):
        _assert_block_is_the_statement(block, psi, om, *case[:3], refine=case[3], what=q)


# ------------------------------------------------------------------------------------------- 3. solvers
def _wall(**kw):
    return dict(YAML, Re=100.0, nx=16, ny=16, max_iterations=300, tolerance=1e-30, check_every=64, grid="tanh",
                grid_stretch=1.5, streamfunction="wall_stretched", vortex_refine="quadratic", **kw)


MODES = {"reference": dict(pressure_equation="reference"),
         "consistent_cu": dict(pressure_equation="consistent_cu", pressure_preconditioner="separable")}


def _axes_of(s):
    return S.axis(s.nx, s.params.Lx, float(s.params.grid_stretch)), S.axis(s.ny, s.params.Ly, float(s.params.grid_stretch))


def _assert_metrics_are_the_statement(s, got):
    ax, ay = _axes_of(s)
    psi, om = s.streamfunction(), s.vorticity()       # the device's fields
    block = S.result_block(psi, om, s._mask_bounds, ax, ay, refine=int(s.params.vortex_refine == "quadratic"))
    want = S.metrics(block, ax, ay)
    for k, v in want.items():
        assert abs(got[k] - v) <= REFINED_TOL * max(1.0, abs(v)), (k, got[k], v)
    st = s.state()
    ulid = s.t["ulid"].cpu().numpy()
    u, v = st["u"].reshape(s.ny, s.nx), st["v"].reshape(s.ny, s.nx)
    om_ref = S.omega(u, v, ulid, ax, ay)
    assert float(np.max(np.abs(om - om_ref))) <= S.omega_bound(u, v, ulid, ax, ay)
    psi_ld = S.psi_solve_ld(om_ref, ax, ay)
    assert float(np.max(np.abs(psi.astype(LD) - psi_ld))) <= S.psi_bound(psi_ld, ax, ay)
    return want, block


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("shape", [(16, 16), (13, 17)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_solver_metrics_are_the_statement_on_the_final_state(fv, shape, mode):
    FVSolver, _ = fv
    s = FVSolver(**dict(_wall(**MODES[mode]), nx=shape[0], ny=shape[1]))
    s.solve()
    m = s.metrics.as_dict()
    assert s.metrics.iterations == 300 and m["psi_min"] < 0
    want, block = _assert_metrics_are_the_statement(s, m)
    assert s.vortex_refine_status == S.statuses(block) and s.vortex_refine_status[0] == 0
    ax, ay = _axes_of(s)
    assert m["psi_min_x"] not in ax[0] and m["psi_min_y"] not in ay[0]                  # a sub-cell centre
    print(shape, mode, {k: m[k] for k in ("psi_min", "psi_min_x", "psi_min_y", "omega_center", "psi_BR", "omega_BR")},
          s.vortex_refine_status)
    plain = FVSolver(**dict(_wall(**MODES[mode]), nx=shape[0], ny=shape[1], vortex_refine="none"))
    plain.set_state(**s.state())
    plain._finalize_fields()
    snapped = plain.compute_vortex_metrics()
    assert plain.vortex_refine_status is None and snapped["psi_min_x"] in ax[0] and snapped["psi_min_y"] in ay[0]
    assert snapped["psi_min"] >= m["psi_min"] and snapped["omega_max"] == m["omega_max"]
    _assert_metrics_are_the_statement(plain, snapped)
    # the host ring rule of a streamfunction="reference" trial is what it was: psi = 0 in the ring cells
    ring = FVSolver(**dict(_wall(**MODES[mode]), nx=shape[0], ny=shape[1], streamfunction="reference", vortex_refine="none"))
    ring.set_state(**s.state())
    psi_ring = ring.streamfunction()
    assert np.all(psi_ring[0] == 0.0) and np.all(psi_ring[:, 0] == 0.0) and np.all(s.streamfunction()[0] != 0.0)
    for t in (s, plain, ring):
        t.close()


@pytest.mark.parametrize("mode", list(MODES))
def test_a_solve_goes_on_after_the_post_processing_as_if_nothing_had_happened(fv, mode):
    FVSolver, _ = fv
    from solvers.fv.solver import postprocess
    a, b = (FVSolver(**dict(_wall(**MODES[mode]), nx=13, ny=17)) for _ in range(2))
    rows = {}
    for s in (a, b):
        s._begin(1e-30)
        rows[s] = [s._advance(20)[0]]
    postprocess([a])
    assert a._post is not None and len(a._post) == S.RESULT_LEN and a._post[0] < 0 and b._post is None
    sa, sb = a.state(), b.state()
    for k in ("u", "v", "p", "mdot"):
        assert np.array_equal(sa[k], sb[k]), k
    for s in (a, b):
        rows[s].append(s._advance(20)[0])
    sa, sb = a.state(), b.state()
    for k in ("u", "v", "p", "mdot"):
        assert np.array_equal(sa[k], sb[k]), k
    assert np.array_equal(np.concatenate(rows[a]), np.concatenate(rows[b])) and np.concatenate(rows[a]).shape == (40, 8)
    assert a.counters() == b.counters() and a.counters()["iterations"] == 40
    a.close()
    b.close()


def test_one_postprocess_call_over_three_routes(fv):
    """A stretched wall trial, a uniform wall trial and a uniform vortex_metrics="device" trial in ONE call: each gets the
    block of a call of its own."""
    FVSolver, _ = fv
    from solvers.fv.solver import postprocess
    uniform = dict(YAML, Re=100.0, nx=16, ny=16, max_iterations=300, tolerance=1e-30, check_every=64)
    kws = [dict(_wall(), nx=13, ny=17), dict(uniform, streamfunction="wall", vortex_refine="quadratic"),
           dict(uniform, nx=8, ny=8, vortex_metrics="device")]
    trials = [FVSolver(**kw) for kw in kws]
    for s in trials:
        s._begin(1e-30)
        s._advance(60)
    lone = []
    for s in trials:
        postprocess([s])
        lone.append((s._post.copy(), s.t["psi"].cpu().numpy(), s.t["omega"].cpu().numpy()))
        s._post = None
    assert [len(r) for r, _, _ in lone] == [S.RESULT_LEN, S.RESULT_LEN, 16]
    postprocess(trials)
    for s, (row, psi, om) in zip(trials, lone):
        assert len(s._post) == S.RESULT_LEN and np.array_equal(s._post[:len(row)], row)
        assert np.array_equal(s.t["psi"].cpu().numpy(), psi) and np.array_equal(s.t["omega"].cpu().numpy(), om)
    assert trials[0]._post[0] < 0 and not np.array_equal(lone[0][0], lone[1][0])
    for s in trials:
        s.close()


def _solve_metrics(s):
    m = s.metrics.as_dict()
    m.pop("wall_time_seconds")
    return m


def test_a_cu_batch_with_a_stretched_wall_trial(fv):
    FVSolver, BatchedFVSolver = fv
    trials = [dict(_wall(**MODES["consistent_cu"]), nx=13, ny=17), dict(_wall(), corner_treatment="saad"),
              dict(YAML, Re=100.0, nx=8, ny=8, max_iterations=300, tolerance=1e-30, check_every=64, vortex_metrics="device"),
              dict(YAML, Re=100.0, nx=16, ny=16, max_iterations=300, tolerance=1e-30, check_every=64, grid="tanh")]
    batch = BatchedFVSolver(trials)
    batch.solve()
    assert batch.errors == {}
    for q, (b, t) in enumerate(zip(batch.solvers, trials)):
        lone = FVSolver(**t)
        lone.solve()
        sb, sl = b.state(), lone.state()
        for k in ("u", "v", "p", "mdot"):
            assert np.array_equal(sb[k], sl[k]), (q, k)
        assert _solve_metrics(b) == _solve_metrics(lone), q                 # bit for bit, vortex metrics included
        lone.close()
    for b in batch.solvers[:2]:
        _assert_metrics_are_the_statement(b, _solve_metrics(b))
        assert b.metrics.as_dict()["psi_min"] < 0 and b.vortex_refine_status[0] == 0
    assert batch.solvers[3].vortex_refine_status is None                    # the host ring rule, as before
    batch.close()


def test_the_launcher_takes_a_stretched_wall_trial(tmp_path):
    r = subprocess.run([sys.executable, str(PKG / "main.py"), "solver=fv", "N=16", "Re=100", "max_iterations=300",
                        "+solver.grid=tanh", "+solver.grid_stretch=1.5", "+solver.streamfunction=wall_stretched",
                        "+solver.vortex_refine=quadratic"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = json.loads(next(tmp_path.rglob("results.json")).read_text())
    assert rec["params"]["grid"] == "tanh" and rec["params"]["streamfunction"] == "wall_stretched"
    m = rec["metrics"]
    print({k: m.get(k) for k in ("psi_min", "psi_min_x", "psi_min_y", "psi_BR", "omega_BR")})
    assert m["psi_min"] < 0 and m["omega_center"] != 0.0
    assert m["psi_min_x"] not in S.axis(16, 1.0, 1.5)[0]                       # a sub-cell centre
