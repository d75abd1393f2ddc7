"""Wall-clustered (tanh) grids on the chip mapping (grid="tanh", mapping="chip", chip_grid="tables"; ldc_fv_wide_set_grid,
csrc/ldc_fv_wide_stretched.inc) on the GPU: TVD trajectories of both pressure equations against the NumPy restatement
(tests/fv_stretched_numpy.py) at the smallest shapes that reach each path, against the one-CU stretched kernel, grid_stretch = 0
against the uniform chip kernel, bit equality across repeats, chunks, graph replay and budgets, a solve to the latch, the
post-processing above 256 cells, the launcher, and the calls that refuse a handle with tables."""
import ctypes as C
import functools
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"
sys.path.insert(0, str(Path(__file__).resolve().parent))
from fv_stretched_numpy import FVStretchedState, centreline_extrema  # noqa: E402

from conftest import PKG  # noqa: E402

pytestmark = pytest.mark.gpu

FIELDS = ("u", "v", "p", "mdot")
MODES = ("consistent", "reference")
CU_MODE = {"consistent": "consistent_cu", "reference": "reference"}     # the one-CU trial of the same equation
CHIP = dict(grid="tanh", mapping="chip", chip_grid="tables")
# TVD, Re 100, 0.4 / 0.2, both solves to 1e-12: the settings of tests/test_gpu_fv_stretched.py
BASE = dict(name="fv", Re=100.0, convection_scheme="TVD", alpha_uv=0.4, alpha_p=0.2, linear_solver_tol=1e-12,
            pressure_tol=1e-12, tolerance=1e-30, check_every=8)


@pytest.fixture(scope="module")
def fv():
    import __graft_entry__ as g
    g.build()
    from solvers.fv.solver import FVSolver
    return FVSolver


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def _rows_rel(got, ref):
    den = np.where(ref == 0.0, 1.0, np.abs(ref))
    return float(np.max(np.abs(got - ref) / den))


def _cols(mode):
    """|div mdot| (column 3) of the consistent equation is zero to the CG tolerance in both runs and has no digits to compare:
    it is held against the size of the fluxes instead (the rule of tests/test_gpu_fv_stretched.py)."""
    return [0, 1, 2, 4, 5, 6] if mode.startswith("consistent") else list(range(7))


def _compare(tag, got_state, got_rows, ref_state, ref_rows, mode, tol=1e-9):
    devs = {k: _rel(got_state[k], ref_state[k]) for k in FIELDS}
    cols = _cols(mode)
    rows = _rows_rel(got_rows[:, cols], ref_rows[:, cols])
    div = float(np.max(np.abs(got_rows[:, 3] - ref_rows[:, 3])))
    flux = float(np.max(np.abs(ref_state["mdot"])))
    print(f"{tag} {mode}: records {rows:.2e}, div {div:.2e} (fluxes {flux:.2e}), fields {devs}")
    assert got_rows.shape == ref_rows.shape
    assert rows <= tol, tag
    assert div <= tol * flux, tag
    for k, d in devs.items():
        assert d <= tol, (tag, k)


def _walls_are_zero(mdot, nx, ny):
    fx, fy = mdot[: ny * (nx + 1)].reshape(ny, nx + 1), mdot[ny * (nx + 1):].reshape(ny + 1, nx)
    return not fx[:, 0].any() and not fx[:, -1].any() and not fy[0].any() and not fy[-1].any()


@functools.lru_cache(maxsize=None)
def _restatement(nx, ny, beta, mode, K, solver):
    """K iterations of the restatement from rest: computed once per case, shared, left unchanged."""
    o = FVStretchedState(nx, ny, 100.0, linear_solver_tol=1e-12, convection_scheme="TVD", grid_stretch=beta,
                         pressure_equation=mode, pressure_solver=solver, pressure_tol=1e-12)
    rec = o.run(K)
    state = dict(u=o.u.ravel().copy(), v=o.v.ravel().copy(), p=o.p.ravel().copy(),
                 mdot=np.concatenate([o.fx.ravel(), o.fy.ravel()]))
    for a in (rec, *state.values()):
        a.setflags(write=False)
    return state, rec


def _solve(FVSolver, K, **kw):
    s = FVSolver(**dict(BASE, max_iterations=K, **kw))
    s.solve()
    out = (s.state(), s.history.copy(), s.counters())
    s.close()
    return out


# ------------------------------------------------------------------------------------------- 1, 2. the restatement
# 13 x 17: one work-group, odd sizes; 40 x 24: 4 work-groups, GEMM tiles with ragged edges; 264 x 8 and 8 x 264: an axis beyond
# the one-CU range; 264 x 250: 66 000 cells, the work-group count capped at 256 and a second pass of the grid-stride loop
# (the dense pressure matrix of the restatement's "direct" solve does not fit there: its CG stands in)
CASES = [(13, 17, 1.0, 30, "direct"), (40, 24, 1.5, 30, "direct"), (264, 8, 1.5, 12, "direct"), (8, 264, 1.5, 12, "direct"),
         (264, 250, 1.5, 3, "cg")]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nx,ny,beta,K,solver", CASES, ids=lambda v: str(v))
def test_tvd_trajectories_match_the_restatement(fv, nx, ny, beta, K, solver, mode):
    """u, v, p, mdot and every record column (E, Z, P by the Gauss rule) to 1e-9 from rest; in consistent mode |div mdot| is
    held against 1e-9 max|mdot| and the wall faces are exactly 0.0."""
    from solvers.fv import ldc_fv_lib as F
    st, rows, c = _solve(fv, K, nx=nx, ny=ny, grid_stretch=beta, pressure_equation=mode, **CHIP)
    print(c)
    assert F.wide_groups(nx, ny) == {221: 1, 960: 4, 2112: 9, 66000: 256}[nx * ny]
    ref_state, ref_rows = _restatement(nx, ny, beta, mode, K, solver)
    _compare(f"{nx}x{ny} beta {beta}", st, rows, ref_state, ref_rows, mode)
    assert c["iterations"] == K and c["nan"] == 0 and c["linear_giveups"] == 0
    if mode == "consistent":
        assert c["pressure_caps"] == 0 and c["pressure_solves"] == K
        assert _walls_are_zero(st["mdot"], nx, ny)


# ------------------------------------------------------------------------------------------- 3. the one-CU stretched kernel
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nx,ny,K", [(96, 80, 20), (256, 256, 4)], ids=lambda v: str(v))
def test_the_chip_chain_follows_the_one_cu_kernel(fv, nx, ny, K, mode):
    """The same trial on mapping="cu" (consistent_cu for consistent) and on the chip chain, beta 1.5: fields and records to
    1e-9.  256 x 256 is the largest size both take, and 256 work-groups."""
    kw = dict(nx=nx, ny=ny, grid_stretch=1.5)
    got = _solve(fv, K, pressure_equation=mode, **kw, **CHIP)
    ref = _solve(fv, K, pressure_equation=CU_MODE[mode], grid="tanh", **kw)
    _compare(f"{nx}x{ny} chip / cu", got[0], got[1], ref[0], ref[1], mode)
    for k in ("iterations", "nan", "linear_giveups", "linear_iterations", "momentum_solves"):
        assert got[2][k] == ref[2][k], k
    if mode == "consistent":
        assert got[2]["pressure_caps"] == ref[2]["pressure_caps"] == 0
        assert abs(got[2]["pressure_iterations"] - ref[2]["pressure_iterations"]) <= K       # (a stop test at rounding)


# ------------------------------------------------------------------------------------------- 4. beta = 0: the uniform chain
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nx,ny", [(13, 17), (264, 250)])
def test_zero_stretch_follows_the_uniform_chip_kernel(fv, nx, ny, mode):
    """grid_stretch = 0 (uniform vertices through the stretched twins) against the uniform chip chain of the same mode, 6 TVD
    iterations: fields and every record column to 1e-9 (the constant lid: the Gauss rule is the ghost-cell rule)."""
    kw = dict(nx=nx, ny=ny, pressure_equation=mode)
    got = _solve(fv, 6, grid_stretch=0.0, **kw, **CHIP)
    ref = _solve(fv, 6, mapping="chip", **kw)
    _compare(f"{nx}x{ny} beta 0 / uniform", got[0], got[1], ref[0], ref[1], mode)


# ------------------------------------------------------------------------------------------- 5. bit equality
def _run(s, chunks=(24,)):
    z = np.zeros(s.n_cells)
    s.set_state(z, z, z, np.zeros(s.t["mdot"].numel()))
    s._begin(1e-30)
    rows = np.concatenate([s._advance(k)[0] for k in chunks], axis=0)
    return rows, s.state(), s.counters()


def _same_bits(a, b, counters=("iterations", "nan", "linear_giveups", "linear_iterations", "momentum_solves",
                               "pressure_iterations", "pressure_solves", "pressure_caps", "pressure_last")):
    assert np.array_equal(a[0], b[0])
    for k in FIELDS:
        assert np.array_equal(a[1][k], b[1][k]), k
    for k in counters:
        assert a[2][k] == b[2][k], k


def test_repeats_chunks_graphs_and_budgets_change_no_bit(fv):
    """40 x 24, consistent mode, 24 iterations from rest.  Two solves on one handle and a third in chunks (7, 1, 16); graph
    replay against kernel-by-kernel launches; a pressure budget and a linear budget of 2, whose retry protocol repeats
    iterations until the budgets fit, against the defaults: the same bits every time."""
    kw = dict(BASE, nx=40, ny=24, grid_stretch=1.5, pressure_equation="consistent", check_every=32, linear_solver_tol=1e-9,
              **CHIP)
    s = fv(**kw)
    first = _run(s)
    assert first[2]["iterations"] == 24 and first[2]["nan"] == 0 and first[2]["pressure_solves"] == 24
    _same_bits(first, _run(s))
    _same_bits(first, _run(s, (7, 1, 16)))
    for on in (False, True):
        s.set_wide_graph(on)
        _same_bits(first, _run(s))
        _same_bits(first, _run(s, (7, 1, 16)))
    s.close()
    t = fv(**dict(kw, pressure_budget=2, linear_budget=2))
    small = _run(t)
    _same_bits(first, small)
    assert small[2]["pressure_budget_retries"] > 0 and small[2]["linear_budget_retries"] > 0
    t.close()


# ------------------------------------------------------------------------------------------- 6. a solve to the latch
def test_convergence_at_32_re1000(fv):
    """32 x 32, Re 1000, beta 1.5, TVD, consistent, 0.7 / 0.3, pressure_tol 1e-8, tolerance 1e-7: the restatement stops after
    1704 iterations, 4.6e-4 and 7.7e-4 relative away from the tolerance on either side (the fixture), so rounding cannot move
    the count.  No pressure cap, no give-up, no NaN; the centreline extrema to 1e-6; and the wall-stretched metrics with the
    quadratic refinement equal those of a one-CU trial on the same converged state (that kernel reads raw pointers only)."""
    want = json.loads((GOLD / "g17_fv_stretched_converged.json").read_text())
    assert want["iterations"] == 1704 and min(want["margins"].values()) >= 1e-4
    kw = dict(name="fv", Re=1000.0, nx=32, ny=32, convection_scheme="TVD", alpha_uv=0.7, alpha_p=0.3, linear_solver_tol=1e-9,
              pressure_tol=1e-8, pressure_max_iters=200, tolerance=1e-7, max_iterations=5000, check_every=512,
              grid_stretch=1.5, streamfunction="wall_stretched", vortex_refine="quadratic")
    s = fv(**kw, pressure_equation="consistent", pressure_budget=64, **CHIP)
    s.solve()
    c = s.counters()
    ny, nx = s.shape_full
    xs, ys = s.fields.x.reshape(ny, nx)[0], s.fields.y.reshape(ny, nx)[:, 0]
    ext = centreline_extrema(s.fields.u.reshape(ny, nx), s.fields.v.reshape(ny, nx), xs, ys)
    print("iterations", int(s.metrics.iterations), ext, c)
    assert s.metrics.converged and c["pressure_caps"] == 0 and c["linear_giveups"] == 0 and c["nan"] == 0
    assert int(s.metrics.iterations) == want["iterations"]
    for k in ext:
        assert abs(ext[k] - want["extrema"][k]) <= 1e-6, k
    assert c["pressure_iterations"] / c["pressure_solves"] == pytest.approx(want["cg_iterations_mean"], abs=1.0)
    got = s.compute_vortex_metrics()
    st = s.state()
    one = fv(**kw, pressure_equation="consistent_cu", grid="tanh")
    one.set_state(st["u"], st["v"], st["p"], st["mdot"])
    ref = one.compute_vortex_metrics()
    assert set(got) == set(ref) and got["psi_min"] < -0.09
    for k in ref:
        assert abs(got[k] - ref[k]) <= 1e-9 * max(1.0, abs(ref[k])), k
    assert s.vortex_refine_status == one.vortex_refine_status
    one.close()
    s.close()


# ------------------------------------------------------------------------------------------- 7. post-processing above 256
def test_the_wall_rule_takes_a_trial_without_a_one_cu_handle(fv):
    s = fv(**dict(BASE, max_iterations=12, nx=264, ny=8, grid_stretch=1.5, streamfunction="wall_stretched", **CHIP))
    s.solve()
    assert s.handle is None and s._wide is not None
    m = s.compute_vortex_metrics()
    assert m and all(np.isfinite(v) for v in m.values()) and m["psi_min"] < 0
    psi = s.streamfunction()
    assert psi.shape == (8, 264) and np.all(np.isfinite(psi)) and s.vorticity().shape == (8, 264)
    r = fv(**dict(BASE, max_iterations=12, nx=264, ny=8, grid_stretch=1.5, streamfunction="wall_stretched",
                  vortex_refine="quadratic", pressure_equation="consistent", **CHIP))
    r.solve()
    assert all(np.isfinite(v) for v in r.compute_vortex_metrics().values()) and len(r.vortex_refine_status) == 4
    r.close()
    s.close()


# ------------------------------------------------------------------------------------------- 8. the launcher
def test_main_runs_a_stretched_chip_trial(tmp_path):
    r = subprocess.run([sys.executable, str(PKG / "main.py"), "solver=fv", "N=16", "+solver.mapping=chip", "+solver.grid=tanh",
                        "+solver.chip_grid=tables"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    res = list(tmp_path.rglob("results.json"))
    assert res, r.stderr[-3000:]
    rec = json.loads(res[0].read_text())
    assert rec["solver"] == "fv" and rec["metrics"]["converged"] == 1 and rec["metrics"]["psi_min"] < 0


# ------------------------------------------------------------------------------------------- 9. an uncaught route
def test_the_library_refuses_a_handle_with_tables_where_equal_spacing_is_assumed(fv):
    """Past the solver's own checks: the handle of a stretched chip trial given to ldc_fv_wide_batch_create and to
    ldc_fv_wide_post_enqueue is LDC_E_ARG, before any launch -- the state, the record and the control words stay as they are."""
    import torch
    from solvers.fv import ldc_fv_lib as F
    from solvers.fv.solver import sine_eig
    s = fv(**dict(BASE, max_iterations=4, nx=40, ny=24, grid_stretch=1.5, **CHIP))
    s.solve()
    before = {k: s.t[k].clone() for k in ("u", "v", "p", "mdot", "rec", "ctrl", "work")}
    L, dev = F.lib(), s.device
    table = torch.zeros(F.wide_batch_table_len([(40, 24)]), dtype=torch.uint8, device=dev)
    b = C.c_void_p()
    hs = (C.c_void_p * 1)(s._wide)
    assert L.ldc_fv_wide_batch_create(hs, 1, C.c_void_p(table.data_ptr()), table.numel(), C.byref(b)) == -1 and not b.value
    lamx, Sx = sine_eig(40 - 2, dev)
    lamy, Sy = sine_eig(24 - 2, dev)
    out = {k: torch.zeros(n, dtype=torch.float64, device=dev) for k, n in (("psi", 960), ("omega", 960), ("result", 16),
                                                                           ("scratch", F.wide_post_scratch_len(40, 24)))}
    post = F.Post(Sx=Sx.data_ptr(), lamx=lamx.data_ptr(), Sy=Sy.data_ptr(), lamy=lamy.data_ptr(), ix_lt=0, ix_gt=0, jy_lt=0,
                  jy_gt=0, psi=out["psi"].data_ptr(), omega=out["omega"].data_ptr(), result=out["result"].data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    assert L.ldc_fv_wide_post_enqueue(s._wide, C.byref(post), C.c_void_p(out["scratch"].data_ptr()), out["scratch"].numel(),
                                      stream) == -1
    assert L.ldc_fv_wide_prolong_enqueue(s._wide, s._wide, stream) == -1
    torch.cuda.synchronize()
    assert not any(t.any().item() for t in out.values()) and not table.any().item()
    for k, t in before.items():
        assert torch.equal(s.t[k], t), k
    s.close()
