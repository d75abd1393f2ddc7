"""The separable scaled preconditioner on the chip mapping (chip_preconditioner="separable"; ldc_fv_wide_set_preconditioner,
csrc/ldc_fv_wide_separable.inc) on the GPU: TVD trajectories against the NumPy restatement (tests/fv_separable_numpy.py) at the
shapes of tests/test_gpu_fv_wide_stretched.py, against the one-CU separable kernel, against the laplacian chain above the
restatement's range, bit equality across repeats, chunks, graph replay, budgets and detaching, a solve to the latch with both
preconditioners, and the launcher."""
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
from fv_separable_numpy import FVSeparableState  # noqa: E402
from fv_stretched_numpy import centreline_extrema  # noqa: E402

from conftest import PKG  # noqa: E402

pytestmark = pytest.mark.gpu

FIELDS = ("u", "v", "p", "mdot")
MODE = "consistent"
CHIP = dict(grid="tanh", mapping="chip", chip_grid="tables", pressure_equation=MODE)
SEP = dict(CHIP, chip_preconditioner="separable")
LAP = dict(CHIP, chip_preconditioner="laplacian")
# TVD, Re 100, 0.4 / 0.2, both solves to 1e-12: the settings of tests/test_gpu_fv_wide_stretched.py
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


def _compare(tag, got_state, got_rows, ref_state, ref_rows, tol=1e-9):
    """The rule of tests/test_gpu_fv_wide_stretched.py for the consistent equation: u, v, p, mdot and the record columns to
    `tol`; |div mdot| (column 3), zero to the CG tolerance in both runs, against tol max|mdot|."""
    devs = {k: _rel(got_state[k], ref_state[k]) for k in FIELDS}
    cols = [0, 1, 2, 4, 5, 6]
    rows = _rows_rel(got_rows[:, cols], ref_rows[:, cols])
    div = float(np.max(np.abs(got_rows[:, 3] - ref_rows[:, 3])))
    flux = float(np.max(np.abs(ref_state["mdot"])))
    print(f"{tag}: records {rows:.2e}, div {div:.2e} (fluxes {flux:.2e}), fields {devs}")
    assert got_rows.shape == ref_rows.shape
    assert rows <= tol, tag
    assert div <= tol * flux, tag
    for k, d in devs.items():
        assert d <= tol, (tag, k)


def _walls_are_zero(mdot, nx, ny):
    fx, fy = mdot[: ny * (nx + 1)].reshape(ny, nx + 1), mdot[ny * (nx + 1):].reshape(ny + 1, nx)
    return not fx[:, 0].any() and not fx[:, -1].any() and not fy[0].any() and not fy[-1].any()


@functools.lru_cache(maxsize=None)
def _restatement(nx, ny, beta, K):
    """K iterations of the restatement from rest: computed once per case, shared, left unchanged."""
    o = FVSeparableState(nx, ny, 100.0, linear_solver_tol=1e-12, convection_scheme="TVD", grid_stretch=beta,
                         pressure_solver="cg", pressure_tol=1e-12)
    rec = o.run(K)
    state = dict(u=o.u.ravel().copy(), v=o.v.ravel().copy(), p=o.p.ravel().copy(),
                 mdot=np.concatenate([o.fx.ravel(), o.fy.ravel()]))
    for a in (rec, *state.values()):
        a.setflags(write=False)
    assert o.cg_caps == 0
    return state, rec, tuple(o.cg_iters)


def _solve(FVSolver, K, **kw):
    s = FVSolver(**dict(BASE, max_iterations=K, **kw))
    s.solve()
    out = (s.state(), s.history.copy(), s.counters())
    s.close()
    return out


# ------------------------------------------------------------------------------------------- 1. the restatement
# 13 x 17: one work-group, odd sizes; 40 x 24: 4 work-groups, GEMM tiles with ragged edges; 264 x 8 and 8 x 264: an axis beyond
# the one-CU range; 264 x 250: 256 work-groups and a second pass of the grid-stride loop.  CG per solve of the restatement:
# 10 ... 13, 14 ... 17, 5 ... 6, 5, 16 ... 17
CASES = [(13, 17, 1.0, 30, (10, 13)), (40, 24, 1.5, 30, (14, 17)), (264, 8, 1.5, 12, (5, 6)), (8, 264, 1.5, 12, (5, 5)),
         (264, 250, 1.5, 3, (16, 17))]


@pytest.mark.parametrize("nx,ny,beta,K,cg", CASES, ids=lambda v: str(v))
def test_tvd_trajectories_match_the_restatement(fv, nx, ny, beta, K, cg):
    """u, v, p, mdot and every record column to 1e-9 from rest, |div mdot| against 1e-9 max|mdot|, wall faces exactly 0.0; the
    card's CG count within one per solve of the restatement's (a stop test at rounding), no cap."""
    from solvers.fv import ldc_fv_lib as F
    st, rows, c = _solve(fv, K, nx=nx, ny=ny, grid_stretch=beta, **SEP)
    print(c)
    assert F.wide_groups(nx, ny) == {221: 1, 960: 4, 2112: 9, 66000: 256}[nx * ny]
    ref_state, ref_rows, ref_cg = _restatement(nx, ny, beta, K)
    print("CG per solve of the restatement:", ref_cg)
    assert (min(ref_cg), max(ref_cg)) == cg and len(ref_cg) == K
    _compare(f"{nx}x{ny} beta {beta}", st, rows, ref_state, ref_rows)
    assert c["iterations"] == K and c["nan"] == 0 and c["linear_giveups"] == 0
    assert c["pressure_caps"] == 0 and c["pressure_solves"] == K
    assert abs(c["pressure_iterations"] - sum(ref_cg)) <= K and abs(c["pressure_last"] - ref_cg[-1]) <= 1
    assert _walls_are_zero(st["mdot"], nx, ny)


# ------------------------------------------------------------------------------------------- 2. the one-CU separable kernel
@pytest.mark.parametrize("nx,ny,K", [(96, 80, 20), (256, 256, 4)], ids=lambda v: str(v))
def test_the_chip_chain_follows_the_one_cu_kernel(fv, nx, ny, K):
    """The same trial on mapping="cu" (consistent_cu, pressure_preconditioner="separable") and on the chip chain, beta 1.5: fields
    and records to 1e-9, equal linear counters, CG totals within K.  256 x 256 is the largest size both take."""
    kw = dict(nx=nx, ny=ny, grid_stretch=1.5)
    got = _solve(fv, K, **kw, **SEP)
    ref = _solve(fv, K, grid="tanh", pressure_equation="consistent_cu", pressure_preconditioner="separable", **kw)
    print(got[2], ref[2])
    _compare(f"{nx}x{ny} chip / cu", got[0], got[1], ref[0], ref[1])
    for k in ("iterations", "nan", "linear_giveups", "linear_iterations", "momentum_solves"):
        assert got[2][k] == ref[2][k], k
    assert got[2]["pressure_caps"] == ref[2]["pressure_caps"] == 0
    assert abs(got[2]["pressure_iterations"] - ref[2]["pressure_iterations"]) <= K       # (a stop test at rounding)


# ------------------------------------------------------------------------------------------- 3. above the helper's range
@pytest.mark.parametrize("nx,ny", [(1024, 8), (8, 1024)])
def test_separable_follows_laplacian_at_1024_cells(fv, nx, ny):
    """beta 1.5, 6 iterations from rest, both preconditioners on the card: both solve the same equation to 1e-12 (the
    restatement pair of these meshes agrees to 1e-14), so fields and records agree to 1e-9; the restatement takes 4 CG
    iterations per solve against 85 ... 87, the card at most half."""
    kw = dict(nx=nx, ny=ny, grid_stretch=1.5)
    sep = _solve(fv, 6, **kw, **SEP)
    lap = _solve(fv, 6, **kw, **LAP)
    print(sep[2], lap[2])
    _compare(f"{nx}x{ny} separable / laplacian", sep[0], sep[1], lap[0], lap[1])
    for c in (sep[2], lap[2]):
        assert c["iterations"] == 6 and c["nan"] == 0 and c["linear_giveups"] == 0
        assert c["pressure_caps"] == 0 and c["pressure_solves"] == 6
    assert sep[2]["pressure_iterations"] <= 0.5 * lap[2]["pressure_iterations"]
    assert _walls_are_zero(sep[0]["mdot"], nx, ny)


# ------------------------------------------------------------------------------------------- 4. bit equality
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


def test_repeats_chunks_graphs_budgets_and_detaching_change_no_bit(fv):
    """40 x 24, 24 iterations from rest.  Two solves on one handle and a third in chunks (7, 1, 16); graph replay against
    kernel-by-kernel launches; a pressure budget and a linear budget of 2, whose retry protocol repeats iterations until the
    budgets fit, against the defaults: the same bits every time.  The handle with its tables detached gives the bits of a
    fresh laplacian trial, and with them attached again those of the fresh separable one."""
    from solvers.fv import ldc_fv_lib as F
    kw = dict(BASE, nx=40, ny=24, grid_stretch=1.5, check_every=32, linear_solver_tol=1e-9)
    s = fv(**kw, **SEP)
    first = _run(s)
    assert first[2]["iterations"] == 24 and first[2]["nan"] == 0 and first[2]["pressure_solves"] == 24
    _same_bits(first, _run(s))
    _same_bits(first, _run(s, (7, 1, 16)))
    for on in (False, True):
        s.set_wide_graph(on)
        _same_bits(first, _run(s))
        _same_bits(first, _run(s, (7, 1, 16)))
    t = fv(**dict(kw, pressure_budget=2, linear_budget=2), **SEP)
    small = _run(t)
    _same_bits(first, small)
    assert small[2]["pressure_budget_retries"] > 0 and small[2]["linear_budget_retries"] > 0
    t.close()
    lap = fv(**kw, **LAP)
    plain = _run(lap)
    lap.close()
    assert plain[2]["pressure_iterations"] > 2 * first[2]["pressure_iterations"]
    assert not np.array_equal(plain[1]["p"], first[1]["p"])                  # (they differ at the level of pressure_tol)
    F.check(F.lib().ldc_fv_wide_set_preconditioner(s._wide, None), "ldc_fv_wide_set_preconditioner")
    _same_bits(plain, _run(s))
    F.wide_set_preconditioner(s._wide, s.t["precx"].data_ptr(), s.t["precx"].numel(), s.t["precy"].data_ptr(),
                              s.t["precy"].numel())
    _same_bits(first, _run(s))
    s.close()


# ------------------------------------------------------------------------------------------- 5. a solve to the latch
def test_both_chip_preconditioners_stop_at_the_restatements_count(fv):
    """32 x 32, Re 1000, beta 1.5, TVD, consistent, 0.7 / 0.3, pressure_tol 1e-8, tolerance 1e-7
    (tests/golden/g17_fv_stretched_converged.json: the restatement stops after 1704 iterations, 4.6e-4 and 7.7e-4 relative
    away from the tolerance), with both preconditioners on the chip chain.  Both stop at that count with no cap, give-up or NaN
    and the fixture's extrema to 1e-6.  The field bound is that of
    tests/test_gpu_fv_separable.py::test_both_preconditioners_stop_at_the_restatements_count: the two RESTATEMENT runs differ at
    their stops by 6.37e-11 at most over u, v and p, with 43.2 and 17.0 CG iterations per solve; ten times it is allowed
    between the card's two runs."""
    want = json.loads((GOLD / "g17_fv_stretched_converged.json").read_text())
    assert want["iterations"] == 1704 and min(want["margins"].values()) >= 1e-4
    measured = 6.37e-11
    kw = dict(name="fv", Re=1000.0, nx=32, ny=32, convection_scheme="TVD", alpha_uv=0.7, alpha_p=0.3, linear_solver_tol=1e-9,
              grid_stretch=1.5, pressure_tol=1e-8, pressure_max_iters=200, tolerance=1e-7, max_iterations=5000, check_every=512)
    out = {}
    for name, mode, budget in (("laplacian", LAP, 64), ("separable", SEP, 32)):
        s = fv(**kw, pressure_budget=budget, **mode)
        s.solve()
        c = s.counters()
        ny, nx = s.shape_full
        xs, ys = s.fields.x.reshape(ny, nx)[0], s.fields.y.reshape(ny, nx)[:, 0]
        ext = centreline_extrema(s.fields.u.reshape(ny, nx), s.fields.v.reshape(ny, nx), xs, ys)
        print(name, int(s.metrics.iterations), ext, c)
        assert s.metrics.converged and c["pressure_caps"] == 0 and c["linear_giveups"] == 0 and c["nan"] == 0
        assert int(s.metrics.iterations) == want["iterations"]
        for k in ext:
            assert abs(ext[k] - want["extrema"][k]) <= 1e-6, k
        out[name] = (s.state(), c["pressure_iterations"] / c["pressure_solves"])
        s.close()
    diffs = {k: float(np.max(np.abs(out["separable"][0][k] - out["laplacian"][0][k]))) for k in ("u", "v", "p")}
    print(f"card, separable against laplacian at the stop: {diffs}; CG per solve {out['laplacian'][1]:.2f} and "
          f"{out['separable'][1]:.2f}")
    assert out["laplacian"][1] == pytest.approx(want["cg_iterations_mean"], abs=1.0)
    assert want["cg_iterations_mean"] == pytest.approx(43.16, abs=0.01)
    assert out["separable"][1] <= 0.5 * out["laplacian"][1]
    assert out["separable"][1] == pytest.approx(17.0, abs=1.0)
    assert max(diffs.values()) <= 10 * measured


# ------------------------------------------------------------------------------------------- 6. the launcher
def test_main_runs_a_separable_chip_trial(tmp_path):
    r = subprocess.run([sys.executable, str(PKG / "main.py"), "solver=fv", "N=16", "+solver.mapping=chip", "+solver.grid=tanh",
                        "+solver.chip_grid=tables", "+solver.pressure_equation=consistent",
                        "+solver.chip_preconditioner=separable"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    res = list(tmp_path.rglob("results.json"))
    assert res, r.stderr[-3000:]
    rec = json.loads(res[0].read_text())
    assert rec["solver"] == "fv" and rec["metrics"]["converged"] == 1 and rec["metrics"]["psi_min"] < 0
