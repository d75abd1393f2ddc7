"""The consistent pressure equation of chip and shared finite-volume trials (pressure_equation="consistent",
csrc/ldc_fv_wide_pressure.inc) on the GPU: one iteration from a developed state against a dense solve, trajectories against
the NumPy restatement (tests/fv_consistent_numpy.py), mass conservation row by row, solves to the latch, bit equality across
repeats, graphs, budgets, chunkings and batches of both modes, the accepted cap hit, and the launcher."""
import ctypes as C
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"
sys.path.insert(0, str(Path(__file__).resolve().parent))
from fv_consistent_numpy import FVConsistentState  # noqa: E402

from conftest import PKG  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
C_RHS, Y = 23, 26                       # work vectors: rhs_p (entry 0 = 0) and x of the pressure solve (FvVec)
YAML = dict(name="fv", convection_scheme="TVD", alpha_uv=0.4, alpha_p=0.2, linear_solver_tol=1e-9)      # conf/solver/fv.yaml
CONSISTENT = dict(mapping="chip", pressure_equation="consistent")
COUNTERS = ("done", "iterations", "nan", "linear_giveups", "linear_iterations", "momentum_solves", "anderson_fallbacks")
PCOUNTERS = ("pressure_iterations", "pressure_solves", "pressure_caps", "pressure_last")


@pytest.fixture(scope="module")
def fv():
    import __graft_entry__ as g
    g.build()
    from solvers.fv.batched import BatchedFVSolver
    from solvers.fv.solver import FVSolver
    return FVSolver, BatchedFVSolver


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def _rows_rel(got, ref):
    den = np.where(ref == 0.0, 1.0, np.abs(ref))
    return float(np.max(np.abs(got - ref) / den))


def _oracle(nx, ny, Re, scheme="TVD", **kw):
    return FVConsistentState(nx, ny, Re, linear_solver_tol=1e-9, convection_scheme=scheme, pressure_solver="direct", **kw)


def _mdot(o):
    return np.concatenate([o.fx.ravel(), o.fy.ravel()])


# ------------------------------------------------------------------------------------------- one iteration
def _own_cg_count(o, lin_tol):
    """The CG iterations the restatement itself takes (pressure_tol 1e-13) for the iteration that follows ``o``'s state."""
    r = FVConsistentState(o.nx, o.ny, 100.0, linear_solver_tol=lin_tol, convection_scheme="TVD", pressure_solver="cg",
                          pressure_tol=1e-13)
    r.set_state(o.u.ravel(), o.v.ravel(), o.p.ravel(), _mdot(o))
    r.step()
    assert r.cg_caps == 0
    return r.cg_iters[-1]


@pytest.mark.parametrize("nx,ny", [(8, 8), (16, 16), (24, 16), (33, 19), (37, 50)])
def test_one_iteration_from_a_developed_state(fv, nx, ny):
    """20 iterations of the restatement, then ONE on the device with pressure_tol 1e-13.  The CG iterate x, read from its
    work vector, against the dense solve x* of the same system: A (x - x*) = -r with |r| <= pressure_tol |b|, and both lie
    (after their means are taken off) in the range of the symmetric positive semi-definite A, so
    |x - x*|_2 <= pressure_tol |b|_2 / lambda_min+(A), to which the rounding of x itself adds 64 eps |x|_2.  A, b and
    lambda_min+ are the test's own, from the restatement's weights.  Then u, v, p and mdot at the tolerance of the TVD
    trajectory test.  The CG count is the restatement's own for this system within max(1, 10 x its sensitivity), the
    sensitivity being how far that count moves when linear_solver_tol goes from 1e-9 to 1e-10 (tests/fv_krylov_probe.py)."""
    FVSolver, _ = fv
    tol = 1e-13
    o = _oracle(nx, ny, 100.0)
    o.run(20)
    want = _own_cg_count(o, 1e-9)
    count_bound = max(1, 10 * abs(_own_cg_count(o, 1e-10) - want))
    s = FVSolver(**dict(YAML, **CONSISTENT, nx=nx, ny=ny, Re=100.0, pressure_tol=tol, tolerance=1e-30, max_iterations=10**6,
                        check_every=8))
    s.set_state(o.u.ravel(), o.v.ravel(), o.p.ravel(), _mdot(o))
    rows, done, total = s._advance(1)
    assert total == 1 and rows.shape == (1, 8) and np.all(np.isfinite(rows))
    o.step()
    n = nx * ny
    w = s.t["work"].cpu().numpy()
    x = w[Y * n: (Y + 1) * n]
    rhs = w[C_RHS * n: (C_RHS + 1) * n]
    assert rhs[0] == 0.0
    A = o.dense(o.last["wx"], o.last["wy"])
    b, xs = o.last["b"].ravel(), o.last["x"].ravel()
    lam = np.linalg.eigvalsh(A)
    assert abs(lam[0]) <= 1e-12 * lam[-1] and lam[1] > 1e-6 * lam[-1]            # one zero mode: the constants
    xm, xsm = x - x.mean(), xs - xs.mean()
    err, bound = np.linalg.norm(xm - xsm), tol * np.linalg.norm(b) / lam[1] + 64 * EPS * np.linalg.norm(xsm)
    c = s.counters()
    print(f"{nx}x{ny}: CG {c['pressure_last']} iterations (restatement {want}, within {count_bound}), |x - x*| {err:.2e}, "
          f"bound {bound:.2e} "
          f"(|b| {np.linalg.norm(b):.2e}, lambda_min+ {lam[1]:.2e}, |x| {np.linalg.norm(xsm):.2e}), "
          f"rhs_p {_rel(rhs[1:], b[1:]):.1e}")
    assert 1 <= want <= 40 and abs(c["pressure_last"] - want) <= count_bound
    assert c["pressure_caps"] == 0 and c["pressure_solves"] == 1
    assert err <= bound
    st = s.state()
    devs = {k: _rel(st[k], ref) for k, ref in (("u", o.u.ravel()), ("v", o.v.ravel()), ("p", o.p.ravel()),
                                               ("mdot", _mdot(o)))}
    print(devs)
    for k, d in devs.items():
        assert d <= 1e-9, k
    s.close()


# ------------------------------------------------------------------------------------------- trajectories
@pytest.mark.parametrize("nx,ny,scheme", [(16, 16, "TVD"), (24, 16, "TVD"), (16, 16, "Upwind"), (24, 16, "Upwind")])
def test_trajectories_match_the_restatement(fv, nx, ny, scheme):
    """20 iterations from rest; the restatement solves every pressure system directly, the device to 1e-12."""
    FVSolver, _ = fv
    K = 20
    s = FVSolver(**dict(YAML, **CONSISTENT, nx=nx, ny=ny, Re=100.0, convection_scheme=scheme, pressure_tol=1e-12,
                        tolerance=1e-30, max_iterations=K, check_every=8))
    s.solve()
    o = _oracle(nx, ny, 100.0, scheme)
    rec = o.run(K)
    st = s.state()
    devs = {k: _rel(st[k], ref) for k, ref in (("u", o.u.ravel()), ("v", o.v.ravel()), ("p", o.p.ravel()),
                                               ("mdot", _mdot(o)))}
    cols = [0, 1, 2, 4, 5, 6]                # (column 3, |div mdot|, is rounding in both: the next test bounds it)
    print(f"{nx}x{ny} {scheme}: records {_rows_rel(s.history[:, cols], rec[:, cols]):.2e}, fields {devs}, {s.counters()}")
    assert s.history.shape == rec.shape
    assert _rows_rel(s.history[:, cols], rec[:, cols]) <= 1e-9
    for k, d in devs.items():
        assert d <= 1e-9, k
    s.close()


# ------------------------------------------------------------------------------------------- mass conservation
@pytest.mark.parametrize("nx,ny,Re", [(16, 16, 100.0), (33, 19, 400.0)])
def test_the_corrected_fluxes_conserve_mass(fv, nx, ny, Re):
    """div mdot = -(b - A x) cell by cell, so after every iteration |div mdot|_2 <= pressure_tol |b|_2; the bound asked is
    twice that plus 64 eps sum |mdot| for the rounding of the four-term differences.  (The reference equation leaves 1e-2.)"""
    FVSolver, _ = fv
    s = FVSolver(**dict(YAML, **CONSISTENT, nx=nx, ny=ny, Re=Re, tolerance=1e-30, max_iterations=10**6, check_every=4))
    tol, n = float(s.params.pressure_tol), nx * ny
    s._begin(1e-30)
    worst = 0.0
    for k in range(20):
        rows, _, _ = s._advance(1)
        rhs = s.t["work"][C_RHS * n: (C_RHS + 1) * n].cpu().numpy().copy()
        rhs[0] = -np.sum(rhs[1:])
        bound = 2 * tol * np.linalg.norm(rhs) + 64 * EPS * float(np.sum(np.abs(s.state()["mdot"])))
        worst = max(worst, rows[0, 3] / bound)
        assert rows[0, 3] <= bound, (k, rows[0, 3], bound)
    print(f"{nx}x{ny}: |div mdot| at most {worst:.2e} of its bound; {s.counters()}")
    s.close()


# ------------------------------------------------------------------------------------------- solves to the latch
def _golden(tag):
    g = np.load(GOLD / "g16_fv_consistent.npz")
    return int(g[f"{tag}_iterations"]), g[f"{tag}_u"], g[f"{tag}_v"]


@pytest.mark.parametrize("tag,N,Re,auv,ap,want", [("N16_Re100_04_02", 16, 100.0, 0.4, 0.2, 660),
                                                  ("N32_Re1000_07_03", 32, 1000.0, 0.7, 0.3, 958)])
def test_solve_to_the_latch_takes_the_restatements_iterations(fv, tag, N, Re, auv, ap, want):
    FVSolver, _ = fv
    its, u, v = _golden(tag)
    assert its == want                                   # (the recorded restatement is the table of DESIGN.md section 7)
    s = FVSolver(**dict(YAML, **CONSISTENT, nx=N, ny=N, Re=Re, alpha_uv=auv, alpha_p=ap, tolerance=1e-6,
                        max_iterations=3000, check_every=256))
    s.solve()
    got = int(s.metrics.iterations)
    du, dv = np.max(np.abs(s.fields.u - u)), np.max(np.abs(s.fields.v - v))
    bound = (abs(got - want) + 1) * 1e-6 * np.max(np.abs(u))
    print(f"{tag}: {got} iterations (restatement {want}), max|du| {du:.2e} max|dv| {dv:.2e} bound {bound:.2e}; {s.counters()}")
    assert s.metrics.converged and abs(got - want) <= 2
    assert du <= bound and dv <= bound
    s.close()


def test_the_reference_equation_does_not_latch_where_the_consistent_one_does(fv):
    """32 x 32, Re = 1000, 0.7 / 0.3: the consistent equation latches after 958 iterations (above); the reference's is not
    there after 2000 (it stalls or meets a NaN)."""
    FVSolver, _ = fv
    from solvers.spectral.ldc_lib import LdcError
    s = FVSolver(**dict(YAML, mapping="chip", nx=32, ny=32, Re=1000.0, alpha_uv=0.7, alpha_p=0.3, tolerance=1e-6,
                        max_iterations=2000, check_every=256))
    try:
        s.solve()
        latched = bool(s.metrics.converged)
    except LdcError as exc:
        print(exc)
        latched = False
    print(s.counters())
    assert not latched
    s.close()


# ------------------------------------------------------------------------------------------- bit equality
def _run37(FVSolver, chunks, graph=None, **kw):
    s = FVSolver(**dict(YAML, **CONSISTENT, nx=37, ny=50, Re=400.0, tolerance=1e-30, max_iterations=10**6, check_every=64,
                        **kw))
    if graph is not None:
        s.set_wide_graph(graph)
    s._begin(1e-30)
    rows = np.concatenate([s._advance(k)[0] for k in chunks], axis=0)
    out = (rows, s.state(), s.counters())
    s.close()
    return out


def test_runs_repeat_bit_for_bit_whatever_the_graph_the_chunks_and_the_budgets(fv):
    FVSolver, _ = fv
    rows, st, c = _run37(FVSolver, [24])
    assert rows.shape == (24, 8) and c["iterations"] == 24 and c["pressure_solves"] == 24 and c["pressure_caps"] == 0
    cases = dict(again=_run37(FVSolver, [24]), chunks=_run37(FVSolver, [7, 1, 9, 7]),
                 eager=_run37(FVSolver, [24], graph=False), graph=_run37(FVSolver, [24], graph=True),
                 pbudget2=_run37(FVSolver, [24], pressure_budget=2), pbudget8=_run37(FVSolver, [24], pressure_budget=8),
                 pbudget64=_run37(FVSolver, [24], pressure_budget=64),
                 graph_chunks_budgets2=_run37(FVSolver, [7, 1, 9, 7], graph=True, pressure_budget=2, linear_budget=2))
    for name, (rows2, st2, c2) in cases.items():
        assert np.array_equal(rows2, rows), name
        for k in ("u", "v", "p", "mdot"):
            assert np.array_equal(st2[k], st[k]), (name, k)
        for k in COUNTERS + PCOUNTERS:
            assert c2[k] == c[k], (name, k)
    print(f"CG iterations {c['pressure_iterations']} in {c['pressure_solves']} solves; retries: default "
          f"{c['pressure_budget_retries']}, 2 -> {cases['pbudget2'][2]['pressure_budget_retries']}, 64 -> "
          f"{cases['pbudget64'][2]['pressure_budget_retries']}")
    assert cases["pbudget2"][2]["pressure_budget_retries"] > 0 and cases["pbudget64"][2]["pressure_budget_retries"] == 0


def test_a_pressure_overflow_touches_neither_the_state_nor_the_control_words(fv):
    import torch
    from solvers.fv import ldc_fv_lib as F
    FVSolver, _ = fv
    rows, st, _ = _run37(FVSolver, [5])
    s = FVSolver(**dict(YAML, **CONSISTENT, nx=37, ny=50, Re=400.0, tolerance=1e-30, max_iterations=10**6, check_every=64))
    s._begin(1e-30)
    s._advance(2)
    before, ctrl, stats = s.state(), s.t["ctrl"].cpu().numpy().copy(), s.t["pstats"].cpu().numpy().copy()
    L, stream = F.lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.ldc_fv_wide_set_pressure_budget(s._wide, 1) == 0
    assert L.ldc_fv_wide_enqueue(s._wide, 3, 64, stream) == 0
    torch.cuda.synchronize()
    assert L.ldc_fv_wide_status(s._wide) == F.E_BUDGET
    assert int(s.t["scratch"][:1].view(torch.int64).item()) == F.OVERFLOW_PRESSURE
    assert np.array_equal(s.t["ctrl"].cpu().numpy(), ctrl) and np.array_equal(s.t["pstats"].cpu().numpy(), stats)
    for k in ("u", "v", "p", "mdot"):
        assert np.array_equal(s.state()[k], before[k]), k
    assert L.ldc_fv_wide_set_pressure_budget(s._wide, 64) == 0
    assert L.ldc_fv_wide_enqueue(s._wide, 3, 64, stream) == 0
    torch.cuda.synchronize()
    assert L.ldc_fv_wide_status(s._wide) == 0
    assert np.array_equal(s.t["rec"][:3].cpu().numpy(), rows[2:])
    for k in ("u", "v", "p", "mdot"):
        assert np.array_equal(s.state()[k], st[k]), k
    s.close()


# both modes, one trial above 256 cells on an axis, one with mixing; every trial leaves the batch at another chunk
BATCH = [dict(YAML, nx=13, ny=17, Re=400.0, check_every=5, max_iterations=17, pressure_equation="consistent"),
         dict(YAML, nx=37, ny=50, Re=400.0, check_every=7, max_iterations=12),
         dict(YAML, nx=24, ny=16, Re=100.0, convection_scheme="Upwind", check_every=16, max_iterations=14,
              pressure_equation="consistent", acceleration="anderson_chip", anderson_depth=3, anderson_start=4),
         dict(YAML, nx=300, ny=9, Re=400.0, corner_treatment="saad", check_every=64, max_iterations=8,
              pressure_equation="consistent"),
         dict(YAML, nx=16, ny=16, Re=100.0, check_every=9, max_iterations=10, acceleration="anderson_chip",
              anderson_depth=2, anderson_start=3)]


def _snapshot(s):
    st = s.state()
    return dict(st, history=np.array(s.history), ctrl=s.t["ctrl"].cpu().numpy().copy(), counters=s.counters(),
                astate=s.t["astate"].cpu().numpy().copy())


@pytest.mark.parametrize("pressure_budget", [24, 2])
def test_a_batch_of_both_modes_is_its_lone_chip_runs_bit_for_bit(fv, pressure_budget):
    FVSolver, BatchedFVSolver = fv
    trials = [dict(t, tolerance=1e-30, pressure_budget=pressure_budget) for t in BATCH]
    batch = BatchedFVSolver([dict(t, mapping="shared") for t in trials])
    batch.solve()
    assert batch.errors == {} and len(batch) == 5
    for q, (s, t) in enumerate(zip(batch.solvers, trials)):
        got = _snapshot(s)
        lone = FVSolver(**dict(t, mapping="chip", pressure_budget=24))
        lone.solve()
        want = _snapshot(lone)
        lone.close()
        print(q, f"{t['nx']}x{t['ny']}", got["counters"])
        assert got["history"].shape == (t["max_iterations"], 8)
        for k in ("u", "v", "p", "mdot", "history", "ctrl", "astate"):
            assert np.array_equal(got[k], want[k]), (q, k)
        for k in COUNTERS + (PCOUNTERS if s.consistent else ()):
            assert got["counters"][k] == want["counters"][k], (q, k)
    batch.close()


def test_a_reference_trial_is_still_the_reference_fixtures(fv):
    """pressure_equation="reference", spelled out, beside the new code: the upwind trajectory of g14 at its tolerances."""
    FVSolver, _ = fv
    g = np.load(GOLD / "g14_fv_traj.npz")
    tag = "nx24_ny16_Re100_none_K30"
    m = json.loads((GOLD / "g14_fv_traj.json").read_text())[tag]
    s = FVSolver(name="fv", Re=m["Re"], nx=m["nx"], ny=m["ny"], corner_treatment=m["lid"], alpha_uv=m["alpha_uv"],
                 alpha_p=m["alpha_p"], linear_solver_tol=m["linear_solver_tol"], convection_scheme=m["convection_scheme"],
                 tolerance=1e-30, max_iterations=m["K"], check_every=256, mapping="chip", pressure_equation="reference")
    s.solve()
    ref = g[f"{tag}_rec"]
    assert s.history.shape == ref.shape and _rows_rel(s.history[:, :7], ref[:, :7]) <= 1e-8
    st = s.state()
    for k in ("u", "v", "p", "mdot"):
        assert _rel(st[k], g[f"{tag}_{k}"]) <= 1e-8, k
    assert "pressure_solves" not in s.counters()
    s.close()


# ------------------------------------------------------------------------------------------- the cap
def test_a_cap_hit_is_counted_and_the_iterate_accepted(fv):
    import torch
    from solvers.fv import ldc_fv_lib as F
    FVSolver, _ = fv
    K = 12
    s = FVSolver(**dict(YAML, **CONSISTENT, nx=24, ny=16, Re=100.0, pressure_max_iters=3, tolerance=1e-30, max_iterations=K,
                        check_every=5))
    s.solve()
    torch.cuda.synchronize()
    assert F.lib().ldc_fv_wide_status(s._wide) == 0
    c = s.counters()
    print(c)
    assert (c["iterations"], c["nan"], c["done"]) == (K, 0, 0) and c["pressure_budget_retries"] == 0
    assert (c["pressure_iterations"], c["pressure_solves"], c["pressure_caps"], c["pressure_last"]) == (3 * K, K, K, 3)
    assert np.all(np.isfinite(s.history)) and all(np.all(np.isfinite(v)) for v in s.state().values())
    o = FVConsistentState(24, 16, 100.0, linear_solver_tol=1e-9, convection_scheme="TVD", pressure_max_iters=3)
    o.run(K)
    assert o.cg_caps == K
    for k, ref in (("u", o.u), ("v", o.v), ("p", o.p)):
        assert _rel(s.state()[k], ref.ravel()) <= 1e-9, k
    s.close()


# ------------------------------------------------------------------------------------------- sequencing, metrics
def test_sequencing_start_from_and_chip_metrics_take_such_a_trial(fv):
    """Coarse-to-fine sequencing (every level inherits the mode), start_from and vortex_metrics="chip".  Both solves stop
    when one iteration changes u by less than tol |u|_2; with a contraction rate rho (the largest ratio of successive
    changes over a run's last 20 rows) a run then stands within tol |u|_2 rho / (1 - rho) of the common fixed point, so the
    two differ by at most the sum of the two margins (2-norm, which bounds the largest entry).  A first version of this
    test asked for 1e-5 outright, ten times ONE iteration's change, which forgets the 1 / (1 - rho): the runs differ by
    3.0e-5 at rho = 0.99."""
    FVSolver, _ = fv
    from solvers.fv.fsg import FVFSGSolver
    kw = dict(YAML, **CONSISTENT, nx=32, ny=32, Re=100.0, tolerance=1e-6, max_iterations=5000, check_every=256,
              vortex_metrics="chip")
    lone = FVSolver(**kw)
    lone.solve()
    seq = FVFSGSolver(**dict(kw, name="fv_fsg", n_levels=2, coarsest_n=16))
    seq.solve()
    print(f"lone {lone.metrics.iterations} iterations, sequenced {seq.level_iterations}; psi_min {lone.metrics.psi_min:.6f} "
          f"{seq.metrics.psi_min:.6f}")
    assert lone.metrics.converged and seq.metrics.converged and len(seq.level_iterations) == 2
    assert seq.level_iterations[-1] < lone.metrics.iterations
    margin = 0.0
    for s in (lone, seq):
        rel = np.asarray(s.history)[-21:, 0]
        rho = float(np.max(rel[1:] / rel[:-1]))
        assert 0.0 < rho < 1.0
        margin += 1e-6 * np.linalg.norm(s.fields.u) * rho / (1.0 - rho)
    diff = float(np.max(np.abs(seq.fields.u - lone.fields.u)))
    print(f"max|du| {diff:.2e}, margin {margin:.2e}")
    assert diff <= margin and lone.metrics.psi_min < 0
    assert abs(seq.metrics.psi_min - lone.metrics.psi_min) <= 1e-3 * abs(lone.metrics.psi_min)
    again = FVSolver(**dict(kw, Re=200.0))
    again.start_from(lone)
    assert np.all(np.isfinite(again.state()["u"])) and np.max(np.abs(again.state()["u"])) > 0
    again.solve()
    assert again.metrics.converged
    for s in (lone, seq, again):
        s.close()


# ------------------------------------------------------------------------------------------- the launcher
def test_main_runs_a_consistent_chip_trial(tmp_path):
    r = subprocess.run([sys.executable, str(PKG / "main.py"), "solver=fv", "+solver.mapping=chip",
                        "+solver.pressure_equation=consistent", "N=32", "Re=400"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    res = list(tmp_path.rglob("results.json"))
    assert res, r.stderr[-3000:]
    rec = json.loads(res[0].read_text())
    print(rec["metrics"]["iterations"], rec["objective"])
    assert rec["solver"] == "fv" and rec["metrics"]["converged"] == 1
    assert np.isfinite(rec["objective"]) and rec["params"]["pressure_equation"] == "consistent"
