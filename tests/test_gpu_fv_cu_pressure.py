"""The consistent pressure equation of one-CU finite-volume trials (mapping="cu", pressure_equation="consistent_cu",
csrc/ldc_fv_cu_pressure.hip) on the GPU: one iteration from a developed state against a dense solve, trajectories against
the NumPy restatement (tests/fv_consistent_numpy.py), mass conservation row by row, solves to the latch, the chip chain,
bit equality across repeats, chunkings and batches of both modes with and without mixing, the accepted cap hit, a NaN
trial beside a healthy one, sequencing, device metrics, start_from, and the launcher."""
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
from test_gpu_fv_pressure import YAML  # noqa: E402

from conftest import PKG  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
C_RHS, Y = 23, 26                       # work vectors: rhs_p (entry 0 = 0) and x of the pressure solve (FvVec)
CU = dict(mapping="cu", pressure_equation="consistent_cu")
COUNTERS = ("done", "iterations", "nan", "linear_giveups", "linear_iterations", "momentum_solves", "anderson_fallbacks")
PCOUNTERS = ("pressure_iterations", "pressure_solves", "pressure_caps", "pressure_last")
FIELDS = ("u", "v", "p", "mdot")


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


def _devs(st, o):
    return {k: _rel(st[k], ref) for k, ref in (("u", o.u.ravel()), ("v", o.v.ravel()), ("p", o.p.ravel()),
                                               ("mdot", _mdot(o)))}


# ------------------------------------------------------------------------------------------- one iteration
@pytest.mark.parametrize("nx,ny", [(8, 8), (16, 16), (24, 16), (33, 19)])
def test_one_iteration_from_a_developed_state(fv, nx, ny):
    """20 iterations of the restatement, then ONE on the device with pressure_tol 1e-13.  The CG iterate x, read from its
    work vector, against the dense solve x* of the same system: A (x - x*) = -r with |r| <= pressure_tol |b|, and both lie
    (after their means are taken off) in the range of the symmetric positive semi-definite A, so
    |x - x*|_2 <= pressure_tol |b|_2 / lambda_min+(A), to which the rounding of x itself adds 64 eps |x|_2.  A, b and
    lambda_min+ are the test's own, from the restatement's weights.  Then u, v, p and mdot at the tolerance of the TVD
    trajectory test, and the CG count under the chip test's cap (the CPU restatement takes at most 28 at 1e-13)."""
    FVSolver, _ = fv
    tol = 1e-13
    o = _oracle(nx, ny, 100.0)
    o.run(20)
    s = FVSolver(**dict(YAML, **CU, nx=nx, ny=ny, Re=100.0, pressure_tol=tol, tolerance=1e-30, max_iterations=10**6,
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
    print(f"{nx}x{ny}: CG {c['pressure_last']} iterations, |x - x*| {err:.2e}, bound {bound:.2e} "
          f"(|b| {np.linalg.norm(b):.2e}, lambda_min+ {lam[1]:.2e}, |x| {np.linalg.norm(xsm):.2e}), "
          f"rhs_p {_rel(rhs[1:], b[1:]):.1e}")
    assert 1 <= c["pressure_last"] <= 40 and c["pressure_caps"] == 0 and c["pressure_solves"] == 1
    assert "pressure_budget_retries" not in c
    assert err <= bound
    devs = _devs(s.state(), o)
    print(devs)
    for k, d in devs.items():
        assert d <= 1e-9, k
    s.close()


# ------------------------------------------------------------------------------------------- trajectories
@pytest.mark.parametrize("nx,ny,scheme", [(16, 16, "TVD"), (24, 16, "Upwind"), (130, 9, "TVD")])
def test_trajectories_match_the_restatement(fv, nx, ny, scheme):
    """20 iterations from rest; the restatement solves every pressure system directly, the device to 1e-12.  130 x 9: an
    axis above 128 cells, where a wave of the GEMM loop takes more than one tile column."""
    FVSolver, _ = fv
    K = 20
    s = FVSolver(**dict(YAML, **CU, nx=nx, ny=ny, Re=100.0, convection_scheme=scheme, pressure_tol=1e-12,
                        tolerance=1e-30, max_iterations=K, check_every=8))
    s.solve()
    o = _oracle(nx, ny, 100.0, scheme)
    rec = o.run(K)
    devs = _devs(s.state(), o)
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
    twice that plus 64 eps sum |mdot| for the rounding of the four-term differences (the chip test's bound)."""
    FVSolver, _ = fv
    s = FVSolver(**dict(YAML, **CU, nx=nx, ny=ny, Re=Re, tolerance=1e-30, max_iterations=10**6, check_every=4))
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
@pytest.mark.parametrize("tag,N,Re,auv,ap,want", [("N16_Re100_04_02", 16, 100.0, 0.4, 0.2, 660),
                                                  ("N32_Re1000_07_03", 32, 1000.0, 0.7, 0.3, 958)])
def test_solve_to_the_latch_takes_the_restatements_iterations(fv, tag, N, Re, auv, ap, want):
    FVSolver, _ = fv
    g = np.load(GOLD / "g16_fv_consistent.npz")
    its, u, v = int(g[f"{tag}_iterations"]), g[f"{tag}_u"], g[f"{tag}_v"]
    assert its == want
    s = FVSolver(**dict(YAML, **CU, nx=N, ny=N, Re=Re, alpha_uv=auv, alpha_p=ap, tolerance=1e-6, max_iterations=3000,
                        check_every=256))
    s.solve()
    got = int(s.metrics.iterations)
    du, dv = np.max(np.abs(s.fields.u - u)), np.max(np.abs(s.fields.v - v))
    bound = (abs(got - want) + 1) * 1e-6 * np.max(np.abs(u))
    print(f"{tag}: {got} iterations (restatement {want}), max|du| {du:.2e} max|dv| {dv:.2e} bound {bound:.2e}; {s.counters()}")
    assert s.metrics.converged and abs(got - want) <= 2
    assert du <= bound and dv <= bound
    s.close()


# ------------------------------------------------------------------------------------------- the chip chain
def test_the_one_cu_kernel_follows_the_chip_chain(fv):
    """The same 37 x 50, Re 400 trial for 20 iterations on both mappings.  Each is within 1e-9 of the restatement
    (trajectory tests, here and in test_gpu_fv_pressure.py) and only the order of the sums differs: 2e-9 between them."""
    FVSolver, _ = fv
    kw = dict(YAML, nx=37, ny=50, Re=400.0, tolerance=1e-30, max_iterations=20, check_every=8)
    a = FVSolver(**dict(kw, **CU))
    a.solve()
    b = FVSolver(**dict(kw, mapping="chip", pressure_equation="consistent"))
    b.solve()
    sa, sb = a.state(), b.state()
    devs = {k: _rel(sa[k], sb[k]) for k in FIELDS}
    print(devs, a.counters(), b.counters())
    for k, d in devs.items():
        assert d <= 2e-9, k
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------- bit equality
def _run37(FVSolver, chunks, **kw):
    s = FVSolver(**dict(YAML, **CU, nx=37, ny=50, Re=400.0, tolerance=1e-30, max_iterations=10**6, check_every=64, **kw))
    s._begin(1e-30)
    rows = np.concatenate([s._advance(k)[0] for k in chunks], axis=0)
    out = (rows, s.state(), s.counters())
    s.close()
    return out


def test_runs_repeat_bit_for_bit_whatever_the_chunks(fv):
    FVSolver, _ = fv
    rows, st, c = _run37(FVSolver, [24])
    assert rows.shape == (24, 8) and c["iterations"] == 24 and c["pressure_solves"] == 24 and c["pressure_caps"] == 0
    assert c["pressure_iterations"] >= 24
    for name, (rows2, st2, c2) in dict(again=_run37(FVSolver, [24]), chunks=_run37(FVSolver, [7, 1, 9, 7])).items():
        assert np.array_equal(rows2, rows), name
        for k in FIELDS:
            assert np.array_equal(st2[k], st[k]), (name, k)
        for k in COUNTERS + PCOUNTERS:
            assert c2[k] == c[k], (name, k)


# both modes, with and without mixing, one trial with more than 128 cells on an axis; every trial leaves at another chunk
BATCH = [dict(YAML, nx=13, ny=17, Re=400.0, check_every=5, max_iterations=17, pressure_equation="consistent_cu"),
         dict(YAML, nx=37, ny=50, Re=400.0, check_every=7, max_iterations=12),
         dict(YAML, nx=24, ny=16, Re=100.0, convection_scheme="Upwind", check_every=16, max_iterations=14,
              pressure_equation="consistent_cu", acceleration="anderson", anderson_depth=3, anderson_start=4),
         dict(YAML, nx=200, ny=9, Re=400.0, corner_treatment="saad", check_every=64, max_iterations=8,
              pressure_equation="consistent_cu"),
         dict(YAML, nx=16, ny=16, Re=100.0, check_every=9, max_iterations=10, acceleration="anderson",
              anderson_depth=2, anderson_start=3)]


def _snapshot(s):
    st = s.state()
    return dict(st, history=np.array(s.history), ctrl=s.t["ctrl"].cpu().numpy().copy(), counters=s.counters(),
                astate=s.t["astate"].cpu().numpy().copy())


def test_a_batch_of_both_modes_is_its_lone_runs_bit_for_bit(fv):
    """Every trial's u, v, p, mdot, history, ctrl and counters are those of its lone run, bit for bit, and so is astate for
    the trials with mixing.  A trial WITHOUT mixing has no lone astate to equal: beside accelerated trials it rides through
    ldc_fv_anderson_enqueue at depth 0, where the mixing kernel keeps the iteration count it saw last in astate[2]
    (include/ldc_fv.h; tests/test_gpu_fv_anderson.py pins [0, 0, 40, 0] against the lone [0, 0, 0, 0]) for as long as an
    accelerated trial of the batch is live; after that the chunks are plain launches again.  So that word is a count up to
    the trial's own iterations, the three others are 0 as in the lone run, and the lone run's astate is all 0."""
    FVSolver, BatchedFVSolver = fv
    trials = [dict(t, tolerance=1e-30, mapping="cu") for t in BATCH]
    batch = BatchedFVSolver(trials)
    batch.solve()
    assert batch.errors == {} and len(batch) == 5
    for q, (s, t) in enumerate(zip(batch.solvers, trials)):
        got = _snapshot(s)
        lone = FVSolver(**t)
        lone.solve()
        want = _snapshot(lone)
        lone.close()
        print(q, f"{t['nx']}x{t['ny']}", got["counters"])
        assert got["history"].shape == (t["max_iterations"], 8)
        for k in FIELDS + ("history", "ctrl"):
            assert np.array_equal(got[k], want[k]), (q, k)
        if s.accelerated:
            assert np.array_equal(got["astate"], want["astate"]) and got["astate"][2] == t["max_iterations"], q
        else:
            assert list(got["astate"][[0, 1, 3]]) == [0, 0, 0] and 0 <= got["astate"][2] <= t["max_iterations"], q
            assert list(want["astate"]) == [0, 0, 0, 0], q
        assert got["counters"] == want["counters"], q
        assert ("pressure_solves" in got["counters"]) == s.consistent_cu
        if s.consistent_cu:
            assert got["counters"]["pressure_solves"] == t["max_iterations"]
    batch.close()


# ------------------------------------------------------------------------------------------- the cap
def test_a_cap_hit_is_counted_and_the_iterate_accepted(fv):
    FVSolver, _ = fv
    K = 12
    s = FVSolver(**dict(YAML, **CU, nx=24, ny=16, Re=100.0, pressure_max_iters=3, tolerance=1e-30, max_iterations=K,
                        check_every=5))
    s.solve()
    c = s.counters()
    print(c)
    assert (c["iterations"], c["nan"], c["done"]) == (K, 0, 0)
    assert (c["pressure_iterations"], c["pressure_solves"], c["pressure_caps"], c["pressure_last"]) == (36, 12, 12, 3)
    assert np.all(np.isfinite(s.history)) and all(np.all(np.isfinite(v)) for v in s.state().values())
    o = FVConsistentState(24, 16, 100.0, linear_solver_tol=1e-9, convection_scheme="TVD", pressure_max_iters=3)
    o.run(K)
    assert o.cg_caps == K
    devs = _devs(s.state(), o)
    print(devs)
    for k, d in devs.items():
        assert d <= 1e-9, k
    s.close()


# ------------------------------------------------------------------------------------------- a NaN
def test_a_nan_ends_the_trial_and_only_that_trial(fv):
    """One NaN in p of the first trial: its loops are bounded (BiCGSTAB and CG run to their caps on NaN data), the record's
    NaN stops it, and the healthy trial beside it in the launch is its lone run bit for bit."""
    FVSolver, BatchedFVSolver = fv
    from solvers.spectral.ldc_lib import LdcError
    t = dict(YAML, **CU, nx=16, ny=16, Re=100.0, tolerance=1e-30, max_iterations=12, check_every=5)
    batch = BatchedFVSolver([dict(t), dict(t)])
    n = 16 * 16
    p = np.zeros(n)
    p[7 * 16 + 5] = np.nan
    batch.solvers[0].set_state(np.zeros(n), np.zeros(n), p, np.zeros(batch.solvers[0].t["mdot"].numel()))
    batch.solve()
    assert list(batch.errors) == [0], batch.errors
    assert isinstance(batch.errors[0], LdcError) and "NaN" in str(batch.errors[0])
    c = batch.solvers[0].counters()
    print("NaN trial:", c)
    assert c["nan"] == 1 and int(batch.solvers[0].t["ctrl"][2].item()) == 1 and c["iterations"] == 1
    lone = FVSolver(**t)
    lone.solve()
    got, want = _snapshot(batch.solvers[1]), _snapshot(lone)
    for k in FIELDS + ("history", "ctrl"):
        assert np.array_equal(got[k], want[k]), k
    assert got["counters"] == want["counters"] and want["counters"]["nan"] == 0
    lone.close()
    batch.close()


# ------------------------------------------------------------------------------------------- sequencing, metrics
def test_sequencing_device_metrics_and_start_from_take_such_a_trial(fv):
    """Coarse-to-fine sequencing (every level inherits the mode), vortex_metrics="device" and start_from.  The margin
    between the sequenced and the lone solve is that of the chip test (test_gpu_fv_pressure.py): both stop when one
    iteration changes u by less than tol |u|_2; with a contraction rate rho (the largest ratio of successive changes over
    a run's last 20 rows) a run stands within tol |u|_2 rho / (1 - rho) of the common fixed point."""
    FVSolver, _ = fv
    from solvers.fv.fsg import FVFSGSolver
    kw = dict(YAML, **CU, nx=32, ny=32, Re=100.0, tolerance=1e-6, max_iterations=5000, check_every=256,
              vortex_metrics="device")
    lone = FVSolver(**kw)
    lone.solve()
    seq = FVFSGSolver(**dict(kw, name="fv_fsg", n_levels=2, coarsest_n=16))
    seq.solve()
    print(f"lone {lone.metrics.iterations} iterations, sequenced {seq.level_iterations}; psi_min {lone.metrics.psi_min:.6f} "
          f"{seq.metrics.psi_min:.6f}; {seq.counters()}")
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
    assert diff <= margin and lone.metrics.psi_min < 0 and seq.metrics.psi_min < 0
    again = FVSolver(**dict(kw, Re=200.0))
    again.start_from(lone)
    assert np.all(np.isfinite(again.state()["u"])) and np.max(np.abs(again.state()["u"])) > 0
    again.solve()
    assert again.metrics.converged and again.counters()["pressure_solves"] == again.metrics.iterations
    for s in (lone, seq, again):
        s.close()


# ------------------------------------------------------------------------------------------- the launcher
def test_main_runs_a_consistent_one_cu_trial(tmp_path):
    r = subprocess.run([sys.executable, str(PKG / "main.py"), "solver=fv", "+solver.pressure_equation=consistent_cu",
                        "N=32", "Re=400"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    res = list(tmp_path.rglob("results.json"))
    assert res, r.stderr[-3000:]
    rec = json.loads(res[0].read_text())
    print(rec["metrics"]["iterations"], rec["objective"])
    assert rec["solver"] == "fv" and rec["metrics"]["converged"] == 1
    assert np.isfinite(rec["objective"]) and rec["params"]["pressure_equation"] == "consistent_cu"
