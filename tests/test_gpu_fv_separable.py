"""The separable scaled preconditioner of the stretched-grid pressure CG (pressure_preconditioner="separable",
ldc_fv_set_preconditioner, csrc/ldc_fv_stretched_sep.hip) on the GPU: trajectories against the NumPy restatement
(tests/fv_separable_numpy.py), the CG iterate against a dense solve, CG counts against the restatement's and against the
constant-coefficient preconditioner's on the card, bit equality in a mixed batch of all five launch groups and across repeats
and chunkings, and a solve to the latch with both preconditioners."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"
sys.path.insert(0, str(Path(__file__).resolve().parent))
from fv_separable_numpy import FVSeparableState  # noqa: E402
from fv_stretched_numpy import BOTELLA_RE1000, centreline_extrema  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
C_RHS, Y = 23, 26                       # work vectors: rhs_p (entry 0 = 0) and x of the pressure solve (FvVec)
FIELDS = ("u", "v", "p", "mdot")
SEP = dict(grid="tanh", pressure_equation="consistent_cu", pressure_preconditioner="separable")
LAP = dict(grid="tanh", pressure_equation="consistent_cu", pressure_preconditioner="laplacian")


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


def _mdot(o):
    return np.concatenate([o.fx.ravel(), o.fy.ravel()])


def _devs(st, o):
    return {k: _rel(st[k], ref) for k, ref in (("u", o.u.ravel()), ("v", o.v.ravel()), ("p", o.p.ravel()), ("mdot", _mdot(o)))}


# ------------------------------------------------------------------------------------------- trajectories
@pytest.mark.parametrize("nx,ny,beta,geo", [(16, 16, 1.5, {}), (24, 16, 1.0, {}), (13, 17, 1.5, dict(Lx=2.0, Ly=0.5))])
def test_tvd_trajectories_match_the_restatement(fv, nx, ny, beta, geo):
    """30 TVD iterations from rest with both tolerances 1e-12 against the restatement with the dense pressure solve, by the
    rules of tests/test_gpu_fv_stretched.py::test_tvd_trajectories_match_the_restatement: fields and record columns to 1e-9,
    |div mdot| (column 3) against the size of the fluxes; K solves, no caps, wall fluxes exactly 0.0."""
    FVSolver, _ = fv
    K = 30
    s = FVSolver(name="fv", Re=100.0, nx=nx, ny=ny, convection_scheme="TVD", alpha_uv=0.4, alpha_p=0.2,
                 linear_solver_tol=1e-12, grid_stretch=beta, pressure_tol=1e-12, tolerance=1e-30, max_iterations=K,
                 check_every=8, **SEP, **geo)
    assert s.separable
    s.solve()
    o = FVSeparableState(nx, ny, 100.0, linear_solver_tol=1e-12, convection_scheme="TVD", grid_stretch=beta,
                         pressure_equation="consistent", pressure_solver="direct", **geo)
    rec = o.run(K)
    st = s.state()
    devs = _devs(st, o)
    cols = [0, 1, 2, 4, 5, 6]
    c = s.counters()
    print(f"{nx}x{ny} beta {beta}: records {_rows_rel(s.history[:, cols], rec[:, cols]):.2e}, "
          f"div {np.max(np.abs(s.history[:, 3] - rec[:, 3])):.2e}, fields {devs}, {c}")
    assert s.history.shape == rec.shape
    assert _rows_rel(s.history[:, cols], rec[:, cols]) <= 1e-9
    assert np.max(np.abs(s.history[:, 3] - rec[:, 3])) <= 1e-9 * np.max(np.abs(_mdot(o)))
    for k, d in devs.items():
        assert d <= 1e-9, k
    assert c["pressure_caps"] == 0 and c["pressure_solves"] == K and c["iterations"] == K and c["nan"] == 0
    m = st["mdot"]
    fx, fy = m[: ny * (nx + 1)].reshape(ny, nx + 1), m[ny * (nx + 1):].reshape(ny + 1, nx)
    assert not fx[:, 0].any() and not fx[:, -1].any() and not fy[0].any() and not fy[-1].any()      # walls: exactly 0.0
    s.close()


# ------------------------------------------------------------------------------------------- one solve
@pytest.mark.parametrize("nx,ny,beta,geo", [(16, 16, 1.5, {}), (13, 17, 1.5, dict(Lx=2.0, Ly=0.5)), (24, 16, 1.0, {})])
def test_one_iteration_from_a_developed_state(fv, nx, ny, beta, geo):
    """The residual condition of tests/test_gpu_fv_cu_pressure.py::test_one_iteration_from_a_developed_state: 20 iterations of
    the restatement, then ONE on the device with pressure_tol 1e-13; x from work vector 26 against the dense solve x* of the
    same system, |x - x*|_2 <= pressure_tol |b|_2 / lambda_min+(A) + 64 eps |x*|_2 after both means are taken off, and rhs_p
    from work vector 23 with its entry 0 at 0."""
    FVSolver, _ = fv
    tol = 1e-13
    o = FVSeparableState(nx, ny, 100.0, linear_solver_tol=1e-9, convection_scheme="TVD", grid_stretch=beta,
                         pressure_equation="consistent", pressure_solver="direct", **geo)
    o.run(20)
    s = FVSolver(name="fv", Re=100.0, nx=nx, ny=ny, convection_scheme="TVD", alpha_uv=0.4, alpha_p=0.2,
                 linear_solver_tol=1e-9, grid_stretch=beta, pressure_tol=tol, tolerance=1e-30, max_iterations=10**6,
                 check_every=8, **SEP, **geo)
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
    assert err <= bound
    for k, d in _devs(s.state(), o).items():
        assert d <= 1e-9, k
    s.close()


# ------------------------------------------------------------------------------------------- CG counts
@pytest.mark.parametrize("nx,ny,geo", [(16, 16, {}), (13, 17, dict(Lx=2.0, Ly=0.5))])
def test_cg_counts_follow_the_restatement_and_halve_the_laplacian_ones(fv, nx, ny, geo):
    """beta 1.5, Re 100, TVD, 0.7 / 0.3, pressure_tol 1e-8, 30 iterations from rest, one iteration per launch so that every
    solve's count is read (pressure_last).  Each differs from the restatement's by at most one (a stop test at the threshold
    may flip with rounding), so the totals differ by at most one per solve; and the total is at most half that of the same
    trial with the constant-coefficient preconditioner, run here too.  The restatement: 11.9 against 40.4 per solve at 16 x 16,
    8.9 against 36.7 at 13 x 17."""
    FVSolver, _ = fv
    K = 30
    kw = dict(name="fv", Re=100.0, nx=nx, ny=ny, convection_scheme="TVD", alpha_uv=0.7, alpha_p=0.3, linear_solver_tol=1e-9,
              grid_stretch=1.5, pressure_tol=1e-8, pressure_max_iters=300, tolerance=1e-30, max_iterations=10**6,
              check_every=8, **geo)
    o = FVSeparableState(nx, ny, 100.0, alpha_uv=0.7, alpha_p=0.3, linear_solver_tol=1e-9, convection_scheme="TVD",
                         grid_stretch=1.5, pressure_equation="consistent", pressure_solver="cg", pressure_tol=1e-8,
                         pressure_max_iters=300, **geo)
    o.run(K)
    assert o.cg_caps == 0
    totals = {}
    for name, mode in (("separable", SEP), ("laplacian", LAP)):
        s = FVSolver(**kw, **mode)
        s._begin(1e-30)
        per_solve = []
        for _ in range(K):
            s._advance(1)
            per_solve.append(s.counters()["pressure_last"])
        c = s.counters()
        assert c["pressure_caps"] == 0 and c["pressure_solves"] == K and c["pressure_iterations"] == sum(per_solve)
        totals[name] = c["pressure_iterations"]
        if name == "separable":
            worst = max(abs(a - b) for a, b in zip(per_solve, o.cg_iters))
            print(f"{nx}x{ny}: card {per_solve}\n restatement {o.cg_iters}")
            assert worst <= 1
            assert abs(totals[name] - sum(o.cg_iters)) <= K
        s.close()
    print(f"{nx}x{ny}: CG iterations in {K} solves: separable {totals['separable']}, laplacian {totals['laplacian']}, "
          f"restatement (separable) {sum(o.cg_iters)}")
    assert totals["separable"] <= 0.5 * totals["laplacian"]


# ------------------------------------------------------------------------------------------- bit equality
BATCH = [dict(nx=13, ny=17, grid_stretch=1.5, **SEP),
         dict(nx=32, ny=32, grid_stretch=1.5, Re=400.0, **SEP),
         dict(nx=16, ny=16, grid_stretch=1.5, **LAP),
         dict(nx=16, ny=16, grid="tanh", grid_stretch=1.0, pressure_equation="reference", corner_treatment="saad"),
         dict(nx=16, ny=16, pressure_equation="consistent_cu"),
         dict(nx=16, ny=16)]
BASE = dict(name="fv", Re=100.0, convection_scheme="TVD", alpha_uv=0.4, alpha_p=0.2, linear_solver_tol=1e-9, tolerance=1e-30,
            check_every=32)


def _lone(FVSolver, kw, chunks=(24,)):
    s = FVSolver(**dict(BASE, **kw))
    s._begin(1e-30)
    rows = np.concatenate([s._advance(k)[0] for k in chunks], axis=0)
    out = (rows, s.state(), s.counters())
    s.close()
    return out


def test_a_mixed_batch_is_bit_equal_to_the_lone_runs(fv):
    """One ldc_fv_batch_enqueue over two separable trials, a stretched trial with the constant-coefficient preconditioner, a
    stretched reference trial, a uniform consistent and a uniform reference trial: five launch groups.  Every trial is
    bit-equal to its lone run in rec, the fields and counters()."""
    import torch
    from solvers.fv import ldc_fv_lib as F
    FVSolver, _ = fv
    lone = [_lone(FVSolver, kw) for kw in BATCH]
    batch = [FVSolver(**dict(BASE, **kw)) for kw in BATCH]
    assert [s.separable for s in batch] == [True, True, False, False, False, False]
    for s in batch:
        s._begin(1e-30)
    F.batch_enqueue([s.handle for s in batch], 24, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for q, (s, (rows, st, c)) in enumerate(zip(batch, lone)):
        assert np.array_equal(s.t["rec"][:24].cpu().numpy(), rows), q
        got = s.state()
        for k in FIELDS:
            assert np.array_equal(got[k], st[k]), (q, k)
        assert s.counters() == c and c["iterations"] == 24 and c["nan"] == 0, q
        s.close()
    # the two preconditioners are different kernels: the same trial takes fewer CG iterations
    sep = _lone(FVSolver, dict(nx=16, ny=16, grid_stretch=1.5, **SEP))
    assert sep[2]["pressure_iterations"] < lone[2][2]["pressure_iterations"]


def test_the_batched_solver_takes_separable_trials(fv):
    """BatchedFVSolver over the same mix, to each trial's own cap: histories and fields are those of the lone solves."""
    FVSolver, Batched = fv
    trials = [dict(BASE, **kw, max_iterations=20 + 3 * q) for q, kw in enumerate(BATCH)]
    b = Batched(trials)
    b.solve()
    assert not b.errors
    for t, s in zip(trials, b.solvers):
        one = FVSolver(**t)
        one.solve()
        assert np.array_equal(one.history, s.history)
        for k in ("u", "v", "p"):
            assert np.array_equal(getattr(one.fields, k), getattr(s.fields, k)), k
        assert one.counters() == s.counters()
        one.close()
    b.close()


def test_a_repeat_solve_on_one_handle_is_bit_equal(fv):
    """Two solves from the same state on ONE handle, and a third in other chunks: the same bits (fixed summation order, no
    state kept in the kernel between launches; s and s . r are rewritten by every solve)."""
    FVSolver, _ = fv
    for kw in BATCH[:2]:
        s = FVSolver(**dict(BASE, **kw))
        runs = []
        for chunks in ((24,), (24,), (7, 1, 16)):
            z = np.zeros(s.n_cells)
            s.set_state(z, z, z, np.zeros(s.t["mdot"].numel()))
            s._begin(1e-30)
            rows = np.concatenate([s._advance(k)[0] for k in chunks], axis=0)
            runs.append((rows, s.state(), s.counters()))
        assert runs[0][0].shape == (24, 8) and runs[0][2]["pressure_solves"] == 24
        for rows, st, c in runs[1:]:
            assert np.array_equal(rows, runs[0][0]) and c == runs[0][2]
            for k in FIELDS:
                assert np.array_equal(st[k], runs[0][1][k]), k
        s.close()


def test_the_mode_follows_the_calls_on_one_handle(fv):
    """On ONE handle: ldc_fv_set_preconditioner(NULL) and a new ldc_fv_set_grid both give the run of a "laplacian" trial, bit
    for bit, and attaching the tables again gives the separable run back."""
    from solvers.fv import ldc_fv_lib as F
    FVSolver, _ = fv
    kw = dict(nx=13, ny=17, grid_stretch=1.5)
    want = {name: _lone(FVSolver, dict(kw, **mode)) for name, mode in (("separable", SEP), ("laplacian", LAP))}
    assert want["separable"][2]["pressure_iterations"] < want["laplacian"][2]["pressure_iterations"]
    s = FVSolver(**dict(BASE, **kw, **SEP))
    t = s.t

    def run():
        z = np.zeros(s.n_cells)
        s.set_state(z, z, z, np.zeros(t["mdot"].numel()))
        s._begin(1e-30)
        return s._advance(24)[0], s.state(), s.counters()

    def attach():
        F.set_preconditioner(s.handle, t["precx"].data_ptr(), t["precx"].numel(), t["precy"].data_ptr(), t["precy"].numel())

    steps = [("separable", lambda: None),
             ("laplacian", lambda: F.check(F.lib().ldc_fv_set_preconditioner(s.handle, None), "ldc_fv_set_preconditioner")),
             ("separable", attach),
             ("laplacian", lambda: F.set_grid(s.handle, t["gridx"].data_ptr(), t["gridx"].numel(), t["gridy"].data_ptr(),
                                              t["gridy"].numel())),
             ("separable", attach)]
    for q, (name, call) in enumerate(steps):
        call()
        rows, st, c = run()
        assert np.array_equal(rows, want[name][0]) and c == want[name][2], (q, name)
        for k in FIELDS:
            assert np.array_equal(st[k], want[name][1][k]), (q, name, k)
    s.close()


# ------------------------------------------------------------------------------------------- a solve to the latch
def test_both_preconditioners_stop_at_the_restatements_count(fv):
    """32 x 32, Re 1000, beta 1.5, TVD, consistent_cu, 0.7 / 0.3, tolerance 1e-7 (tests/golden/g17_fv_stretched_converged.json:
    the restatement stops after 1704 iterations, 4.6e-4 and 7.7e-4 relative away from the tolerance), with both
    preconditioners on the card.  Both stop at that count.  The field bound: the two RESTATEMENT runs (FVStretchedState and
    FVSeparableState, the same settings, on the CPU) both stop at 1704 and differ at their stops by 6.37e-11 at most over u, v
    and p (u 1.10e-12, v 1.03e-12, p 6.37e-11; mdot 5.4e-14), with 43.2 and 17.0 CG iterations per solve.  Both solve the same
    equation to pressure_tol, so that figure measures the tolerance and not the code under test; ten times it, 6.37e-10, is
    allowed between the card's two runs.  The three centreline errors print as in profiles/fv_stretched.md: 2.5e-02, 2.4e-02,
    1.8e-02."""
    FVSolver, _ = fv
    want = json.loads((GOLD / "g17_fv_stretched_converged.json").read_text())
    assert want["iterations"] == 1704 and min(want["margins"].values()) >= 1e-4
    measured = 6.37e-11
    kw = dict(name="fv", Re=1000.0, nx=32, ny=32, convection_scheme="TVD", alpha_uv=0.7, alpha_p=0.3, linear_solver_tol=1e-9,
              grid_stretch=1.5, pressure_tol=1e-8, pressure_max_iters=200, tolerance=1e-7, max_iterations=5000, check_every=512)
    out = {}
    for name, mode in (("laplacian", LAP), ("separable", SEP)):
        s = FVSolver(**kw, **mode)
        s.solve()
        c = s.counters()
        ny, nx = s.shape_full
        xs, ys = s.fields.x.reshape(ny, nx)[0], s.fields.y.reshape(ny, nx)[:, 0]
        ext = centreline_extrema(s.fields.u.reshape(ny, nx), s.fields.v.reshape(ny, nx), xs, ys)
        err = {k: abs(abs(ext[k]) - abs(BOTELLA_RE1000[k])) for k in ext}
        print(name, int(s.metrics.iterations), ext, err, c)
        assert s.metrics.converged and c["pressure_caps"] == 0 and c["linear_giveups"] == 0 and c["nan"] == 0
        assert int(s.metrics.iterations) == want["iterations"]
        assert [f"{err[k]:.1e}" for k in ("u_min", "v_max", "v_min")] == ["2.5e-02", "2.4e-02", "1.8e-02"]
        for k in ext:
            assert abs(ext[k] - want["extrema"][k]) <= 1e-6, k
        out[name] = (s.state(), c["pressure_iterations"] / c["pressure_solves"])
        s.close()
    diffs = {k: float(np.max(np.abs(out["separable"][0][k] - out["laplacian"][0][k]))) for k in ("u", "v", "p")}
    print(f"card, separable against laplacian at the stop: {diffs}; CG per solve {out['laplacian'][1]:.1f} and "
          f"{out['separable'][1]:.1f}")
    assert out["laplacian"][1] == pytest.approx(want["cg_iterations_mean"], abs=1.0)
    assert out["separable"][1] <= 0.5 * out["laplacian"][1]
    assert max(diffs.values()) <= 10 * measured
