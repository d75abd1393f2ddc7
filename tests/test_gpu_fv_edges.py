"""Finite-volume kernel on the GPU at its edges (csrc/ldc_fv_kernel.inc): sizes that are no multiple of 4 nor of the
16 x 16 MFMA tile, MAX_N and thin rectangles, Lx != Ly, lid_velocity != 1 and the smoothed lid (fixtures g15 and the
NumPy restatement), the pressure correction alone against a long-double solve, the BiCGSTAB exits and counters, the
reference's stopping iteration, chunk boundaries, repeat solves and the C ABI's refusals on a live handle."""
import ctypes as C
import functools
import json
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"
sys.path.insert(0, str(Path(__file__).resolve().parent))
from fv_numpy import FVState  # noqa: E402
from test_fv_cpu import ld_pressure_solve  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(float).eps)


@pytest.fixture(scope="module")
def fv():
    import __graft_entry__ as g
    g.build()
    from solvers.fv.batched import BatchedFVSolver
    from solvers.fv.solver import FVSolver
    return FVSolver, BatchedFVSolver


def _kwargs(m, **kw):
    """FVSolver keywords of a fixture's settings record (or of a dict laid out like one)."""
    args = dict(name="fv", Re=m["Re"], nx=m["nx"], ny=m["ny"], corner_treatment=m.get("lid", "none"),
                alpha_uv=m.get("alpha_uv", 0.4), alpha_p=m.get("alpha_p", 0.2),
                linear_solver_tol=m["linear_solver_tol"], convection_scheme=m["convection_scheme"],
                Lx=m.get("Lx", 1.0), Ly=m.get("Ly", 1.0), lid_velocity=m.get("lid_velocity", 1.0),
                tolerance=m.get("tolerance", 1e-30), max_iterations=10**6, check_every=256)
    args.update(kw)
    return args


def _restatement(m, **kw):
    return FVState(m["nx"], m["ny"], m["Re"], corner_treatment=m.get("lid", "none"), alpha_uv=m.get("alpha_uv", 0.4),
                   alpha_p=m.get("alpha_p", 0.2), linear_solver_tol=m["linear_solver_tol"],
                   convection_scheme=m["convection_scheme"], Lx=m.get("Lx", 1.0), Ly=m.get("Ly", 1.0),
                   lid_velocity=m.get("lid_velocity", 1.0), **kw)


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def _rows_err(got, ref):
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.max(np.abs(got[:, :7] - ref[:, :7]) / np.abs(ref[:, :7])))


def _state_of(o):
    return dict(u=o.u.ravel(), v=o.v.ravel(), p=o.p.ravel(), mdot=np.concatenate([o.fx.ravel(), o.fy.ravel()]))


def _assert_against(s, rows, ref_rows, ref_state, bound, what):
    err = _rows_err(rows, ref_rows)
    st = s.state()
    errs = {k: _rel(st[k], ref_state[k]) for k in ("u", "v", "p", "mdot")}
    print(what, "rows", err, errs)
    assert err <= bound, what
    for k, e in errs.items():
        assert e <= bound, (what, k)


def _assert_same_bits(a, b, what):
    """Everything a solve leaves behind, bit for bit (wall time aside)."""
    assert a.metrics.iterations == b.metrics.iterations, what
    assert a.metrics.converged == b.metrics.converged, what
    assert a.history.shape == b.history.shape and np.array_equal(a.history, b.history), what
    sa, sb = a.state(), b.state()
    for k in ("u", "v", "p", "mdot"):
        assert np.array_equal(sa[k], sb[k]), (what, k)
    assert a.counters() == b.counters(), what


# ------------------------------------------------------------------------------------------- a. fixtures at odd sizes
@pytest.mark.parametrize("tag", ["13x17", "37x50"])
def test_step_debug_matches_reference_at_odd_sizes(fv, tag):
    """g15_fv_step: 13 x 17, and 37 x 50 = 1850 cells (more than three strides of the 512 threads) on a 2 x 0.5 cavity
    with lid speed 2; bounds of test_gpu_fv.py::test_step_debug_matches_reference_intermediates."""
    g = np.load(GOLD / "g15_fv_step.npz")
    m = json.loads((GOLD / "g15_fv_step.json").read_text())[tag]
    s = fv[0](**_kwargs(m))
    s.set_state(g[f"{tag}_u0"], g[f"{tag}_v0"], g[f"{tag}_p0"], g[f"{tag}_mdot0"])
    out = s.step_debug()
    for k, v in out.items():
        assert np.all(np.isfinite(v)), k
        bound = 1e-8 if k == "p_prime" else 1e-10
        assert _rel(v, g[f"{tag}_{k}"]) <= bound, (k, _rel(v, g[f"{tag}_{k}"]))
    st = s.state()
    for k in ("u", "v", "p"):
        assert _rel(st[k], g[f"{tag}_{k}"]) <= 1e-10, k
    s.close()


@pytest.mark.parametrize("tag", ["13x17", "37x50"])
def test_production_and_debug_kernels_leave_the_same_bits(fv, tag):
    """The production kernel and ldc_fv_step_debug's are two instantiations of one template (csrc/ldc_fv_kernel.inc).
    One iteration from the seeded state of g15_fv_step through ``_advance(1)`` (production), ``step_debug()`` with
    every output selected and ``ldc_fv_step_debug`` with ``which = 0`` (debug, all copies and none): the same
    arithmetic, so u, v, p, mdot, record row 0 and the six ctrl words are equal bit for bit."""
    import torch
    from solvers.fv import ldc_fv_lib as F
    g = np.load(GOLD / "g15_fv_step.npz")
    m = json.loads((GOLD / "g15_fv_step.json").read_text())[tag]
    seed = [g[f"{tag}_{k}0"] for k in ("u", "v", "p", "mdot")]

    def production(s):
        s._advance(1)

    def debug_all(s):
        assert set(s.step_debug()) == set(F.DBG)

    def debug_none(s):
        with torch.cuda.device(s.device):
            F.check(F.lib().ldc_fv_step_debug(s.handle, 0, None, C.c_void_p(s._stream())), "ldc_fv_step_debug")
            torch.cuda.current_stream(s.device).synchronize()

    left = []
    for step in (production, debug_all, debug_none):
        s = fv[0](**_kwargs(m))
        s.set_state(*seed)
        step(s)
        left.append(dict(s.state(), row=s.t["rec"][0].cpu().numpy(), ctrl=s.t["ctrl"][:6].cpu().numpy()))
        s.close()
    ref = left[0]
    assert ref["ctrl"].tolist()[:3] == [0, 1, 0] and ref["ctrl"][5] == 2 and ref["ctrl"][4] > 0
    assert np.all(np.isfinite(ref["row"][:7])) and ref["row"][0] > 0
    for name, got in zip(("step_debug, all outputs", "ldc_fv_step_debug, which = 0"), left[1:]):
        for k in ("u", "v", "p", "mdot", "row", "ctrl"):
            assert np.array_equal(got[k], ref[k]), (name, k)


def test_upwind_trajectories_match_reference_at_odd_sizes(fv):
    """g15_fv_traj, each trial alone and all four as one batch: 1e-8, as test_upwind_trajectories_match_reference."""
    FVSolver, BatchedFVSolver = fv
    g = np.load(GOLD / "g15_fv_traj.npz")
    meta = json.loads((GOLD / "g15_fv_traj.json").read_text())
    assert len(meta) == 4
    trials = [_kwargs(m, max_iterations=m["K"]) for m in meta.values()]
    batch = BatchedFVSolver(trials)
    batch.solve()
    assert batch.errors == {}
    for (tag, m), t, b in zip(meta.items(), trials, batch.solvers):
        ref = {k: g[f"{tag}_{k}"] for k in ("u", "v", "p", "mdot")}
        s = FVSolver(**t)
        s.solve()
        _assert_against(s, s.history, g[f"{tag}_rec"], ref, 1e-8, tag + " lone")
        _assert_against(b, b.history, g[f"{tag}_rec"], ref, 1e-8, tag + " batched")
        s.close()
    batch.close()


# ------------------------------------------------------------------------------------------- b. TVD from a seeded state
def test_tvd_from_a_seeded_state_matches_restatement(fv):
    """The seeded state of g15_fv_step at 37 x 50 (both signs of every face flux, Lx = 2, Ly = 0.5, lid speed 2) put on
    both sides, then TVD: one step_debug, every intermediate, then 20 more iterations."""
    tag = "37x50"
    g = np.load(GOLD / "g15_fv_step.npz")
    m = dict(json.loads((GOLD / "g15_fv_step.json").read_text())[tag], convection_scheme="TVD")
    seed = [g[f"{tag}_{k}0"] for k in ("u", "v", "p", "mdot")]
    assert (seed[3] > 0).any() and (seed[3] < 0).any()
    s = fv[0](**_kwargs(m))
    o = _restatement(m)
    s.set_state(*seed)
    o.set_state(*seed)
    cap = {}
    o.step(cap)
    out = s.step_debug()
    assert set(out) == set(cap)
    for k, v in out.items():
        bound = 1e-8 if k == "p_prime" else 1e-10
        assert _rel(v, cap[k]) <= bound, (k, _rel(v, cap[k]))
    ref_rows = o.run(20)
    rows, _, total = s._advance(20)
    assert total == 21 and "cap" not in o.exits
    _assert_against(s, rows, ref_rows, _state_of(o), 1e-9, "seeded TVD")
    s.close()


# ------------------------------------------------------------------------------------------- c, d. shapes
SHAPES = [(13, 17, 40), (9, 250, 20), (256, 8, 20), (8, 256, 20), (131, 77, 15), (255, 253, 6), (256, 256, 4)]
SHAPE_IDS = [f"{nx}x{ny}" for nx, ny, _ in SHAPES]


def _shape_case(nx, ny):
    return dict(nx=nx, ny=ny, Re=400.0, linear_solver_tol=1e-12, convection_scheme="TVD")


@functools.lru_cache(maxsize=None)
def _shape_reference(nx, ny, K):
    """The restatement's K iterations from rest, computed once: (rows, state, exits)."""
    o = _restatement(_shape_case(nx, ny))
    rows = o.run(K)
    return rows, _state_of(o), tuple(o.exits)


@pytest.mark.parametrize("nx,ny,K", SHAPES, ids=SHAPE_IDS)
def test_tvd_trajectories_match_restatement_at_edge_shapes(fv, nx, ny, K):
    """Partial 16 x 16 tiles and K-remainders of the pressure GEMMs (13, 9, 131, 77, 255, 253), one tile along an axis
    (8, 9, 13) beside sixteen along the other, and MAX_N = 256 on both."""
    rows, state, exits = _shape_reference(nx, ny, K)
    assert "cap" not in exits and np.all(np.isfinite(rows))
    s = fv[0](**_kwargs(_shape_case(nx, ny), max_iterations=K))
    s.solve()
    _assert_against(s, s.history, rows, state, 1e-9, f"{nx}x{ny}")
    assert s.counters()["linear_giveups"] == 0
    s.close()


@pytest.mark.parametrize("nx,ny,K", SHAPES, ids=SHAPE_IDS)
def test_pressure_correction_alone_against_long_double(fv, nx, ny, K):
    """The four fp64-MFMA GEMMs in isolation: the kernel's p' of ITS OWN rhs_p (state after 3 iterations) against the
    long-double solve x_ld of that right-hand side.  With e = max |x_64 - x_ld| of the restatement's fp64 solve (same
    host eigenvectors, BLAS summation order), the kernel may be 8 e + 64 eps max |x_ld| away: another summation order
    over up to 256 terms, not another algorithm.  The kernel's side of this bound had not been measured when the test
    was written (profiles/fv_perf.md): the ratio got / e is printed per shape."""
    s = fv[0](**_kwargs(_shape_case(nx, ny)))
    s._begin(1e-30)
    s._advance(3)
    out = s.step_debug(("rhs_p", "p_prime"))
    s.close()
    rhs = out["rhs_p"].reshape(ny, nx)
    assert rhs.flat[0] == 0.0 and np.all(np.isfinite(rhs)) and np.max(np.abs(rhs)) > 0
    o = _restatement(_shape_case(nx, ny))
    x_ld = ld_pressure_solve(rhs, o.dx, o.dy)
    e = float(np.max(np.abs(o.pressure_solve(rhs) - x_ld)))
    got = float(np.max(np.abs(out["p_prime"].reshape(ny, nx) - x_ld)))
    top = float(np.max(np.abs(x_ld)))
    print(f"pressure {nx}x{ny}: kernel {got:.3e}  restatement e {e:.3e}  ratio {got / e:.3f}  max|x| {top:.3e}  "
          f"bound {8 * e + 64 * EPS * top:.3e}")
    assert got <= 8 * e + 64 * EPS * top


# ------------------------------------------------------------------------------------------- e. linear-solver exits
def test_capped_linear_solves_are_counted_and_accepted(fv, monkeypatch):
    """max_lin_iters = 3: every momentum solve but the first v solve (b = 0) gives up after 3 iterations and its
    iterate is accepted, as the reference accepts SciPy's non-convergence."""
    import solvers.fv.solver as S
    monkeypatch.setattr(S, "LINEAR_MAX_ITERATIONS", 3)
    K = 30
    m = dict(nx=13, ny=17, Re=100.0, linear_solver_tol=1e-12, convection_scheme="TVD")
    o = _restatement(m, max_lin_iters=3)
    ref_rows = o.run(K)
    assert o.exits.count("cap") == 59 and o.exits.count("b0") == 1 and sum(o.iters) == 177
    assert np.all(np.isfinite(ref_rows))
    s = fv[0](**_kwargs(m, max_iterations=K))
    s.solve()
    _assert_against(s, s.history, ref_rows, _state_of(o), 1e-9, "capped")
    c = s.counters()
    assert c["linear_giveups"] == o.exits.count("cap")
    assert c["linear_iterations"] == sum(o.iters)
    assert c["momentum_solves"] == 2 * K
    s.close()


@pytest.mark.parametrize("nx,ny,Re,scheme,lin_tol", [(13, 17, 100.0, "TVD", 1e-9), (30, 21, 400.0, "Upwind", 1e-6)],
                         ids=["13x17-TVD-1e-9", "30x21-Upwind-1e-6"])
def test_both_bicgstab_exits_and_unequal_u_v_counts(fv, nx, ny, Re, scheme, lin_tol):
    """Loose linear tolerances: solves end on |r| at the top of an iteration and on |s| in its middle, and u and v
    leave the shared loop at different iterations (restatement: 43 r / 36 s / 16 differing of 40, and 44 / 35 / 33)."""
    K = 40
    m = dict(nx=nx, ny=ny, Re=Re, linear_solver_tol=lin_tol, convection_scheme=scheme)
    o = _restatement(m)
    ref_rows = o.run(K)
    it = np.array(o.iters).reshape(-1, 2)
    assert "r" in o.exits and "s" in o.exits and "cap" not in o.exits
    assert int((it[:, 0] != it[:, 1]).sum()) >= 10
    s = fv[0](**_kwargs(m, max_iterations=K))
    s.solve()
    _assert_against(s, s.history, ref_rows, _state_of(o), 1e-8, f"{nx}x{ny} {scheme}")
    c = s.counters()
    print("linear iterations", c["linear_iterations"], "restatement", int(it.sum()))
    assert c["linear_giveups"] == 0 and c["momentum_solves"] == 2 * K
    assert abs(c["linear_iterations"] - int(it.sum())) <= 2 * K      # rounding may move a stopping test by one
    s.close()


# ------------------------------------------------------------------------------------------- f. stopping rule
METRIC_KEYS = ("final_energy", "final_enstrophy", "final_palinstrophy", "psi_min", "psi_min_x", "psi_min_y",
               "omega_center", "omega_max", "psi_BR", "psi_BL", "u_momentum_residual", "v_momentum_residual",
               "continuity_residual")


@pytest.fixture(scope="module")
def converged_case():
    meta = json.loads((GOLD / "g15_fv_converged.json").read_text())
    return meta, np.load(GOLD / "g15_fv_converged.npz")


def test_solve_stops_at_the_reference_iteration(fv, converged_case):
    """The reference's own solve() at 13 x 17, Re 100, tolerance 1e-4 stops after 280 iterations, its rel 9.5e-4
    (relative) below the tolerance there and 7.7e-3 above it one iteration earlier (g15_fv_converged)."""
    FVSolver, BatchedFVSolver = fv
    meta, g = converged_case
    ref = meta["metrics"]
    s = FVSolver(**_kwargs(meta))
    s.solve()
    m = s.metrics
    assert m.converged and m.iterations == ref["iterations"] == 280
    st = s.state()
    for k in ("u", "v", "p", "mdot"):
        assert _rel(st[k], g[k]) <= 1e-8, k
    for k in ("u", "v", "p"):
        assert np.array_equal(getattr(s.fields, k), st[k]), k
    assert abs(m.final_residual - ref["final_residual"]) <= 1e-8 * ref["final_residual"]
    for key in METRIC_KEYS:
        assert getattr(m, key) == pytest.approx(ref[key], rel=1e-7, abs=1e-10), key
    for key, n in meta["time_series_len"].items():
        assert len(getattr(s.time_series, key)) == n == 270, key
    assert _rel(np.array(s.time_series.rel_iter_residual), g["ts_rel_iter_residual"]) <= 1e-8
    # the same trial between two others of other sizes, schemes and tolerances
    batch = BatchedFVSolver([_kwargs(dict(nx=9, ny=30, Re=400.0, linear_solver_tol=1e-9, convection_scheme="TVD"),
                                     tolerance=1e-3, max_iterations=2000),
                             _kwargs(meta),
                             _kwargs(dict(nx=24, ny=16, Re=100.0, linear_solver_tol=1e-9, convection_scheme="Upwind"),
                                     tolerance=1e-5, max_iterations=150)])
    batch.solve()
    assert batch.errors == {}
    print("batch iterations", [b.metrics.iterations for b in batch.solvers])
    _assert_same_bits(batch.solvers[1], s, "batched")
    assert batch.solvers[1].metrics.iterations == 280 and batch.solvers[1].metrics.converged
    batch.close()
    s.close()


# ------------------------------------------------------------------------------------------- g. chunking
@pytest.mark.parametrize("max_iter", [None, 45], ids=["to-tolerance", "capped-45"])
def test_chunk_length_changes_nothing(fv, converged_case, max_iter):
    meta, _ = converged_case
    runs = []
    for every in (1, 7, 64, 256):
        s = fv[0](**_kwargs(meta, check_every=every))
        s.solve(max_iter=max_iter)
        runs.append(s)
    assert runs[0].metrics.iterations == (280 if max_iter is None else 45)
    assert runs[0].metrics.converged is (max_iter is None)
    assert runs[0].history.shape == (runs[0].metrics.iterations, 8)
    for every, s in zip((7, 64, 256), runs[1:]):
        _assert_same_bits(s, runs[0], f"check_every={every}")
    for s in runs:
        s.close()


# ------------------------------------------------------------------------------------------- h. repeat solves
def test_second_solve_on_a_converged_state_stops_after_the_warmup(fv, converged_case):
    meta, _ = converged_case
    s = fv[0](**_kwargs(meta))
    s.solve()
    assert s.metrics.iterations == 280 and s.metrics.converged
    s.solve(max_iter=50)
    assert s.metrics.iterations == 11 and s.metrics.converged
    assert s.history.shape == (11, 8) and len(s.time_series.rel_iter_residual) == 1
    assert np.all(s.history[:, 0] < meta["tolerance"])      # converged all along: only the warm-up kept it going
    c = s.counters()
    assert (c["done"], c["iterations"], c["momentum_solves"]) == (1, 11, 22)
    s.close()


def test_two_capped_solves_continue_like_one(fv, converged_case):
    """30 + 30 iterations leave the state of 60: a new solve() keeps the fields and restarts only the count (the
    warm-up's rel is not consulted, so the arithmetic is the same; asserted to 1e-12)."""
    meta, _ = converged_case
    a, b = fv[0](**_kwargs(meta)), fv[0](**_kwargs(meta))
    a.solve(max_iter=30)
    assert a.metrics.iterations == 30 and not a.metrics.converged
    first = a.history.copy()
    a.solve(max_iter=30)
    assert a.metrics.iterations == 30 and not a.metrics.converged and a.history.shape == (30, 8)
    assert a.counters()["iterations"] == 30 and a.counters()["momentum_solves"] == 60
    b.solve(max_iter=60)
    assert b.metrics.iterations == 60
    sa, sb = a.state(), b.state()
    for k in ("u", "v", "p", "mdot"):
        assert _rel(sa[k], sb[k]) <= 1e-12, k
    assert _rows_err(np.concatenate([first, a.history]), b.history) <= 1e-12
    a.close()
    b.close()


def test_batched_repeat_solves_equal_lone_repeat_solves(fv, converged_case):
    FVSolver, BatchedFVSolver = fv
    meta, _ = converged_case
    trials = [_kwargs(meta), _kwargs(dict(nx=9, ny=30, Re=400.0, linear_solver_tol=1e-9, convection_scheme="TVD"),
                                     tolerance=1e-3, max_iterations=40)]
    batch = BatchedFVSolver(trials)
    lone = [FVSolver(**t) for t in trials]
    for max_iter in (None, 50, 25):
        batch.solve(max_iter=max_iter)
        assert batch.errors == {}
        for q, (b, s) in enumerate(zip(batch.solvers, lone)):
            s.solve(max_iter=max_iter)
            print(max_iter, q, "iterations", b.metrics.iterations, s.metrics.iterations, b.metrics.converged)
            _assert_same_bits(b, s, (max_iter, q))
    assert [s.metrics.iterations for s in batch.solvers][0] == 11
    batch.close()
    for s in lone:
        s.close()


# ------------------------------------------------------------------------------------------- i. C ABI, live handle
def test_enqueue_refuses_more_iterations_than_the_record_holds(fv):
    import torch
    from solvers.fv import ldc_fv_lib as F
    m = dict(nx=13, ny=17, Re=100.0, linear_solver_tol=1e-9, convection_scheme="TVD")
    a, b = fv[0](**_kwargs(m, check_every=4)), fv[0](**_kwargs(m, check_every=8))
    assert (a.rec_cap, b.rec_cap) == (4, 8)
    for s in (a, b):
        s._begin(1e-30)
        s._advance(3)
    before = [(s.counters(), s.state(), s.t["rec"].cpu().numpy().copy()) for s in (a, b)]
    assert before[0][0]["iterations"] == 3
    L = F.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.ldc_fv_enqueue(a.handle, a.rec_cap + 1, stream) == -1
    assert L.ldc_fv_enqueue(a.handle, 0, stream) == -1
    arr = (C.c_void_p * 2)(b.handle.value, a.handle.value)
    assert L.ldc_fv_batch_enqueue(arr, 2, 5, stream) == -1        # fits b's record, not a's: neither is launched
    assert L.ldc_fv_batch_enqueue(arr, 2, 0, stream) == -1
    torch.cuda.synchronize()
    for s, (ctrl, st, rec) in zip((a, b), before):
        assert s.counters() == ctrl
        assert np.array_equal(s.t["rec"].cpu().numpy(), rec)
        for k in ("u", "v", "p", "mdot"):
            assert np.array_equal(s.state()[k], st[k]), k
    assert L.ldc_fv_batch_enqueue(arr, 2, 4, stream) == 0         # and the handles are still good
    torch.cuda.synchronize()
    assert a.counters()["iterations"] == b.counters()["iterations"] == 7
    a.close()
    b.close()


def test_a_lone_nan_trial_raises(fv):
    """16 x 16, Re 1000 without under-relaxation overflows within about ten iterations (the case of
    test_gpu_fv_batched.py); the kernel's NaN latch stops the trial and a lone solve() raises what the batch stores."""
    from solvers.spectral.ldc_lib import LdcError
    s = fv[0](name="fv", nx=16, ny=16, Re=1000.0, convection_scheme="TVD", alpha_uv=1.0, alpha_p=1.0,
              linear_solver_tol=1e-9, tolerance=1e-5, max_iterations=2000, check_every=256)
    with pytest.raises(LdcError, match="NaN"):
        s.solve()
    c = s.counters()
    assert c["nan"] == 1 and c["done"] == 0 and c["iterations"] < 256
    s.close()
