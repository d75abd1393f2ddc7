"""The three stretched-grid kernels of a one-CU finite-volume trial on the GPU at their edges (fv_stretched_kernel<false>,
fv_stretched_kernel<true>, fv_stretched_sep_kernel; csrc/ldc_fv_stretched.hip, csrc/ldc_fv_stretched_sep.hip,
csrc/ldc_fv_stretched_phases.inc): every phase of one iteration from a seeded state with both signs among the face fluxes,
read from the work vectors (tests/fv_stretched_probe.py); trajectories at sizes that take several strides of the 512
threads, partial MFMA tiles, MIN_N beside MAX_N, MAX_N on both axes and a grid_stretch of 2.5; CG counts there; pressure
solves and BiCGSTAB solves that end at their caps; the NaN latch; more handles than one launch takes; repeat solves and chunk
lengths at four strides.  "reference", "laplacian" and "separable" name the three kernels throughout.

The restatement runs are the probe's, made once per case; tests/test_fv_stretched_edges_cpu.py asserts their preconditions.
Measured deviations and times: profiles/fv_stretched_edges.md."""
import sys
import time
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import fv_stretched_probe as P  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(float).eps)
FIELDS = ("u", "v", "p", "mdot")
CONSISTENT_COLS = [0, 1, 2, 4, 5, 6]            # |div mdot| (3) of a converged CG has no digits: held against max |mdot|


@pytest.fixture(scope="module")
def fv():
    import __graft_entry__ as g
    g.build()
    from solvers.fv.batched import BatchedFVSolver
    from solvers.fv.solver import FVSolver
    return FVSolver, BatchedFVSolver


def _rel(a, b):
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def _rows_rel(got, ref):
    den = np.where(ref == 0.0, 1.0, np.abs(ref))
    return float(np.max(np.abs(got - ref) / den))


def _walls(m, nx, ny):
    fx, fy = m[: ny * (nx + 1)].reshape(ny, nx + 1), m[ny * (nx + 1):].reshape(ny + 1, nx)
    return fx[:, 0], fx[:, -1], fy[0], fy[-1]


def _trajectory_devs(rows, state, ref_rows, ref_state, kernel):
    """(record columns relative, column 3 over max |mdot|, fields relative) against a restatement run."""
    assert rows.shape == ref_rows.shape, (rows.shape, ref_rows.shape)
    assert np.all(np.isfinite(rows[:, :7]))
    cols = list(range(7)) if kernel == "reference" else CONSISTENT_COLS
    devs = dict(rows=_rows_rel(rows[:, cols], ref_rows[:, cols]),
                div=float(np.max(np.abs(rows[:, 3] - ref_rows[:, 3])) / np.max(np.abs(ref_state["mdot"]))))
    devs.update({k: _rel(state[k], ref_state[k]) for k in FIELDS})
    return devs


def _assert_trajectory(what, devs, bound):
    print(f"EDGE {what}: " + ", ".join(f"{k} {v:.2e}" for k, v in devs.items()) + f" (bound {bound:.0e})")
    for k, v in devs.items():
        assert v <= bound, (what, k, v)


def _assert_same_bits(a, b, what):
    """Everything a solve leaves behind, bit for bit."""
    assert a.metrics.iterations == b.metrics.iterations and a.metrics.converged == b.metrics.converged, what
    assert a.history.shape == b.history.shape and np.array_equal(a.history, b.history), what
    sa, sb = a.state(), b.state()
    for k in FIELDS:
        assert np.array_equal(sa[k], sb[k]), (what, k)
    assert a.counters() == b.counters(), what


# ------------------------------------------------------------------------------------------- a. phases from a seeded state
@pytest.mark.parametrize("kernel", P.KERNELS)
@pytest.mark.parametrize("tag", P.PHASE_TAGS)
def test_every_phase_of_one_iteration_from_a_seeded_state(fv, tag, kernel):
    """The seeds of g17's step fixtures (13 x 17 at beta 1.5; 37 x 50 = 1850 cells at beta 1, Lx 2, Ly 0.5, lid 2, Re 400) with
    TVD on both sides, one ``step(capture)`` of the restatement with the dense pressure solve against one ``_advance(1)``.
    Relative to max |ref|, as tests/test_gpu_fv_edges.py::test_step_debug_matches_reference_at_odd_sizes: 1e-10 up to rhs_p,
    1e-8 for the reference kernel's p', 1e-9 for u', v', mdot, omega, the record row and u, v, p.  The first key that departs
    names the phase.  A consistent kernel's p' by the residual condition of
    tests/test_gpu_fv_separable.py::test_one_iteration_from_a_developed_state, x* the dense solve of the kernel's own
    right-hand side with the restatement's A.  Then ten more iterations on both sides to 1e-9."""
    m, seed = P.phase_case(tag)
    nx, ny = m["nx"], m["ny"]
    consistent = kernel != "reference"
    tol = P.PHASE_TOL["pressure_tol"]
    ref = P.phase_reference(tag, consistent)
    cap = ref["cap"]
    s = fv[0](**P.phase_solver_kwargs(m, kernel))
    assert s.stretched and s.separable == (kernel == "separable") and s.consistent_cu == consistent
    s.set_state(*seed)
    t0 = time.perf_counter()
    rows, done, total = s._advance(1)
    dt = time.perf_counter() - t0
    assert total == 1 and not done and rows.shape == (1, 8) and np.all(np.isfinite(rows[:, :7]))
    got = P.intermediates(s, kernel)
    st = s.state()
    c = s.counters()
    devs = {}
    for k in ("grad_p", "diag", "b", "u_star", "v_star", "mdot_star", "rhs_p"):            # in the order of the phases
        if k == "mdot_star" and not consistent:
            continue
        assert np.all(np.isfinite(got[k])), k
        devs[k] = (_rel(got[k], cap[k]), 1e-10)
    if consistent:
        assert got["rhs_p"][0] == 0.0
        for f in (got["mdot"], got["mdot_star"]):                                         # walls: exactly 0.0
            for wall in _walls(f, nx, ny):
                assert not wall.any()
        b = got["rhs_p"].reshape(ny, nx).copy()
        b.flat[0] = -np.sum(b.ravel()[1:])
        A = ref["A"]
        o = P.restatement("laplacian", nx, ny, m["Re"], grid_stretch=m["beta"], **P.phase_geometry(m))      # (for apply)
        xs = np.zeros(nx * ny)
        xs[1:] = np.linalg.solve(A[1:, 1:], b.ravel()[1:])
        x = got["y"]
        xm, xsm = x - x.mean(), xs - xs.mean()
        err = float(np.linalg.norm(xm - xsm))
        bound = tol * np.linalg.norm(b) / ref["lam1"] + 64 * EPS * np.linalg.norm(xsm)
        devs["p_prime"] = (err, float(bound))
        far = float(np.linalg.norm(xm - (ref["xs"].ravel() - ref["xs"].mean())))
        print(f"EDGE phases {tag} {kernel}: CG {c['pressure_last']} iterations, |x - x*| {err:.2e} (x* of the restatement's b: "
              f"{far:.2e}), bound {bound:.2e}")
        assert c["pressure_caps"] == 0 and c["pressure_solves"] == 1 and c["pressure_last"] >= 1
        r_true = b - o.apply(ref["wx"], ref["wy"], x.reshape(ny, nx))
        ratio = float(np.linalg.norm(r_true) / (tol * np.linalg.norm(b)))
        rec = float(np.linalg.norm(got["cg_r"]) / (tol * np.linalg.norm(b)))
        print(f"EDGE phases {tag} {kernel}: |b - A y| / (pressure_tol |b|) {ratio:.3f}, the recurrence's |r| likewise {rec:.3f}")
        assert rec <= 1.0 + 4 * nx * ny * EPS            # the stop test itself, the norms summed in another order
        if kernel == "separable":
            devs["sep_s"] = (_rel(got["sep_s"], ref["s"]), 1e-12)
            devs["true_residual"] = (ratio, 2.0)         # pressure_tol |b| and a factor of 2 for residual drift
    else:
        devs["p_prime"] = (_rel(got["p_prime"], cap["p_prime"]), 1e-8)
        total_abs = float(np.sum(np.abs(got["rhs_p"])))
        devs["b00"] = (abs(got["b00"] + float(np.sum(got["rhs_p"][1:]))), 64 * EPS * total_abs)
    for k in ("u_prime", "v_prime", "mdot"):
        devs[k] = (_rel(got[k], cap[k]), 1e-9)
    devs["omega"] = (_rel(got["omega"], ref["omega"]), 1e-9)
    cols = CONSISTENT_COLS if consistent else list(range(7))
    devs["row"] = (_rows_rel(got["row"][cols], ref["row"][cols]), 1e-9)
    devs["row_div"] = (abs(got["row"][3] - ref["row"][3]) / float(np.max(np.abs(cap["mdot"]))), 1e-9)
    for k in ("u", "v", "p"):
        devs[k] = (_rel(st[k], ref["state"][k]), 1e-9)
    print(f"EDGE phases {tag} {kernel} ({dt * 1e3:.1f} ms): " + ", ".join(f"{k} {v:.2e}/{b_:.0e}" for k, (v, b_) in devs.items()))
    for k, (v, bound) in devs.items():                   # dicts keep the order: the first failure names the phase
        assert v <= bound, (tag, kernel, k, v, bound)
    rows, _, total = s._advance(P.PHASE_MORE)
    assert total == 1 + P.PHASE_MORE
    _assert_trajectory(f"phases+{P.PHASE_MORE} {tag} {kernel}",
                       _trajectory_devs(rows, s.state(), ref["rows"], ref["state_after"], kernel), 1e-9)
    assert s.counters()["linear_giveups"] == 0
    s.close()


# ------------------------------------------------------------------------------------------- b. edge shapes
@pytest.mark.parametrize("kernel", P.KERNELS)
@pytest.mark.parametrize("shape", P.SHAPES, ids=P.SHAPE_IDS)
def test_tvd_trajectories_match_the_restatement_at_edge_shapes(fv, shape, kernel):
    """TVD from rest, Re 400, linear_solver_tol 1e-12, pressure_tol 1e-13, against the restatement with the same pressure solve
    (CG with the kernel's preconditioner; the exact solve in reference mode): 37 x 50 and 24 x 40 (several strides; beta 2.5),
    131 x 77, 255 x 253 (partial tiles and K-remainders of every GEMM), MIN_N beside MAX_N both ways, MAX_N on both axes.
    Fields and record columns to 1e-9, |div mdot| against max |mdot|; K pressure solves, none capped, no BiCGSTAB give-up."""
    nx, ny, beta, geo, K = shape
    ref = P.shape_reference(*shape, kernel)
    s = fv[0](**P.shape_solver_kwargs(*shape, kernel))
    t0 = time.perf_counter()
    s.solve()
    dt = time.perf_counter() - t0
    c = s.counters()
    print(f"EDGE shape {nx}x{ny} beta {beta} {kernel}: {dt:.2f} s for {K} iterations, {c}")
    _assert_trajectory(f"shape {nx}x{ny} beta {beta} {kernel}", _trajectory_devs(s.history, s.state(), ref["rows"], ref["state"], kernel),
                       1e-9)
    assert c["iterations"] == K and c["nan"] == 0 and c["linear_giveups"] == 0 and c["momentum_solves"] == 2 * K
    if kernel != "reference":
        assert c["pressure_caps"] == 0 and c["pressure_solves"] == K
        for wall in _walls(s.state()["mdot"], nx, ny):
            assert not wall.any()
    s.close()


# ------------------------------------------------------------------------------------------- c. CG counts at an edge
@pytest.mark.parametrize("kernel", ["separable", "laplacian"])
def test_cg_counts_follow_the_restatement_at_beta_2_5(fv, kernel):
    """24 x 40, beta 2.5 (the case of the list above), one iteration per launch so that every solve's count is read.  The
    restatement takes about 28 iterations per solve with the separable preconditioner and 410 to 470 with the laplacian one.
    Separable: each count within one of the restatement's, the rule of
    tests/test_gpu_fv_separable.py::test_cg_counts_follow_the_restatement_and_halve_the_laplacian_ones (measured: 1 in one
    solve of twelve).  Laplacian: that rule does not hold, on either side: 460 CG iterations on 960 unknowns lose conjugacy to
    rounding, and the restatement's own counts move by up to 2 per solve when its linear_solver_tol goes from 1e-12 to 1e-13
    (and by up to 3 at 1e-11), with every field unchanged to 1e-14.  The card is 3 away in one solve, 1 in another, 0 in ten
    (1.5 times the restatement's figure); ten times that figure, 20, is allowed (fv_stretched_probe.count_bound; the fields
    of this very run are held to 1e-9 by the shape test above)."""
    K = P.COUNTS[4]
    ref = P.counts_reference(kernel)
    s = fv[0](**P.counts_solver_kwargs(kernel))
    s._begin(1e-30)
    per_solve = []
    for _ in range(K):
        s._advance(1)
        per_solve.append(s.counters()["pressure_last"])
    c = s.counters()
    worst = max(abs(a - b) for a, b in zip(per_solve, ref["cg_iters"]))
    print(f"EDGE counts {kernel}: card {per_solve}\nEDGE counts {kernel}: restatement {list(ref['cg_iters'])}, worst {worst}, "
          f"bound {P.count_bound(kernel)}")
    assert c["pressure_caps"] == 0 and c["pressure_solves"] == K and c["pressure_iterations"] == sum(per_solve)
    assert worst <= P.count_bound(kernel)
    assert abs(c["pressure_iterations"] - sum(ref["cg_iters"])) <= K * P.count_bound(kernel)
    s.close()


# ------------------------------------------------------------------------------------------- d. capped pressure solves
@pytest.mark.parametrize("kernel", ["laplacian", "separable"])
def test_capped_pressure_solves_are_counted_and_accepted(fv, kernel):
    """pressure_max_iters = 3 at pressure_tol 1e-10: every one of the 30 solves ends at the cap and its iterate is accepted.
    Both sides do the same three iterations, so the trajectory agrees to 1e-9."""
    K = P.SMALL["K"]
    ref = P.capped_cg_reference(kernel)
    s = fv[0](**P.small_solver_kwargs(kernel, **P.CAPPED_CG))
    s.solve()
    c = s.counters()
    print(f"EDGE capped-cg {kernel}: {c}")
    assert c["pressure_caps"] == K == ref["cg_caps"] and c["pressure_iterations"] == 90 and c["pressure_last"] == 3
    assert c["pressure_solves"] == K and c["nan"] == 0 and c["iterations"] == K
    _assert_trajectory(f"capped-cg {kernel}", _trajectory_devs(s.history, s.state(), ref["rows"], ref["state"], kernel), 1e-9)
    s.close()


# ------------------------------------------------------------------------------------------- e. BiCGSTAB exits
@pytest.mark.parametrize("kernel", P.KERNELS)
def test_capped_linear_solves_are_counted_and_accepted(fv, monkeypatch, kernel):
    """max_lin_iters = 3, as tests/test_gpu_fv_edges.py::test_capped_linear_solves_are_counted_and_accepted: 59 solves give
    up, the first v solve has b = 0, 177 iterations; the counters are the restatement's and the trajectory agrees to 1e-9."""
    import solvers.fv.solver as S
    monkeypatch.setattr(S, "LINEAR_MAX_ITERATIONS", P.CAPPED_LINEAR["max_lin_iters"])
    K = P.SMALL["K"]
    ref = P.capped_linear_reference(kernel)
    s = fv[0](**P.small_solver_kwargs(kernel, linear_solver_tol=P.CAPPED_LINEAR["linear_solver_tol"],
                                      pressure_tol=P.CAPPED_LINEAR["pressure_tol"]))
    s.solve()
    c = s.counters()
    print(f"EDGE capped-bicgstab {kernel}: {c}")
    assert c["linear_giveups"] == ref["exits"].count("cap") == 59
    assert c["linear_iterations"] == sum(ref["iters"]) == 177
    assert c["momentum_solves"] == 2 * K
    if kernel != "reference":
        assert c["pressure_caps"] == 0 and c["pressure_solves"] == K
    _assert_trajectory(f"capped-bicgstab {kernel}", _trajectory_devs(s.history, s.state(), ref["rows"], ref["state"], kernel),
                       1e-9)
    s.close()


@pytest.mark.parametrize("kernel", P.KERNELS)
def test_loose_linear_solves_with_unequal_u_v_counts(fv, kernel):
    """linear_solver_tol 1e-6 at 30 x 21, Re 400, beta 1: solves end on |r| and on |s|, and u and v leave the shared loop at
    different iterations in 16 or 17 of the 40 iterations (the restatement).  Counters within 2 K, fields to 1e-8, as
    tests/test_gpu_fv_edges.py::test_both_bicgstab_exits_and_unequal_u_v_counts."""
    K = P.LOOSE["K"]
    ref = P.loose_reference(kernel)
    s = fv[0](**P.small_solver_kwargs(kernel, case=P.LOOSE, linear_solver_tol=P.LOOSE["linear_solver_tol"],
                                      pressure_tol=P.LOOSE["pressure_tol"]))
    s.solve()
    c = s.counters()
    print(f"EDGE loose {kernel}: linear iterations {c['linear_iterations']}, restatement {sum(ref['iters'])}")
    assert c["linear_giveups"] == 0 and c["momentum_solves"] == 2 * K
    assert abs(c["linear_iterations"] - sum(ref["iters"])) <= 2 * K          # rounding may move a stopping test by one
    _assert_trajectory(f"loose {kernel}", _trajectory_devs(s.history, s.state(), ref["rows"], ref["state"], kernel), 1e-8)
    s.close()


# ------------------------------------------------------------------------------------------- f. the NaN latch
@pytest.mark.parametrize("kernel", P.KERNELS)
def test_a_lone_nan_trial_raises(fv, kernel):
    """16 x 16, beta 1.5, Re 1000 without under-relaxation: the restatement's first non-finite record row is row 10 (consistent)
    or 11 (reference), counted from 0; each kernel's NaN latch stops the trial within its first chunk.  The card latched one
    row earlier (10 and 11 iterations counted, the last one the NaN row): by then max |u| is 1e102 ... 1e146 and the BiCGSTAB
    solves run to their cap of 1000, so the row of the overflow is rounding's to choose and is not asserted."""
    from solvers.spectral.ldc_lib import LdcError
    kw = P.nan_solver_kwargs(kernel)
    s = fv[0](**kw)
    with pytest.raises(LdcError, match="NaN"):
        s.solve()
    c = s.counters()
    print(f"EDGE nan {kernel}: {c} (restatement: iteration {P.NAN_AT[kernel]})")
    assert c["nan"] == 1 and c["done"] == 0 and c["iterations"] < kw["check_every"]
    s.close()


def test_nan_trials_of_all_three_kernels_leave_a_healthy_neighbour_alone(fv):
    """The same three trials in one BatchedFVSolver beside a healthy separable trial (16 x 16, Re 100, 60 iterations): three
    stored errors, and the healthy trial is bit-equal to its lone run."""
    FVSolver, BatchedFVSolver = fv
    from solvers.spectral.ldc_lib import LdcError
    healthy = dict(name="fv", nx=16, ny=16, Re=100.0, convection_scheme="TVD", alpha_uv=0.4, alpha_p=0.2,
                   linear_solver_tol=1e-9, grid_stretch=1.5, tolerance=1e-30, max_iterations=60, check_every=256, **P.SEP)
    trials = [P.nan_solver_kwargs(k) for k in P.KERNELS[:2]] + [healthy, P.nan_solver_kwargs(P.KERNELS[2])]
    batch = BatchedFVSolver(trials)
    batch.solve()
    assert sorted(batch.errors) == [0, 1, 3], batch.errors
    for q in (0, 1, 3):
        assert isinstance(batch.errors[q], LdcError) and "NaN" in str(batch.errors[q])
        assert batch.solvers[q].counters()["nan"] == 1
    lone = FVSolver(**healthy)
    lone.solve()
    assert lone.metrics.iterations == 60 and lone.counters()["nan"] == 0
    _assert_same_bits(batch.solvers[2], lone, "healthy")
    lone.close()
    batch.close()


# ------------------------------------------------------------------------------------------- g. more than one launch
def test_more_handles_than_one_launch_takes_of_every_kind(fv):
    """LAUNCH_MAX + 2 handles of each kernel in ONE ldc_fv_batch_enqueue, interleaved: ldc_fv_stretched_launch (twice) and
    ldc_fv_stretched_sep_launch each cut their group into 256 + 2.  8 x 8, beta 1.5, 0.05 / 0.05, Re 100 ... 1000 (the case of
    tests/test_gpu_fv_batched.py::test_more_trials_than_one_launch_takes), 20 iterations: every handle reports 20 and no NaN;
    handles 0, 255, 256 and 257 of each group are bit-equal to lone runs."""
    import torch
    from solvers.fv import ldc_fv_lib as F
    FVSolver, _ = fv
    assert P.LAUNCH_MAX == F.LAUNCH_MAX
    K, n = P.LAUNCH_K, P.LAUNCH_N
    groups = {kernel: [FVSolver(**P.launch_solver_kwargs(kernel, q)) for q in range(n)] for kernel in P.KERNELS}
    handles = []
    for q in range(n):
        for kernel in P.KERNELS:
            s = groups[kernel][q]
            s._begin(1e-30)
            handles.append(s.handle)
    assert len(handles) == 3 * n
    F.batch_enqueue(handles, K, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for kernel, ss in groups.items():
        ctrl = torch.stack([s.t["ctrl"] for s in ss]).cpu().numpy()
        assert np.all(ctrl[:, F.CTRL_ITER] == K) and not ctrl[:, F.CTRL_NAN].any(), kernel
        for q in P.LAUNCH_CHECKED:
            lone = FVSolver(**P.launch_solver_kwargs(kernel, q))
            lone._begin(1e-30)
            rows = lone._advance(K)[0]
            assert rows.shape == (K, 8) and np.all(np.isfinite(rows[:, :7]))
            assert np.array_equal(ss[q].t["rec"][:K].cpu().numpy(), rows), (kernel, q)
            a, b = ss[q].state(), lone.state()
            for k in FIELDS:
                assert np.array_equal(a[k], b[k]), (kernel, q, k)
            assert ss[q].counters() == lone.counters(), (kernel, q)
            lone.close()
        for s in ss:
            s.close()


# ------------------------------------------------------------------------------------------- h. repeats and chunks
@pytest.mark.parametrize("kernel", P.STRIDES_KERNELS)
def test_a_repeat_solve_at_four_strides_is_bit_equal(fv, kernel):
    """tests/test_gpu_fv_separable.py::test_a_repeat_solve_on_one_handle_is_bit_equal at 37 x 50: two solves from rest on ONE
    handle and a third in other chunks leave the same bits."""
    s = fv[0](**P.strides_solver_kwargs(kernel))
    runs = []
    for chunks in ((24,), (24,), (7, 1, 16)):
        z = np.zeros(s.n_cells)
        s.set_state(z, z, z, np.zeros(s.t["mdot"].numel()))
        s._begin(1e-30)
        rows = np.concatenate([s._advance(k)[0] for k in chunks], axis=0)
        runs.append((rows, s.state(), s.counters()))
    assert runs[0][0].shape == (24, 8) and np.all(np.isfinite(runs[0][0][:, :7])) and runs[0][2]["iterations"] == 24
    for rows, st, c in runs[1:]:
        assert np.array_equal(rows, runs[0][0]) and c == runs[0][2]
        for k in FIELDS:
            assert np.array_equal(st[k], runs[0][1][k]), k
    s.close()


@pytest.mark.parametrize("kernel", P.STRIDES_KERNELS)
def test_chunk_length_changes_nothing_at_four_strides(fv, kernel):
    """tests/test_gpu_fv_edges.py::test_chunk_length_changes_nothing at 37 x 50: check_every 1, 7 and 64 over 24 iterations."""
    runs = []
    for every in (1, 7, 64):
        s = fv[0](**P.strides_solver_kwargs(kernel, check_every=every, max_iterations=24))
        s.solve()
        runs.append(s)
    assert runs[0].metrics.iterations == 24 and runs[0].history.shape == (24, 8)
    for every, s in zip((7, 64), runs[1:]):
        _assert_same_bits(s, runs[0], f"check_every={every}")
    for s in runs:
        s.close()
