"""Batches of equal-N trials on the chip-wide trial kernel (ldc_batch_mode 5, N = 81 ... 256): launch groups of
floor(CUs / T^2) trials, T x T work-groups each, one per CU.

Judged like the other batch forms (tests/test_gpu_batched.py): every trial of a batch equals, bit for bit, the same trial
run alone on the same kernel in the same layout; and against the reference (g4c) and the oracle."""
import numpy as np
import pytest

from oracle import ldc_oracle as orc
from test_gpu_parity import check_g4c
from test_gpu_xcd import oracle_rows, rel

pytestmark = pytest.mark.gpu


def kw(N, Re, cs=0.15, **extra):
    d = dict(name="spectral", Re=float(Re), lid_velocity=1.0, Lx=1.0, Ly=1.0, nx=N, ny=N, tolerance=1e-6,
             max_iterations=10_000_000, basis_type="chebyshev", CFL=1.5, beta_squared=5.0,
             corner_treatment="smoothing", corner_smoothing=cs, multigrid="none", check_every=512, graph_iters=16,
             persistent=5)
    d.update(extra)
    return d


def batch_mode(b):
    from solvers.spectral import ldc_lib as L
    return int(L.lib().ldc_batch_mode(b._batch))


def per_launch(N, sp=0):
    import ctypes as C
    from solvers.spectral import ldc_lib as L
    cus, xcds = C.c_int(), C.c_int()
    L.check(L.lib().ldc_device_info(C.byref(cus), C.byref(xcds)), "ldc_device_info")
    return int(L.lib().ldc_wide_trials_per_launch(N, N, sp, cus.value))


RES = [100, 400, 1000, 250, 700, 150, 550]
CSS = [0.15, 0.10, 0.30, 0.05, 0.20, 0.12, 0.25]


def test_batch_mode_5_is_chosen_by_the_batch_rule(monkeypatch):
    """Every trial asking for persistent=5 gives mode 5; so does auto mode with LDC_BATCH_WIDE=1.  Without the knob an
    auto-mode batch stays on the launch path, and a batch that mixes 5 and -1 is not mode 5."""
    from solvers.spectral.batched import BatchedSGSolver
    monkeypatch.delenv("LDC_BATCH_WIDE", raising=False)
    monkeypatch.delenv("LDC_WIDE_LAYOUT", raising=False)

    def mode(trials):
        b = BatchedSGSolver(trials)
        b._ensure_batch([0.0] * len(trials))
        m = (b.kernel_mode, batch_mode(b), [s.kernel_mode for s in b.solvers])
        b.close()
        return m

    asked = [kw(96, Re, cs) for Re, cs in zip(RES[:3], CSS[:3])]
    auto = [dict(t, persistent=-1) for t in asked]
    assert mode(asked) == (5, 5, [5, 5, 5])
    assert mode(auto) == (0, 0, [0, 0, 0])
    monkeypatch.setenv("LDC_WIDE_LAYOUT", "tail")             # batches run the tiles layout only
    assert mode(asked) == (0, 0, [0, 0, 0])
    monkeypatch.delenv("LDC_WIDE_LAYOUT")
    assert mode([kw(256, Re, cs) for Re, cs in zip(RES[:2], CSS[:2])])[0] == 0
    assert mode([asked[0], auto[1], asked[2]])[0] != 5
    monkeypatch.setenv("LDC_BATCH_WIDE", "1")
    assert mode(auto) == (5, 5, [5, 5, 5])
    assert mode([asked[0], auto[1], asked[2]])[0] != 5


CASES = [(96, "tiles", 7), (128, "tiles", 4), (160, "tiles", 4), (176, "tiles", 2)]


@pytest.mark.parametrize("N,layout,B", CASES)
def test_wide_batch_equals_lone_runs_bit_for_bit(monkeypatch, N, layout, B):
    """Distinct Re and corner_smoothing per trial, diagnostics on, 300 iterations; at least two launch groups where the size
    allows several trials per launch.  Each trial's records and final u, v, p equal (==) the same trial alone on mode 5."""
    from solvers.spectral.batched import BatchedSGSolver
    from solvers.spectral.sg import SGSolver
    monkeypatch.setenv("LDC_WIDE_LAYOUT", layout)
    G = per_launch(N)
    assert G >= 1 and (G == 1 or B > G)
    trials = [kw(N, Re, cs) for Re, cs in zip(RES[:B], CSS[:B])]
    b = BatchedSGSolver(trials)
    recs = b.run_iterations(300)
    assert batch_mode(b) == 5 and b.kernel_mode == 5
    for t, s, r in zip(trials, b.solvers, recs):
        one = SGSolver(**t)
        r1 = one.run_iterations(300)
        assert one.kernel_mode == 5
        assert r.shape == (300, 8) and np.all(np.isfinite(r))
        assert np.array_equal(r, r1), t["Re"]
        assert np.array_equal(s.arrays.u, one.arrays.u) and np.array_equal(s.arrays.v, one.arrays.v)
        assert np.array_equal(s.arrays.p, one.arrays.p)
        one.close()
    b.close()


@pytest.mark.parametrize("K", [40, 400])
def test_wide_batch_trial_vs_reference(golden_dir, monkeypatch, K):
    """The middle trial of a 3-trial N=128 batch is the reference's g4c run (Re=1000)."""
    from solvers.spectral.batched import BatchedSGSolver
    monkeypatch.delenv("LDC_WIDE_LAYOUT", raising=False)
    g = np.load(golden_dir / f"g4c_traj_N128_Re1000_K{K}.npz")
    b = BatchedSGSolver([kw(128, 400, 0.10), kw(128, 1000, 0.15), kw(128, 250, 0.30)])
    recs = b.run_iterations(K)
    assert b.kernel_mode == 5
    assert recs[1].shape == (K, 8)
    check_g4c(g, b.solvers[1], recs[1], 128)
    b.close()


def test_wide_batch_latches_each_trial_independently(monkeypatch):
    """Different caps and tolerances: each trial stops on its own (the host latches a capped trial with code 3, a converged
    one latches on the device), the others keep iterating in the same launches, and a latched trial's state stays what
    it was at its stop -- each equals its stand-alone solve."""
    from solvers.spectral.batched import BatchedSGSolver
    from solvers.spectral.sg import SGSolver
    monkeypatch.delenv("LDC_WIDE_LAYOUT", raising=False)
    trials = [kw(96, 100, max_iterations=150, check_every=256), kw(96, 100, 0.10, max_iterations=700, check_every=256),
              kw(96, 400, 0.30, max_iterations=333, check_every=256),
              kw(96, 100, 0.05, tolerance=1e-2, max_iterations=5000, check_every=256),
              kw(96, 250, 0.20, tolerance=3e-3, max_iterations=5000, check_every=256)]
    b = BatchedSGSolver(trials)
    ms = b.solve()
    assert b.kernel_mode == 5
    assert [m.iterations for m in ms[:3]] == [150, 700, 333] and not any(m.converged for m in ms[:3])
    its = []
    for t, s, m in zip(trials, b.solvers, ms):
        one = SGSolver(**t)
        one.solve()
        assert (m.iterations, m.converged) == (one.metrics.iterations, one.metrics.converged)
        assert np.array_equal(s.fields.u, one.fields.u) and np.array_equal(s.fields.p, one.fields.p)
        assert s.time_series.energy == one.time_series.energy
        its.append(m.iterations)
        one.close()
    assert ms[3].converged and ms[3].iterations < 5000 and len(set(its[:4])) == 4
    b.close()


def test_wide_batch_fsg_config5_shape(monkeypatch):
    """BASELINE config 5: eight FSG trials at N=128 (levels 64 -> 128, 150 iterations per level) as one batch with
    LDC_BATCH_WIDE=1.  The fine level (the smoother on 9 x 9 tiles, 3 trials per launch) runs on mode 5, the coarse level
    keeps the one-XCD kernel; trials 0 and 7 against the oracle's FSG sequence, every trial against its lone FSG solve."""
    from solvers.spectral import batched
    from solvers.spectral.fsg import FSGSolver
    monkeypatch.setenv("LDC_BATCH_WIDE", "1")
    monkeypatch.delenv("LDC_WIDE_LAYOUT", raising=False)
    modes = []
    ensure = batched.BatchedSGSolver._ensure_batch

    def spy(self, tolerances):
        ensure(self, tolerances)
        modes.append((self.solvers[0].M - 1, self.kernel_mode))
    monkeypatch.setattr(batched.BatchedSGSolver, "_ensure_batch", spy)
    cs = [0.02 + 0.011 * q for q in range(8)]
    base = dict(name="spectral_fsg", Re=1000.0, lid_velocity=1.0, Lx=1.0, Ly=1.0, nx=128, ny=128, tolerance=1e-6,
                max_iterations=150, basis_type="chebyshev", CFL=1.5, beta_squared=5.0, corner_treatment="smoothing",
                multigrid="fsg", n_levels=2, coarse_tolerance_factor=1.0, prolongation_method="fft",
                restriction_method="fft", check_every=64, graph_iters=16)
    trials = [dict(base, corner_smoothing=c) for c in cs]
    b = batched.BatchedFSGSolver(trials)
    assert b.orders == [64, 128]
    b.solve()
    assert {m for n, m in modes if n == 128} == {5} and {m for n, m in modes if n == 64} == {3}
    for q in (0, 7):
        lvl, total, conv = orc.oracle_fsg(128, 1000.0, max_iterations=150, corner_smoothing=cs[q])
        s = b.solvers[q]
        assert s.metrics.iterations == total == 300 and s.metrics.converged == conv
        assert np.max(np.abs(s.arrays.u.reshape(129, 129) - lvl.u)) < 1e-10
        assert np.max(np.abs(s.arrays.v.reshape(129, 129) - lvl.v)) < 1e-10
        assert np.max(np.abs(s.arrays.p.reshape(127, 127) - lvl.p)) < 1e-10
    monkeypatch.setattr(batched.BatchedSGSolver, "_ensure_batch", ensure)
    for t, s in zip(trials, b.solvers):
        one = FSGSolver(**t)
        one.solve()
        assert one.metrics.iterations == s.metrics.iterations
        assert np.array_equal(one.arrays.u, s.arrays.u) and np.array_equal(one.arrays.v, s.arrays.v)
        assert np.array_equal(one.arrays.p, s.arrays.p)
        one.close()
    b.close()


def test_wide_batch_and_launch_path_hand_the_state_to_each_other(monkeypatch):
    """A batch advanced on mode 5, then on the launch path (persistent=0: the batch is rebuilt), then on mode 5 again: the
    trial at Re=400 against the oracle, as a lone trial is in test_gpu_wide.py."""
    from solvers.spectral.batched import BatchedSGSolver
    monkeypatch.delenv("LDC_WIDE_LAYOUT", raising=False)
    N, Re = 128, 400.0
    b = BatchedSGSolver([kw(N, 1000, 0.10), kw(N, Re, 0.15), kw(N, 250, 0.30)])
    rows = [b.run_iterations(60)[1]]
    assert b.kernel_mode == 5
    for s in b.solvers:
        s.params.persistent = 0
    rows.append(b.run_iterations(21)[1])
    assert b.kernel_mode == 0
    for s in b.solvers:
        s.params.persistent = 5
    rows.append(b.run_iterations(40)[1])
    assert b.kernel_mode == 5
    for s in b.solvers:
        s.params.persistent = 0
    rows.append(b.run_iterations(1)[1])
    rec = np.concatenate(rows, axis=0)
    o = orc.OracleSG(N, Re)
    want = oracle_rows(o, 122)
    s = b.solvers[1]
    assert rec.shape == (122, 8)
    assert np.max(np.abs(s.arrays.u.reshape(N + 1, N + 1) - o.u)) < 1e-12
    assert np.max(np.abs(s.arrays.p.reshape(N - 1, N - 1) - o.p)) < 1e-12
    assert rel(rec[:, 7], want[:, 7]) < 1e-12
    for c in range(1, 7):
        assert rel(rec[:, c], want[:, c]) < (1e-10 if c < 5 else 1e-9), c
    b.close()
