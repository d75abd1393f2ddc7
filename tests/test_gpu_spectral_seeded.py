"""Every mapping of the spectral RK kernels from a seeded, developed state (tests/spectral_seed.py): the launch path (mode 0),
the one-XCD kernel (3), the trial-per-CU kernel (4), the chip-wide kernel (5) in both layouts, the smoother loop, unequal
grids in both orientations, non-default parameters, the four batch forms and a hand-over between kernels.

The from-rest tests of these kernels run where the flow sits under the lid: away from it the quadratic terms are below
the state tolerance, and a kernel that drops them there passes (tests/test_spectral_seeded_cpu.py pins that, and shows
for every case below that the oracle's own rounding floor is a hundredth of the tolerances used here and that each of six
arithmetic faults moves the state by a hundred times them).  Here every tile holds O(1) data from the first residual on.

Tolerances: the suite's own (tests/test_gpu_parity.py) -- state <= 1e-12 absolute, dt <= 1e-12 relative, the relative
change as in test_short_run_records_vs_oracle, norms and E <= 1e-10, Z and P <= 1e-9 relative.  K = 4: in the host's tail
layout the first iteration after an upload runs alone on the launch path, the persistent kernel runs the other three.
"""
import ctypes as C

import numpy as np
import pytest

from spectral_seed import BATCHES, CASES, HANDOVER, RAW_CASES, RAW_REFUSED, oracle_rows
from test_gpu_xcd import rel

pytestmark = pytest.mark.gpu


def device_cus():
    from solvers.spectral import ldc_lib as L
    cus, xcds = C.c_int(), C.c_int()
    L.check(L.lib().ldc_device_info(C.byref(cus), C.byref(xcds)), "ldc_device_info")
    return cus.value, xcds.value


def layout_or_skip(monkeypatch, c):
    """LDC_WIDE_LAYOUT as the case asks; skip only where the device has too few CUs for the case's tiles."""
    if c.layout is None:
        monkeypatch.delenv("LDC_WIDE_LAYOUT", raising=False)
    else:
        monkeypatch.setenv("LDC_WIDE_LAYOUT", c.layout)
    if c.mode == 5:
        M = max(c.N, c.N if c.ny is None else c.ny) + 1
        T = (M - 1) // 16 if c.layout == "tail" else (M + 15) // 16
        cus, _ = device_cus()
        if T * T > cus:
            pytest.skip(f"{T} x {T} tiles do not fit {cus} CUs")


def compare(tag, s, rec, o, want, K, diagnostics):
    """State and records of solver ``s`` against oracle ``o`` (already advanced: ``want`` are its K rows); prints every
    figure before it asserts."""
    assert rec.shape == (K, 8)
    u = s.arrays.u.reshape(o.M, o.My)
    v = s.arrays.v.reshape(o.M, o.My)
    p = s.arrays.p.reshape(o.M - 2, o.My - 2)
    du, dv, dp = np.max(np.abs(u - o.u)), np.max(np.abs(v - o.v)), np.max(np.abs(p - o.p))
    d0 = np.max(np.abs(rec[:, 0] - want[:, 0]) / (np.abs(want[:, 0]) + 1e-9))
    cols = [rel(rec[:, c], want[:, c]) for c in range(1, 8)]
    print(f"SEEDED {tag}: u {du:.2e} v {dv:.2e} p {dp:.2e} | rel {d0:.2e} " +
          " ".join(f"{n} {e:.2e}" for n, e in zip(("Ru", "Rv", "Rp", "E", "Z", "P", "dt"), cols)))
    assert np.all(np.isfinite(rec))
    assert du < 1e-12 and dv < 1e-12 and dp < 1e-12, (tag, du, dv, dp)
    assert cols[6] < 1e-12, (tag, "dt", cols[6])
    assert d0 < 1e-8, (tag, "rel", d0)
    for c in range(1, 5):
        assert cols[c - 1] < 1e-10, (tag, c, cols[c - 1])
    if diagnostics:
        assert cols[4] < 1e-9 and cols[5] < 1e-9, (tag, cols[4], cols[5])
    else:
        assert not rec[:, 5:7].any()


def seeded_solver(c):
    from solvers.spectral.sg import SGSolver
    o, (u, v, p) = c.oracle()
    s = SGSolver(**c.solver_kw())
    if c.smoother:
        s._smoother_mode()
    s.set_state(u, v, p)
    return o, s


def mode_of(s):
    from solvers.spectral import ldc_lib as L
    return int(L.lib().ldc_solver_mode(s._handle))


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.id)
def test_seeded_run_vs_oracle(monkeypatch, c):
    layout_or_skip(monkeypatch, c)
    o, s = seeded_solver(c)
    rec = s.run_iterations(c.K, diagnostics=c.diagnostics)
    assert mode_of(s) == c.mode and s.kernel_mode == c.mode
    want = oracle_rows(o, c.K, c.diagnostics)
    compare(c.id, s, rec, o, want, c.K, c.diagnostics)
    s.close()


@pytest.mark.parametrize("c", RAW_CASES, ids=lambda c: c.id)
def test_seed_that_breaks_the_boundary_conditions(monkeypatch, c):
    """u and v nonzero on all four edges, index M-1 inside the tiles.  The oracle takes the first residual from the state as
    uploaded and imposes the boundary values on every stage; so must every kernel."""
    layout_or_skip(monkeypatch, c)
    o, s = seeded_solver(c)
    assert not s.tail
    assert np.abs(o.u[0, :]).max() > 0.01 and np.abs(o.v[:, -1]).max() > 0.01 and np.abs(o.v[-1, :]).max() > 0.01
    rec = s.run_iterations(c.K)
    assert mode_of(s) == c.mode and s.kernel_mode == c.mode
    want = oracle_rows(o, c.K)
    compare(c.id, s, rec, o, want, c.K, True)
    s.close()


@pytest.mark.parametrize("c", RAW_REFUSED, ids=lambda c: c.id)
def test_seed_that_breaks_the_boundary_conditions_is_refused_in_the_tail_layout(monkeypatch, c):
    """N = 16 T: no tile rewrites index M-1, and every kernel takes that row / column of phi^n for boundary values that never
    change (include/ldc_hip.h, ldc_problem::U).  From a state that holds anything else there the end state, dt and the residual
    norms still came out right, but the first record did not (measured before the refusal, N = 16 / N = 96: relative change
    off by 0.31 / 0.52, E by 1.1e-3 / 3.6e-5, Z by 0.35 / 0.64, P by 0.41 / 0.23): iterating from it is refused, one
    residual evaluation of it is not, and the same seed with its boundary values imposed runs."""
    layout_or_skip(monkeypatch, c)
    o, s = seeded_solver(c)
    assert s.tail
    with pytest.raises(ValueError, match="boundary values"):
        s.run_iterations(c.K)
    # the first residual of the raw state, rows / columns of index M-1 included, within the rounding bound of
    # test_gpu_parity.test_single_residual_vs_oracle: 24 eps |A| |B| term by term (D2 has entries ~ N^4 / 10 that cancel)
    Ru, Rv, Rp = o.residual(o.u, o.v, o.p)
    got = s.residual_fields()
    A, nu, eps = np.abs, 1.0 / o.Re, np.finfo(float).eps
    Dx, Dy, D2x, D2y = A(o.ax.D), A(o.ay.D), A(o.ax.D2), A(o.ay.D2)
    pf = A(o.ax.I) @ A(o.p) @ A(o.ay.I).T
    bu = A(o.u) * (Dx @ A(o.u)) + A(o.v) * (A(o.u) @ Dy.T) + Dx @ pf + nu * (D2x @ A(o.u) + A(o.u) @ D2y.T)
    bv = A(o.u) * (Dx @ A(o.v)) + A(o.v) * (A(o.v) @ Dy.T) + pf @ Dy.T + nu * (D2x @ A(o.v) + A(o.v) @ D2y.T)
    eu, ev = A(got["R_u"] - Ru.ravel()), A(got["R_v"] - Rv.ravel())
    print(f"SEEDED {c.id} first residual: R_u {eu.max():.2e} R_v {ev.max():.2e}, largest error / bound "
          f"{max((eu / (24 * eps * bu.ravel())).max(), (ev / (24 * eps * bv.ravel())).max()):.2f}")
    assert np.all(eu <= 24 * eps * bu.ravel()) and np.all(ev <= 24 * eps * bv.ravel())
    o.apply_bc(o.u, o.v)
    s.set_state(u=o.u, v=o.v)
    rec = s.run_iterations(c.K)
    assert mode_of(s) == c.mode
    compare(c.id, s, rec, o, oracle_rows(o, c.K), c.K, True)
    s.close()


@pytest.mark.parametrize("b", BATCHES, ids=lambda b: b.id)
def test_seeded_batch_every_trial_vs_its_own_oracle(monkeypatch, b):
    """Each trial has its own seed and its own Re: a trial that read a neighbour's operand would read other numbers."""
    from solvers.spectral import ldc_lib as L
    from solvers.spectral.batched import BatchedSGSolver
    layout_or_skip(monkeypatch, b.trial(0))
    trials = [b.trial(q) for q in range(b.B)]
    batch = BatchedSGSolver([dict(t.solver_kw(), tolerance=0.0) for t in trials])
    oracles = []
    for t, s in zip(trials, batch.solvers):
        o, (u, v, p) = t.oracle()
        s.set_state(u, v, p)
        oracles.append(o)
    recs = batch.run_iterations(b.K)
    assert int(L.lib().ldc_batch_mode(batch._batch)) == b.mode and batch.kernel_mode == b.mode
    for t, s, o, rec in zip(trials, batch.solvers, oracles, recs):
        compare(t.id, s, rec, o, oracle_rows(o, b.K), b.K, True)
    batch.close()


def test_seeded_hand_over_between_the_chip_wide_kernel_and_the_launch_path(monkeypatch):
    """3 iterations chip-wide, 2 on the launch path, 3 chip-wide again on one seeded N = 128 state: the state and all
    8 records against ONE oracle run of 8 iterations."""
    c = HANDOVER
    layout_or_skip(monkeypatch, c)
    o, s = seeded_solver(c)
    rows = []
    for mode, n in ((5, 3), (0, 2), (5, 3)):
        s.params.persistent = mode
        rows.append(s.run_iterations(n))
        assert mode_of(s) == mode and s.kernel_mode == mode
    rec = np.concatenate(rows, axis=0)
    compare(c.id, s, rec, o, oracle_rows(o, c.K), c.K, True)
    s.close()
