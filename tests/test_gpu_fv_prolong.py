"""Finite-volume prolongation on the GPU (ldc_fv_prolong_enqueue through ``solvers.fv.solver.prolong``) against the NumPy
restatement of tests/fv_prolong_numpy.py applied to the downloaded coarse state: every pair of sizes the kernel treats
differently, what it writes and what it leaves alone, batches against single launches, and the refusals."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import fv_prolong_numpy as P  # noqa: E402
from fv_numpy import FVState  # noqa: E402

pytestmark = pytest.mark.gpu

YAML = dict(name="fv", convection_scheme="TVD", alpha_uv=0.4, alpha_p=0.2, linear_solver_tol=1e-9)      # conf/solver/fv.yaml
# sizes that halve, odd and unequal ones, a ratio that is no integer, the same grid, and the largest pair there is (256
# is LDC_FV_MAX_N): 128 cells per thread and the longest offsets
PAIRS = [((8, 8), (16, 16)), ((12, 8), (25, 17)), ((16, 16), (37, 37)), ((32, 32), (32, 32)), ((128, 128), (256, 256))]
STATE = ("u", "v", "p", "mdot")


@pytest.fixture(scope="module")
def fv():
    import __graft_entry__ as g
    g.build()
    from solvers.fv import ldc_fv_lib as F
    from solvers.fv.solver import FVSolver, prolong
    return FVSolver, prolong, F


def _trial(FVSolver, size, lid="none", iters=0, Re=100.0):
    s = FVSolver(**dict(YAML, nx=size[0], ny=size[1], Re=Re, corner_treatment=lid, tolerance=1e-30, check_every=8))
    if iters:
        s._begin(1e-30)
        s._advance(iters)                         # a few iterations of a real solve: u, v, p and mdot all non-trivial
    return s


def _poison(s):
    s.set_state(*(np.full(s.t[k].numel(), np.nan) for k in STATE))


def _restated(coarse, fine):
    """The restatement applied to the coarse trial's downloaded state, in the layout of ``state()``."""
    c = FVState(coarse.nx, coarse.ny, 100.0)
    c.set_state(**coarse.state())
    c.ulid = coarse.t["ulid"].cpu().numpy()
    f = FVState(fine.nx, fine.ny, 100.0)
    P.prolong(c, f)
    return dict(u=f.u.ravel(), v=f.v.ravel(), p=f.p.ravel(), mdot=P.mdot(f))


def _untouched(s):
    return {k: s.t[k].cpu().numpy().copy() for k in ("ctrl", "rec", "work", "ulid")}


@pytest.mark.parametrize("lid", ["none", "saad"])
@pytest.mark.parametrize("coarse,fine", PAIRS)
def test_device_matches_the_restatement(fv, coarse, fine, lid):
    FVSolver, prolong, F = fv
    c, f = _trial(FVSolver, coarse, lid, iters=6), _trial(FVSolver, fine, lid, iters=3)
    _poison(f)
    f.t["ctrl"].copy_(c.t["ctrl"])                # (set_state zeroes the words: give the kernel something to spoil)
    before_c, before_f = dict(c.state(), **_untouched(c)), _untouched(f)
    assert all(np.max(np.abs(before_c[k])) > 0 for k in STATE) and np.any(before_f["ctrl"] != 0)
    prolong([(c, f)])
    got, want = f.state(), _restated(c, f)
    for k in STATE:
        scale = float(np.max(np.abs(want[k])))
        diff = float(np.max(np.abs(got[k] - want[k])))
        print(coarse, fine, lid, k, "max|field|", scale, "max|device - restatement|", diff)
        assert np.all(np.isfinite(got[k])) and diff <= 1e-13 * scale, k
    # exact zeros: the pinned cell and the fluxes through the four walls
    assert got["p"][0] == 0.0
    nx, ny = fine
    fx, fy = got["mdot"][: ny * (nx + 1)].reshape(ny, nx + 1), got["mdot"][ny * (nx + 1):].reshape(ny + 1, nx)
    for wall in (fx[:, 0], fx[:, -1], fy[0, :], fy[-1, :]):
        assert np.all(wall == 0.0) and not np.any(np.signbit(wall))
    # nothing else written: the coarse trial, and the fine trial's control words, record and work vectors
    after_c, after_f = dict(c.state(), **_untouched(c)), _untouched(f)
    for k in before_c:
        assert np.array_equal(before_c[k], after_c[k], equal_nan=True), ("coarse", k)
    for k in before_f:
        assert np.array_equal(before_f[k], after_f[k], equal_nan=True), ("fine", k)
    c.close(), f.close()


def test_the_lid_profile_reaches_the_row_under_the_lid(fv):
    """A coarse trial at rest: the only non-zero input is its lid profile, and it must show in the fine top row."""
    FVSolver, prolong, F = fv
    c, f = _trial(FVSolver, (8, 8), "saad"), _trial(FVSolver, (16, 16), "saad")
    _poison(f)
    prolong([(c, f)])
    got, want = f.state(), _restated(c, f)
    u = got["u"].reshape(16, 16)
    assert np.all(u[:-1] == 0.0) and np.all(u[-1, 1:-1] > 0) and np.array_equal(got["u"], want["u"])
    assert np.all(got["v"] == 0.0) and np.all(got["p"] == 0.0) and np.all(got["mdot"][16 * 17:] == 0.0)
    c.close(), f.close()


def test_one_launch_of_three_pairs_equals_three_launches(fv):
    FVSolver, prolong, F = fv
    sizes = [((8, 8), (16, 16)), ((12, 8), (25, 17)), ((16, 16), (37, 37))]
    pairs = [(_trial(FVSolver, c, "saad", iters=4 + q, Re=100.0 * (q + 1)), _trial(FVSolver, f)) for q, (c, f) in enumerate(sizes)]
    for _, f in pairs:
        _poison(f)
    prolong(pairs)
    together = [f.state() for _, f in pairs]
    for _, f in pairs:
        _poison(f)
    for pair in pairs:
        prolong([pair])
    for q, (_, f) in enumerate(pairs):
        alone = f.state()
        for k in STATE:
            assert np.all(np.isfinite(alone[k])) and np.array_equal(alone[k], together[q][k]), (q, k)
    for c, f in pairs:
        c.close(), f.close()


def test_more_pairs_than_a_launch_takes(fv):
    """260 fine trials from one coarse trial: one call, which the library cuts into launches of
    LDC_FV_PROLONG_LAUNCH_MAX; every fine trial, the last ones included, gets the same state."""
    FVSolver, prolong, F = fv
    n = F.LAUNCH_MAX + 4
    c = _trial(FVSolver, (8, 8), iters=5)
    fines = [_trial(FVSolver, (9, 10)) for _ in range(n)]
    for f in fines:
        _poison(f)
    prolong([(c, f) for f in fines])
    want = _restated(c, fines[0])
    for q in (0, 127, 128, 255, 256, n - 1):
        got = fines[q].state()
        for k in STATE:
            assert np.max(np.abs(got[k] - want[k])) <= 1e-13 * np.max(np.abs(want[k])), (q, k)
    first = fines[0].state()
    for f in fines[1:]:
        st = f.state()
        assert all(np.array_equal(st[k], first[k]) for k in STATE)
    c.close()
    for f in fines:
        f.close()


def test_refusals_come_back_without_a_launch(fv):
    FVSolver, prolong, F = fv
    L = F.lib()
    a, b, c = (_trial(FVSolver, (8, 8), iters=2), _trial(FVSolver, (12, 12), iters=2), _trial(FVSolver, (16, 16), iters=2))
    before = [s.state() for s in (a, b, c)]
    stream = C.c_void_p(a._stream())
    arr = lambda *hs: (C.c_void_p * len(hs))(*[h.value if h is not None else None for h in hs])        # noqa: E731
    assert L.ldc_fv_prolong_enqueue(arr(a.handle, None), arr(b.handle, c.handle), 2, stream) == -2      # a null handle
    assert L.ldc_fv_prolong_enqueue(arr(a.handle, a.handle), arr(b.handle, None), 2, stream) == -2
    assert L.ldc_fv_prolong_enqueue(arr(a.handle), arr(a.handle), 1, stream) == -1                      # onto itself
    assert L.ldc_fv_prolong_enqueue(arr(a.handle, a.handle), arr(b.handle, b.handle), 2, stream) == -1  # one fine trial twice
    assert L.ldc_fv_prolong_enqueue(arr(a.handle, b.handle), arr(b.handle, c.handle), 2, stream) == -1  # a chain in one call
    assert L.ldc_fv_prolong_enqueue(arr(a.handle), arr(b.handle), 0, stream) == -1
    wide = FVSolver(**dict(YAML, nx=12, ny=12, Re=100.0, Lx=2.0))
    assert L.ldc_fv_prolong_enqueue(arr(a.handle), arr(wide.handle), 1, stream) == -1                   # another domain
    wide.close()
    import torch
    torch.cuda.synchronize()
    for s, st in zip((a, b, c), before):
        now = s.state()
        assert all(np.array_equal(now[k], st[k]) for k in STATE)
    assert L.ldc_fv_prolong_enqueue(arr(a.handle, a.handle), arr(b.handle, c.handle), 2, stream) == 0   # one coarse trial, two fine
    torch.cuda.synchronize()
    assert np.array_equal(b.state()["u"], _restated(a, b)["u"]) and np.array_equal(c.state()["u"], _restated(a, c)["u"])
    for s in (a, b, c):
        s.close()
