"""Finite-volume trials that share their launches (mapping="shared", ldc_fv_wide_batch_*), CPU side: the C ABI against the
header, create and enqueue validation on host-side handles without a device, the parameter surface, the launcher's
routing, and the batch's budget retry loop driven by a fake device, alone and through run_chunks."""
import ctypes as C
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))

from conftest import PKG  # noqa: E402

NEW = ("ldc_fv_wide_batch_create", "ldc_fv_wide_batch_destroy", "ldc_fv_wide_batch_enqueue",
       "ldc_fv_wide_batch_set_graph", "ldc_fv_wide_batch_launches")
E_ARG, E_STATE, E_NODEVICE = -1, -2, -3


@pytest.fixture(scope="module")
def fvlib():
    import __graft_entry__ as g
    g.build()
    from solvers.fv import ldc_fv_lib
    return ldc_fv_lib


# ------------------------------------------------------------------------------------------- C ABI
def test_batch_entries_are_declared_exported_and_bound(fvlib):
    hdr = (ROOT / "include" / "ldc_fv.h").read_text()
    L = fvlib.lib()
    for name in NEW:
        assert name in fvlib.EXPORTS and re.search(rf"int {name}\(", hdr), name
        assert getattr(L, name).restype is C.c_int
    val = lambda name: int(re.search(rf"#define {name} \(?(-?\d+)", hdr).group(1))        # noqa: E731
    assert val("LDC_FV_WIDE_BATCH_MAX") == fvlib.WIDE_BATCH_MAX == 256
    assert val("LDC_FV_WIDE_BATCH_ENTRY_BYTES") == fvlib.WIDE_BATCH_ENTRY_BYTES
    assert val("LDC_FV_VERSION") == fvlib.VERSION == 2                    # the additions came without a new version
    # the macros, evaluated from the header's own text
    py = lambda text: text.replace("(int64_t)", "").replace("/", "//")    # noqa: E731
    gemm = re.search(r"#define LDC_FV_WIDE_GEMM_GROUPS\(nx, ny\) (.*)", hdr).group(1)
    table = re.search(r"#define LDC_FV_WIDE_BATCH_TABLE_LEN\(n, sweep_groups, gemm_groups\) (.*)", hdr).group(1)
    sizes = [(8, 8), (13, 17), (16, 16), (37, 50), (8, 300), (300, 9), (272, 260), (1024, 1024)]
    for nx, ny in sizes:
        tiles = -(-nx // 16) * -(-ny // 16)
        assert eval(py(gemm), dict(nx=nx, ny=ny)) == fvlib.wide_gemm_groups(nx, ny) == -(-tiles // 4)
    for part in (sizes[:1], sizes[:3], sizes):
        sweep = sum(fvlib.wide_groups(*z) for z in part)
        gg = sum(fvlib.wide_gemm_groups(*z) for z in part)
        want = eval(py(table), dict(n=len(part), sweep_groups=sweep, gemm_groups=gg,
                                    LDC_FV_WIDE_BATCH_ENTRY_BYTES=fvlib.WIDE_BATCH_ENTRY_BYTES))
        assert want == fvlib.wide_batch_table_len(part) == 256 * len(part) + 4 * (sweep + gg)


def test_an_older_library_is_refused_by_name(fvlib, monkeypatch):
    """A library without the new symbols is refused with their names, as for the earlier additions."""
    from solvers.spectral import ldc_lib

    class Old:
        def __getattr__(self, name):
            if name in NEW:
                raise AttributeError(name)
            return object()

    monkeypatch.setattr(fvlib, "_bound", None)
    monkeypatch.setattr(ldc_lib, "lib", lambda: Old())
    with pytest.raises(ldc_lib.LdcError, match="ldc_fv_wide_batch_create.*ldc_fv_wide_batch_launches"):
        fvlib.lib()


class HostWide(C.Structure):
    """The library's host-side ``struct ldc_fv_wide`` (csrc/ldc_fv_wide.hip) as far as ldc_fv_wide_batch_create reads it
    before it asks for a device: the trial's descriptor (sizes, max_lin_iters), the work-groups of a sweep, the device."""
    _fields_ = ([(n, C.c_int) for n in ("nx", "ny", "scheme", "rec_cap", "warmup", "maxit")]
                + [("rest", C.c_double * 21), ("scr", C.c_void_p), ("G", C.c_int), ("pad", C.c_int), ("device", C.c_int),
                   ("graph", C.c_int), ("tail", C.c_double * 8)])


class HostBatch(C.Structure):
    """The head of ``struct ldc_fv_wide_batch``: all that enqueue, launches and set_graph read without a device."""
    _fields_ = [(n, C.c_int) for n in ("n", "maxit", "device", "graph")] + [("rec_cap", C.c_int * 256),
                                                                           ("tail", C.c_double * 16)]


OTHER = 63        # a device number no handle of this process has: a call with everything in order stops at the device


def _wide(fvlib, nx=16, ny=16, maxit=1000, device=OTHER, rec_cap=4):
    return HostWide(nx=nx, ny=ny, scheme=1, rec_cap=rec_cap, warmup=10, maxit=maxit, G=fvlib.wide_groups(nx, ny),
                    device=device)


def _list(hs):
    return (C.c_void_p * len(hs))(*[C.addressof(h) if h is not None else None for h in hs])


def test_batch_create_validation_on_host_side_handles(fvlib):
    L = fvlib.lib()
    out = C.c_void_p()
    fake, big = C.c_void_p(8), 1 << 24                          # never dereferenced: validation comes first
    hs = [_wide(fvlib), _wide(fvlib, 37, 50), _wide(fvlib, 272, 260)]
    create = lambda lst, n, table=fake, length=big: L.ldc_fv_wide_batch_create(lst, n, table, length, C.byref(out))  # noqa: E731
    # LDC_E_ARG: a null list, n < 1, n > MAX, a null table
    assert create(None, 3) == E_ARG
    assert create(_list(hs), 0) == E_ARG and create(_list(hs), -2) == E_ARG
    many = [_wide(fvlib) for _ in range(257)]
    assert create(_list(many), 257) == E_ARG
    assert create(_list(hs), 3, None) == E_ARG
    assert L.ldc_fv_wide_batch_create(_list(hs), 3, fake, big, None) == E_ARG
    # a short table: one byte less than the macro, for one trial and for three
    for part in (hs[:1], hs):
        need = fvlib.wide_batch_table_len([(h.nx, h.ny) for h in part])
        assert create(_list(part), len(part), fake, need - 1) == E_ARG
        assert create(_list(part), len(part), fake, need) in (E_NODEVICE, E_STATE)        # in order up to the device
    # a handle listed twice, trials whose max_lin_iters differ
    assert create(_list([hs[0], hs[1], hs[0]]), 3) == E_ARG
    assert create(_list([hs[0], _wide(fvlib, maxit=999)]), 2) == E_ARG
    # LDC_E_STATE: a null handle, a handle of another device
    assert create(_list([hs[0], None, hs[2]]), 3) == E_STATE
    assert create(_list([hs[0], _wide(fvlib, device=OTHER - 1)]), 2) == E_STATE
    assert not out.value
    # 256 trials are in order
    assert create(_list(many[:256]), 256) in (E_NODEVICE, E_STATE)
    assert not out.value


def test_batch_enqueue_validation_and_launches_on_a_host_side_batch(fvlib):
    L = fvlib.lib()
    b = HostBatch(n=3, maxit=1000, device=OTHER, graph=0)
    b.rec_cap[0], b.rec_cap[1], b.rec_cap[2] = 4, 8, 2
    bp = C.c_void_p(C.addressof(b))
    q = lambda *ks: (C.c_int32 * len(ks))(*ks)        # noqa: E731
    assert L.ldc_fv_wide_batch_enqueue(None, q(1, 1, 1), 12, None) == E_STATE
    assert L.ldc_fv_wide_batch_enqueue(bp, None, 12, None) == E_ARG
    assert L.ldc_fv_wide_batch_enqueue(bp, q(1, 1, 1), 0, None) == E_ARG
    assert L.ldc_fv_wide_batch_enqueue(bp, q(1, -1, 1), 12, None) == E_ARG
    assert L.ldc_fv_wide_batch_enqueue(bp, q(5, 1, 1), 12, None) == E_ARG            # above trial 0's rec_cap
    assert L.ldc_fv_wide_batch_enqueue(bp, q(4, 8, 3), 12, None) == E_ARG            # above trial 2's
    assert L.ldc_fv_wide_batch_enqueue(bp, q(0, 0, 0), 12, None) == E_ARG            # nobody has anything to do
    for ok in (q(4, 8, 2), q(3, 0, 0), q(0, 0, 1)):
        assert L.ldc_fv_wide_batch_enqueue(bp, ok, 12, None) in (E_NODEVICE, E_STATE)
    assert L.ldc_fv_wide_batch_launches(bp, 12) == 11 + 5 * 12
    assert L.ldc_fv_wide_batch_launches(bp, 1000) == L.ldc_fv_wide_batch_launches(bp, 4000) == 11 + 5 * 1000
    assert L.ldc_fv_wide_batch_launches(bp, 0) == E_ARG and L.ldc_fv_wide_batch_launches(None, 12) == E_ARG
    assert L.ldc_fv_wide_batch_set_graph(None, 1) == E_STATE and L.ldc_fv_wide_batch_set_graph(bp, 2) == E_ARG
    assert L.ldc_fv_wide_batch_set_graph(bp, 1) == 0 and b.graph == 1
    assert L.ldc_fv_wide_batch_set_graph(bp, 0) == 0 and b.graph == 0
    assert L.ldc_fv_wide_batch_destroy(None) == E_STATE


# ------------------------------------------------------------------------------------------- parameters, routing
def test_parameter_surface(monkeypatch):
    from solvers.datastructures import FVFSGParameters, FVParameters
    from solvers.fv.batched import BatchedFVFSGSolver, BatchedFVSolver
    from solvers.fv.fsg import FVFSGSolver
    from solvers.fv.solver import MAPPINGS, FVSolver
    from solvers.spectral import ldc_lib
    assert MAPPINGS == ("cu", "chip", "shared") and FVParameters().mapping == "cu"
    ml = FVParameters(mapping="shared", linear_budget=5).to_mlflow()
    assert "mapping" not in ml and "linear_budget" not in ml
    assert "mapping" not in FVFSGParameters(mapping="shared").to_mlflow()
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)        # every ValueError comes before the device
    base = dict(name="fv", Re=100.0, nx=16, ny=16)
    for bad, word in ((dict(mapping="shared", acceleration="anderson"), "anderson.*shared"),
                      (dict(mapping="shared", nx=300, vortex_metrics="device"), "vortex_metrics"),
                      (dict(mapping="shared", nx=1025), "1024"), (dict(mapping="shared", ny=7), "8"),
                      (dict(mapping="each"), "shared")):
        with pytest.raises(ValueError, match=word):
            FVSolver(**dict(base, **bad))
    # what is in order gets as far as the device
    for ok in (dict(mapping="shared"), dict(mapping="shared", nx=1024, ny=8), dict(mapping="shared", nx=300, ny=260),
               dict(mapping="shared", vortex_metrics="device")):
        with pytest.raises(ldc_lib.LdcError, match="no CPU fallback"):
            FVSolver(**dict(base, **ok))
    with pytest.raises(ldc_lib.LdcError, match="no CPU fallback"):
        BatchedFVSolver([dict(base, mapping="shared"), dict(base, mapping="shared", nx=300, ny=9)])
    with pytest.raises(ldc_lib.LdcError, match="no CPU fallback"):
        FVFSGSolver(**dict(base, mapping="shared", nx=64, ny=64))
    with pytest.raises(ValueError, match="FSG level"):
        FVFSGSolver(**dict(base, mapping="shared", nx=512, ny=512))
    # a batch is all shared or not at all; chip is refused as before; sequenced batches do not take shared trials
    for mixed in ([dict(base), dict(base, mapping="shared")], [dict(base, mapping="shared"), dict(base, mapping="cu")]):
        with pytest.raises(ValueError, match="mapping='shared' beside mapping='cu'"):
            BatchedFVSolver(mixed)
    with pytest.raises(ValueError, match="mapping='chip' inside a batch"):
        BatchedFVSolver([dict(base, mapping="shared"), dict(base, mapping="chip")])
    with pytest.raises(ValueError, match="at most 256"):
        BatchedFVSolver([dict(base, mapping="shared")] * 257)
    with pytest.raises(ValueError, match="mapping='shared' in a BatchedFVFSGSolver"):
        BatchedFVFSGSolver([dict(base, mapping="shared"), dict(base, mapping="shared")])


def test_launcher_routes_shared_trials_into_batches_of_their_own():
    sys.path.insert(0, str(PKG))
    import main as M
    from utilities.config import compose as Cmp
    comp = Cmp.Composer(PKG / "conf")
    plain = Cmp.resolve(Cmp.compose_job(comp, ["solver=fv", "N=16"], []))
    shared = Cmp.resolve(Cmp.compose_job(comp, ["solver=fv", "N=16", "+solver.mapping=shared"], []))
    assert shared["solver"] == dict(plain["solver"], mapping="shared")       # conf/solver/fv.yaml itself is unchanged
    assert M.batch_key(shared) == (M.FV, "shared") != M.batch_key(plain)
    seq = Cmp.resolve(Cmp.compose_job(comp, ["solver=fv/fsg", "N=16", "+solver.mapping=shared"], []))
    assert M.batch_key(seq) == (M.FV_FSG, "shared")
    assert M.FV_WIDE_BATCH_MAX == 256
    key = (M.FV, "shared")
    assert M.batch_sizes(key, 6, 64, False) == [6]
    assert M.batch_sizes(key, 300, 64, False) == [256, 44]                   # cut at LDC_FV_WIDE_BATCH_MAX
    assert M.batch_sizes(key, 600, 64, False) == [256, 256, 88]
    assert M.batch_sizes(key, 10, 4, True) == [4, 4, 2]                      # the user's cap
    assert M.batch_sizes(key, 600, 300, True) == [256, 256, 88]              # (a batch object takes no more than 256)
    assert M.batch_sizes(key, 1, 64, False) == [] and M.batch_sizes(key, 5, 1, True) == []
    for given in (False, True):
        assert M.batch_sizes((M.FV_FSG, "shared"), 300, 64, given) == []      # sequenced shared trials: one by one


# ------------------------------------------------------------------------------------------- the batch's retry loop
class FakeBatchDevice:
    """Trials whose iteration i needs ``need[q][i]`` BiCGSTAB iterations.  An enqueue gives trial q ``quotas[q]``
    iterations at one budget for all: the trial completes iterations until one needs more than the budget (overflow:
    that iteration has changed nothing), its latch iteration, or its quota.  A trial that is latched does nothing."""

    def __init__(self, need, max_lin=1000, latch_at=None):
        self.need, self.max_lin = [list(x) for x in need], max_lin
        self.latch_at = latch_at or [None] * len(need)
        self.total, self.latched, self.calls = [0] * len(need), [0] * len(need), []

    def step(self, quotas, budget):
        self.calls.append((list(quotas), budget))
        out = []
        for q, m in enumerate(quotas):
            rows, overflow = [], 0
            for _ in range(m):
                if self.latched[q]:
                    break
                if min(budget, self.max_lin) < min(self.need[q][self.total[q]], self.max_lin):
                    overflow = 1
                    break
                rows.append([float(self.total[q])] * 8)
                self.total[q] += 1
                if self.latch_at[q] is not None and self.total[q] == self.latch_at[q]:
                    self.latched[q] = 1
            out.append((np.array(rows).reshape(-1, 8), self.latched[q], 0, self.total[q], overflow))
        return out


def test_one_trial_of_three_overflows_twice_and_nobody_loses_an_iteration():
    from solvers.fv.solver import advance_batch_with_budget
    d = FakeBatchDevice([[3, 4, 2, 2, 4, 1], [3, 3, 9, 3, 12, 3], [1] * 6], latch_at=[None, None, 4])
    out = advance_batch_with_budget(d.step, [0, 0, 0], [6, 6, 6], [4, 4, 4], 1000)
    # trial 1 stops before its iteration 2 (9 > 4), again at budget 8, and does its four remaining iterations at 16;
    # the others have quota 0 in the retries
    assert d.calls == [([6, 6, 6], 4), ([0, 4, 0], 8), ([0, 4, 0], 16)]
    (r0, l0, n0, t0, b0, x0), (r1, l1, n1, t1, b1, x1), (r2, l2, n2, t2, b2, x2) = out
    assert (l0, n0, t0, b0, x0) == (0, 0, 6, 4, 0) and r0[:, 0].tolist() == [0, 1, 2, 3, 4, 5]
    assert (l1, n1, t1, b1, x1) == (0, 0, 6, 16, 2) and r1[:, 0].tolist() == [0, 1, 2, 3, 4, 5]      # once each, in order
    assert (l2, n2, t2, b2, x2) == (1, 0, 4, 4, 0) and r2[:, 0].tolist() == [0, 1, 2, 3]             # latched in mid-chunk
    # the next chunk: the call's budget is the largest of the LIVE trials' budgets, and trial 2 is not among them
    d.need[0] += [5, 2]
    d.need[1] += [2, 2]
    out = advance_batch_with_budget(d.step, [6, 6, 4], [2, 0, 0], [4, 16, 4], 1000)
    assert d.calls[3:] == [([2, 0, 0], 4), ([2, 0, 0], 8)]
    assert out[0][3:] == (8, 8, 1) and out[0][0][:, 0].tolist() == [6, 7]
    assert out[1][3:] == (6, 16, 0) and len(out[1][0]) == 0 and out[2][3:] == (4, 4, 0)
    out = advance_batch_with_budget(d.step, [8, 6, 4], [0, 2, 0], [8, 16, 4], 1000)
    assert d.calls[5:] == [([0, 2, 0], 16)] and out[1][3:] == (8, 16, 0)


def test_the_batch_loop_agrees_with_the_lone_loop_on_one_trial():
    from solvers.fv.solver import advance_batch_with_budget, advance_with_budget
    need = [3, 4, 9, 9, 20, 5, 5, 5]
    d = FakeBatchDevice([need])
    (rows, latch, nan, total, budget, retries), = advance_batch_with_budget(d.step, [0], [8], [4], 1000)
    calls = []

    def lone(m, b, dev=FakeBatchDevice([need])):
        calls.append(([m], b))
        return dev.step([m], b)[0]

    want = advance_with_budget(lone, 0, 8, 4, 1000)
    assert (latch, nan, total, budget, retries) == want[1:] == (0, 0, 8, 32, 3)
    assert np.array_equal(rows, want[0]) and d.calls == calls == [([8], 4), ([6], 8), ([6], 16), ([4], 32)]


def test_the_batch_loop_stops_at_max_lin_iters_and_reports_a_stuck_device():
    from solvers.fv.solver import advance_batch_with_budget
    d = FakeBatchDevice([[2, 5000, 2], [2, 2, 2]], max_lin=10)
    out = advance_batch_with_budget(d.step, [0, 0], [3, 3], [3, 3], 10)
    assert [c[1] for c in d.calls] == [3, 6, 10]                  # 3 -> 6 -> 10, where the give-up is accepted
    assert out[0][3:] == (3, 10, 2) and out[1][3:] == (3, 3, 0)
    none = np.zeros((0, 8))
    # an overflow at the full budget, no progress without one, rows that do not match the count, a quota-0 trial that
    # moved: errors, not loops
    with pytest.raises(RuntimeError, match="overflow"):
        advance_batch_with_budget(lambda q, b: [(none, 0, 0, 0, 1)], [0], [2], [10], 10)
    with pytest.raises(RuntimeError, match="no progress"):
        advance_batch_with_budget(lambda q, b: [(none, 0, 0, 0, 0)], [0], [2], [4], 10)
    with pytest.raises(RuntimeError, match="record rows"):
        advance_batch_with_budget(lambda q, b: [(np.zeros((1, 8)), 0, 0, 2, 0)], [0], [2], [4], 10)
    with pytest.raises(RuntimeError, match="quota 0"):
        advance_batch_with_budget(lambda q, b: [(np.zeros((2, 8)), 0, 0, 2, 0), (np.zeros((1, 8)), 0, 0, 1, 0)],
                                  [0, 0], [2, 0], [4, 4], 10)
    with pytest.raises(RuntimeError, match="one result per trial"):
        advance_batch_with_budget(lambda q, b: [(none, 0, 0, 0, 0)], [0, 0], [2, 2], [4, 4], 10)


class FakeShared:
    """What BatchedFVSolver._step asks of solver.SharedBatch, on a FakeBatchDevice."""

    def __init__(self, dev, budgets):
        self.dev, self.budgets, self.retries, self.asked = dev, list(budgets), [0] * len(budgets), []

    def advance(self, ks):
        from solvers.fv.solver import advance_batch_with_budget
        self.asked.append(list(ks))
        out = advance_batch_with_budget(self.dev.step, list(self.dev.total), ks, self.budgets, self.dev.max_lin)
        for q, (_, _, _, _, budget, retries) in enumerate(out):
            self.budgets[q] = budget
            self.retries[q] += retries
        return [o[:4] for o in out]


def test_the_same_through_run_chunks():
    """Three trials with rings of 4, 8 and 3 rows and caps of 10, 7 and 20 iterations; trial 1 overflows twice, trial 2
    latches at its iteration 5.  Chunks of 3, 3, 1 and 3 iterations: every trial gets every iteration once."""
    from solvers.fv.batched import BatchedFVSolver, run_chunks
    need = [[2] * 10, [2, 2, 2, 2, 9, 2, 2], [1] * 20]
    dev = FakeBatchDevice(need, latch_at=[None, None, 5])
    batch = object.__new__(BatchedFVSolver)
    batch.solvers, batch.shared = [None] * 3, FakeShared(dev, [4, 4, 4])
    out = run_chunks([4, 8, 3], [10, 7, 20], batch._step)
    assert [(latch, nan, total) for latch, nan, total, _ in out] == [(0, 0, 10), (0, 0, 7), (1, 0, 5)]
    for (_, _, total, rows) in out:
        assert rows[:, 0].tolist() == list(range(total))
    assert batch.shared.asked == [[3, 3, 3], [3, 3, 3], [1, 1, 0], [3, 0, 0]]        # a trial that left gets quota 0
    assert batch.shared.retries == [0, 2, 0] and batch.shared.budgets == [4, 16, 4]
    # the device saw: two chunks for all, trial 1 alone twice, then the chunks of the trials still live, the first of
    # them at trial 1's budget
    assert dev.calls == [([3, 3, 3], 4), ([3, 3, 3], 4), ([0, 2, 0], 8), ([0, 2, 0], 16), ([1, 1, 0], 16), ([3, 0, 0], 4)]
