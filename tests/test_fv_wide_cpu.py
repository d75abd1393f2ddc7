"""A lone finite-volume trial on the whole chip (mapping="chip", ldc_fv_wide_*), CPU side: the C ABI against the
header, argument validation without a device, the parameter surface, the launcher's routing and the budget retry loop
driven by a fake step."""
import ctypes as C
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))

from conftest import PKG  # noqa: E402


@pytest.fixture(scope="module")
def fvlib():
    import __graft_entry__ as g
    g.build()
    from solvers.fv import ldc_fv_lib
    return ldc_fv_lib


# ------------------------------------------------------------------------------------------- C ABI
def test_wide_entries_are_declared_exported_and_bound(fvlib):
    hdr = (ROOT / "include" / "ldc_fv.h").read_text()
    L = fvlib.lib()
    for name in ("ldc_fv_wide_create", "ldc_fv_wide_destroy", "ldc_fv_wide_enqueue", "ldc_fv_wide_launches",
                 "ldc_fv_wide_status", "ldc_fv_wide_set_graph"):
        assert name in fvlib.EXPORTS and re.search(rf"int {name}\(", hdr), name
        assert getattr(L, name).restype is C.c_int
    val = lambda name: int(re.search(rf"#define {name} \(?(-?\d+)", hdr).group(1))        # noqa: E731
    assert val("LDC_FV_WIDE_MAX_N") == fvlib.WIDE_MAX_N == 1024
    assert val("LDC_FV_WIDE_E_BUDGET") == fvlib.E_BUDGET
    assert (val("LDC_FV_MAX_N"), val("LDC_FV_VERSION")) == (256, 2)        # the one-CU kernel's range did not move
    assert C.sizeof(fvlib.Problem) == 24 + 72 + 96                        # nor did struct ldc_fv_problem
    # the scratch macro, evaluated from the header's own text
    groups = re.search(r"#define LDC_FV_WIDE_GROUPS\(nx, ny\) (.*)", hdr).group(1)
    scratch = re.search(r"#define LDC_FV_WIDE_SCRATCH_LEN\(nx, ny\) (.*)", hdr).group(1)
    for nx, ny in ((8, 8), (13, 17), (16, 16), (255, 257), (256, 256), (272, 260), (1024, 1024)):
        g = eval(groups.replace("(int64_t)", "").replace("/", "//").replace("?", " and ").replace(":", " or "),
                 dict(nx=nx, ny=ny))
        assert g == fvlib.wide_groups(nx, ny) == min(256, -(-nx * ny // 256))
        want = eval(scratch.replace("LDC_FV_WIDE_GROUPS(nx, ny)", str(g)))
        assert want == fvlib.wide_scratch_len(nx, ny)


def _good(fvlib, **change):
    fake = 8                                                     # never dereferenced: validation comes first
    good = dict(nx=16, ny=16, scheme=1, rec_cap=4, warmup=10, max_lin_iters=1000, dx=1 / 16, dy=1 / 16, rho=1.0,
                mu=0.01, alpha_uv=0.4, alpha_p=0.2, lin_tol=1e-9, tol=1e-6, lid_velocity=1.0,
                **{k: fake for k in ("ulid", "Qx", "lamx", "Qy", "lamy", "u", "v", "p", "mdot", "work", "rec", "ctrl")})
    return fvlib.Problem(**dict(good, **change))


def test_wide_argument_validation_needs_no_device(fvlib):
    L = fvlib.lib()
    h = C.c_void_p()
    fake, big = 8, 1 << 20
    assert L.ldc_fv_wide_create(None, fake, big, C.byref(h)) == -1
    assert L.ldc_fv_wide_create(C.byref(_good(fvlib)), fake, big, None) == -1
    bad = [dict(nx=7), dict(ny=1025), dict(nx=1025), dict(scheme=2), dict(rec_cap=0), dict(max_lin_iters=0),
           dict(warmup=-1), dict(dx=0.0), dict(mu=-1.0), dict(alpha_uv=0.0), dict(alpha_p=1.5), dict(lin_tol=0.0),
           dict(tol=-1.0), dict(work=None), dict(ctrl=None), dict(Qy=None)]
    for change in bad:
        assert L.ldc_fv_wide_create(C.byref(_good(fvlib, **change)), fake, big, C.byref(h)) == -1, change
        assert not h.value
    # the scratch: null, and one double short of the macro, at a size below and one above the one-CU kernel's range
    for nx, ny in ((16, 16), (272, 260), (1024, 1024)):
        pr = _good(fvlib, nx=nx, ny=ny, dx=1 / nx, dy=1 / ny)
        need = fvlib.wide_scratch_len(nx, ny)
        assert L.ldc_fv_wide_create(C.byref(pr), None, need, C.byref(h)) == -1
        assert L.ldc_fv_wide_create(C.byref(pr), fake, need - 1, C.byref(h)) == -1
        assert not h.value
        # everything the host can check is in order: what is left is the device (none here), or a handle
        rc = L.ldc_fv_wide_create(C.byref(pr), fake, need, C.byref(h))
        assert rc in (0, -3)
        if rc == 0:
            assert L.ldc_fv_wide_enqueue(h, 0, 12, None) == -1
            assert L.ldc_fv_wide_enqueue(h, 5, 12, None) == -1            # n_iters > rec_cap
            assert L.ldc_fv_wide_enqueue(h, 1, 0, None) == -1             # lin_budget < 1
            assert L.ldc_fv_wide_launches(h, 12) == 71 and L.ldc_fv_wide_launches(h, 2000) == 11 + 5 * 1000
            assert L.ldc_fv_wide_set_graph(h, 2) == -1 and L.ldc_fv_wide_set_graph(h, 1) == 0
            assert L.ldc_fv_wide_destroy(h) == 0
            h = C.c_void_p()
    for rc in (L.ldc_fv_wide_destroy(None), L.ldc_fv_wide_enqueue(None, 1, 12, None), L.ldc_fv_wide_status(None)):
        assert rc == -2
    assert L.ldc_fv_wide_launches(None, 12) == -1
    assert L.ldc_fv_wide_set_graph(None, 1) == -2


class HostWide(C.Structure):
    """The head of the library's host-side ``struct ldc_fv_wide`` (csrc/ldc_fv_wide.hip): the trial's descriptor, of
    which enqueue's validation reads rec_cap before it asks for a device."""
    _fields_ = [(n, C.c_int) for n in ("nx", "ny", "scheme", "rec_cap", "warmup", "maxit")] + [("rest", C.c_double * 24)]


def test_wide_enqueue_validation_on_a_host_side_handle(fvlib):
    L = fvlib.lib()
    h = HostWide(nx=16, ny=16, scheme=1, rec_cap=4, warmup=10, maxit=1000)
    hp = C.c_void_p(C.addressof(h))
    assert L.ldc_fv_wide_enqueue(hp, 0, 12, None) == -1
    assert L.ldc_fv_wide_enqueue(hp, 5, 12, None) == -1
    assert L.ldc_fv_wide_enqueue(hp, 4, 0, None) == -1
    assert L.ldc_fv_wide_enqueue(hp, 4, -3, None) == -1
    assert L.ldc_fv_wide_launches(hp, 0) == -1
    assert L.ldc_fv_wide_launches(hp, 12) == 11 + 5 * 12
    assert L.ldc_fv_wide_launches(hp, 1000) == L.ldc_fv_wide_launches(hp, 4000) == 11 + 5 * 1000


# ------------------------------------------------------------------------------------------- parameters, routing
def test_parameter_surface(monkeypatch):
    from solvers.datastructures import FVFSGParameters, FVParameters
    from solvers.fv.batched import BatchedFVSolver
    from solvers.fv.fsg import FVFSGSolver
    from solvers.fv.solver import FVSolver
    from solvers.spectral import ldc_lib
    p = FVParameters()
    assert (p.mapping, p.linear_budget) == ("cu", 12)
    ml = FVParameters(mapping="chip", linear_budget=5).to_mlflow()
    assert "mapping" not in ml and "linear_budget" not in ml and "device" not in ml
    assert FVFSGParameters(mapping="chip").mapping == "chip"
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)        # every ValueError comes before the device
    base = dict(name="fv", Re=100.0, nx=16, ny=16)
    for bad, word in ((dict(mapping="xcd"), "mapping"), (dict(linear_budget=0), "linear_budget"),
                      (dict(mapping="chip", acceleration="anderson"), "anderson"),
                      (dict(mapping="chip", nx=300, vortex_metrics="device"), "vortex_metrics"),
                      (dict(mapping="chip", nx=1025), "1024"), (dict(mapping="chip", ny=7), "8"),
                      (dict(nx=300), "256"), (dict(mapping="cu", ny=257), "256")):
        with pytest.raises(ValueError, match=word):
            FVSolver(**dict(base, **bad))
    # what is in order gets as far as the device
    for ok in (dict(mapping="chip"), dict(mapping="chip", nx=1024, ny=8), dict(mapping="chip", vortex_metrics="device"),
               dict(mapping="chip", nx=300, ny=260)):
        with pytest.raises(ldc_lib.LdcError, match="no CPU fallback"):
            FVSolver(**dict(base, **ok))
    with pytest.raises(ValueError, match="FSG level"):
        FVFSGSolver(**dict(base, mapping="chip", nx=512, ny=512))
    with pytest.raises(ldc_lib.LdcError, match="no CPU fallback"):
        FVFSGSolver(**dict(base, mapping="chip", nx=256, ny=256))
    with pytest.raises(ValueError, match="chip"):
        BatchedFVSolver([dict(base), dict(base, mapping="chip")])


def test_launcher_routes_chip_trials_one_by_one():
    sys.path.insert(0, str(PKG))
    import main as M
    from utilities.config import compose as Cmp
    comp = Cmp.Composer(PKG / "conf")
    plain = Cmp.resolve(Cmp.compose_job(comp, ["solver=fv", "N=16"], []))
    chip = Cmp.resolve(Cmp.compose_job(comp, ["solver=fv", "N=16", "+solver.mapping=chip"], []))
    assert chip["solver"] == dict(plain["solver"], mapping="chip")          # conf/solver/fv.yaml itself is unchanged
    assert "mapping" not in plain["solver"]
    assert M.batch_key(plain) == (M.FV,)
    assert M.batch_key(chip) == (M.FV, "chip")
    seq = Cmp.resolve(Cmp.compose_job(comp, ["solver=fv/fsg", "N=16", "+solver.mapping=chip"], []))
    assert M.batch_key(seq) == (M.FV_FSG, "chip")
    for given in (False, True):
        assert M.batch_sizes((M.FV, "chip"), 5, 64, given) == []
        assert M.batch_sizes((M.FV_FSG, "chip"), 300, 64, given) == []
    assert M.batch_sizes((M.FV,), 5, 64, False) == [5]
    assert M.batch_sizes((M.FV,), 300, 64, False) == [256, 44]


# ------------------------------------------------------------------------------------------- the retry loop
class FakeDevice:
    """A trial whose iteration i needs ``need[i]`` BiCGSTAB iterations: an enqueue completes iterations until one needs
    more than the budget (overflow: that iteration has changed nothing), the latch iteration, or all it was given."""

    def __init__(self, need, max_lin=1000, latch_at=None):
        self.need, self.max_lin, self.latch_at = list(need), max_lin, latch_at
        self.total, self.calls = 0, []

    def step(self, m, budget):
        self.calls.append((self.total, m, budget))
        rows, overflow, latch = [], 0, 0
        for _ in range(m):
            if min(budget, self.max_lin) < min(self.need[self.total], self.max_lin):
                overflow = 1
                break
            rows.append([float(self.total)] * 8)
            self.total += 1
            if self.latch_at is not None and self.total == self.latch_at:
                latch = 1
                break
        return np.array(rows).reshape(-1, 8), latch, 0, self.total, overflow


def test_retry_loop_doubles_the_budget_and_loses_nothing():
    from solvers.fv.solver import advance_with_budget
    need = [3, 4, 9, 9, 20, 5, 5, 5]
    d = FakeDevice(need)
    rows, latch, nan, total, budget, retries = advance_with_budget(d.step, 0, 8, 4, 1000)
    assert (latch, nan, total, budget, retries) == (0, 0, 8, 32, 3)
    assert rows[:, 0].tolist() == [0, 1, 2, 3, 4, 5, 6, 7]                  # every iteration once, in order
    assert d.calls == [(0, 8, 4), (2, 6, 8), (2, 6, 16), (4, 4, 32)]
    # the next chunk goes on from the budget reached, at the count reached
    d.need += [30, 40]
    rows, _, _, total, budget, retries = advance_with_budget(d.step, 8, 2, budget, 1000)
    assert (total, budget, retries) == (10, 64, 1) and rows[:, 0].tolist() == [8, 9]


def test_retry_loop_stops_at_max_lin_iters_and_at_the_latch():
    from solvers.fv.solver import advance_with_budget
    d = FakeDevice([2, 5000, 2], max_lin=10)
    rows, _, _, total, budget, retries = advance_with_budget(d.step, 0, 3, 3, 10)
    assert (total, budget, retries) == (3, 10, 2) and len(rows) == 3        # 3 -> 6 -> 10, where the give-up is accepted
    assert [c[2] for c in d.calls] == [3, 6, 10]
    d = FakeDevice([2] * 10, latch_at=4)
    rows, latch, _, total, budget, retries = advance_with_budget(d.step, 0, 10, 12, 1000)
    assert (latch, total, budget, retries, len(rows)) == (1, 4, 12, 0, 4)
    # a device that reports an overflow at the full budget, or no progress without one, is an error, not a loop
    with pytest.raises(RuntimeError, match="overflow"):
        advance_with_budget(lambda m, b: (np.zeros((0, 8)), 0, 0, 0, 1), 0, 2, 10, 10)
    with pytest.raises(RuntimeError, match="no progress"):
        advance_with_budget(lambda m, b: (np.zeros((0, 8)), 0, 0, 0, 0), 0, 2, 4, 10)
    with pytest.raises(RuntimeError, match="record rows"):
        advance_with_budget(lambda m, b: (np.zeros((1, 8)), 0, 0, 2, 0), 0, 2, 4, 10)
