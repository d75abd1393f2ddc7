"""Anderson acceleration of chip and shared finite-volume trials (acceleration="anderson_chip", ldc_fv_wide_set_anderson),
CPU side: the C ABI against the header, every refused argument on a host-side handle without a device, the launch counts
with and without mixing, the parameter surface and the launcher's override."""
import ctypes as C
import re
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))

from conftest import PKG  # noqa: E402

E_ARG, E_STATE, E_NODEVICE = -1, -2, -3
SIZES = ((8, 8), (300, 260), (1024, 1024))


@pytest.fixture(scope="module")
def fvlib():
    import __graft_entry__ as g
    g.build()
    from solvers.fv import ldc_fv_lib
    return ldc_fv_lib


# ------------------------------------------------------------------------------------------- C ABI
def test_the_entry_and_the_macros_are_declared_exported_and_bound(fvlib):
    hdr = (ROOT / "include" / "ldc_fv.h").read_text()
    L = fvlib.lib()
    assert "ldc_fv_wide_set_anderson" in fvlib.EXPORTS
    assert re.search(r"int ldc_fv_wide_set_anderson\(ldc_fv_wide \*h, const struct ldc_fv_anderson \*acc, double \*scratch, "
                     r"int64_t scratch_len\);", hdr)
    assert L.ldc_fv_wide_set_anderson.restype is C.c_int
    val = lambda name: int(re.search(rf"#define {name} \(?(-?\d+)", hdr).group(1))        # noqa: E731
    assert val("LDC_FV_VERSION") == fvlib.VERSION == L.ldc_fv_version() == 2      # the addition came without a new version
    assert val("LDC_FV_WIDE_ANDERSON_LAUNCHES") == fvlib.WIDE_ANDERSON_LAUNCHES == 3
    assert val("LDC_FV_WIDE_BATCH_ENTRY_BYTES") == 256 and C.sizeof(fvlib.Anderson) == 32
    # the scratch macro, evaluated from the header's own text
    text = re.search(r"#define LDC_FV_WIDE_ANDERSON_SCRATCH_LEN\(nx, ny, depth\) (.*)", hdr).group(1)
    for nx, ny in SIZES:
        g = fvlib.wide_groups(nx, ny)
        for depth in (1, 16):
            want = eval(text.replace("LDC_FV_WIDE_GROUPS(nx, ny)", str(g)).replace("(int64_t)", "").replace("/", "//"),
                        dict(depth=depth))
            assert want == fvlib.wide_anderson_scratch_len(nx, ny, depth) == 8 + g * (depth + depth * (depth + 1) // 2)
    assert [fvlib.wide_groups(*z) for z in SIZES] == [1, 256, 256]
    assert fvlib.wide_anderson_scratch_len(1024, 1024, 16) == 8 + 256 * 152
    # history memory of the docs: (2 depth + 3) L doubles
    L1024 = 3 * 1024 * 1024 + 2 * 1024 * 1025
    assert fvlib.anderson_hist_len(1024, 1024, 5) * 8 == 13 * L1024 * 8 and round(13 * L1024 * 8 / 1e9, 2) == 0.55
    assert fvlib.anderson_hist_len(1024, 1024, 16) * 8 == 35 * L1024 * 8 and round(35 * L1024 * 8 / 1e9, 1) == 1.5


def test_an_older_library_is_refused_by_name(fvlib, monkeypatch):
    from solvers.spectral import ldc_lib

    class Old:
        def __getattr__(self, name):
            if name == "ldc_fv_wide_set_anderson":
                raise AttributeError(name)
            return object()

    monkeypatch.setattr(fvlib, "_bound", None)
    monkeypatch.setattr(ldc_lib, "lib", lambda: Old())
    with pytest.raises(ldc_lib.LdcError, match="ldc_fv_wide_set_anderson"):
        fvlib.lib()


class HostWide(C.Structure):
    """The library's host-side ``struct ldc_fv_wide`` (csrc/ldc_fv_wide.hip): the trial's descriptor, the scratch, the
    work-groups of a sweep, the device, the two switches, the mixing block, and the (empty) list of captured graphs."""
    _fields_ = ([(n, C.c_int) for n in ("nx", "ny", "scheme", "rec_cap", "warmup", "maxit")]
                + [("rest", C.c_double * 21), ("scr", C.c_void_p), ("G", C.c_int), ("pad", C.c_int), ("device", C.c_int),
                   ("graph", C.c_short), ("mixing", C.c_short), ("hist", C.c_void_p), ("astate", C.c_void_p),
                   ("mscr", C.c_void_p), ("depth", C.c_int), ("start", C.c_int), ("graphs", C.c_double * 4)])


class HostBatch(C.Structure):
    """The head of ``struct ldc_fv_wide_batch`` as far as ldc_fv_wide_batch_launches reads it."""
    _fields_ = [(n, C.c_int) for n in ("n", "maxit", "device", "graph")] + [
        ("rec_cap", C.c_int * 256), ("sweep_groups", C.c_int), ("gemm_groups", C.c_int), ("mixing", C.c_int),
        ("tail", C.c_double * 16)]


def _wide(fvlib, nx, ny):
    return HostWide(nx=nx, ny=ny, scheme=1, rec_cap=4, warmup=10, maxit=1000, G=fvlib.wide_groups(nx, ny), device=63)


def test_set_anderson_argument_validation_needs_no_device(fvlib):
    L = fvlib.lib()
    A = fvlib.Anderson
    fake = 8                                                     # never dereferenced: nothing is launched or copied
    call = L.ldc_fv_wide_set_anderson
    assert C.sizeof(HostWide) == 280 and HostWide.hist.offset == 216
    for nx, ny in SIZES:
        h = _wide(fvlib, nx, ny)
        hp = C.c_void_p(C.addressof(h))
        for depth in (1, 3, 16):
            need_h, need_s = fvlib.anderson_hist_len(nx, ny, depth), fvlib.wide_anderson_scratch_len(nx, ny, depth)
            good = dict(depth=depth, start=2, hist=fake, hist_len=need_h, astate=fake)
            assert call(None, C.byref(A(**good)), fake, need_s) == E_STATE
            for bad in (dict(depth=-1), dict(depth=17), dict(start=0), dict(start=-3), dict(astate=None), dict(hist=None),
                        dict(hist_len=need_h - 1), dict(hist_len=0)):
                assert call(hp, C.byref(A(**dict(good, **bad))), fake, need_s) == E_ARG, bad
            if depth < 16:                                      # a history and a scratch for depth, asked for depth + 1
                assert call(hp, C.byref(A(**dict(good, depth=depth + 1))), fake, 1 << 40) == E_ARG
                assert call(hp, C.byref(A(**dict(good, depth=depth + 1, hist_len=1 << 40))), fake, need_s) == E_ARG
            assert call(hp, C.byref(A(**good)), None, need_s) == E_ARG
            assert call(hp, C.byref(A(**good)), fake, need_s - 1) == E_ARG
            assert call(hp, C.byref(A(**good)), fake, 0) == E_ARG
            # a refused call leaves the handle as it was
            assert (h.mixing, h.depth, h.hist, h.astate, h.mscr) == (0, 0, None, None, None)
            # everything in order: the block is in the handle, and the iteration has three more launches
            assert L.ldc_fv_wide_launches(hp, 12) == 11 + 5 * 12
            assert call(hp, C.byref(A(**good)), fake, need_s) == 0
            assert (h.mixing, h.depth, h.start, h.hist, h.astate, h.mscr) == (1, depth, 2, fake, fake, fake)
            assert L.ldc_fv_wide_launches(hp, 12) == 11 + 5 * 12 + 3
            assert L.ldc_fv_wide_launches(hp, 4000) == 11 + 5 * 1000 + 3 and L.ldc_fv_wide_launches(hp, 0) == E_ARG
            # depth 0 detaches (it needs neither history nor scratch, but its words are still checked), and so does NULL
            assert call(hp, C.byref(A(depth=0, start=0, hist=None, hist_len=0, astate=fake)), None, 0) == E_ARG
            assert call(hp, C.byref(A(depth=0, start=1, hist=None, hist_len=0, astate=None)), None, 0) == E_ARG
            assert h.mixing == 1
            assert call(hp, C.byref(A(depth=0, start=1, hist=None, hist_len=0, astate=fake)), None, 0) == 0
            assert (h.mixing, h.depth, h.start, h.hist, h.astate, h.mscr) == (0, 0, 0, None, None, None)
            assert L.ldc_fv_wide_launches(hp, 12) == 11 + 5 * 12
            assert call(hp, C.byref(A(**good)), fake, need_s) == 0 and h.mixing == 1
            assert call(hp, None, None, 0) == 0
            assert (h.mixing, h.depth, h.hist) == (0, 0, None) and L.ldc_fv_wide_launches(hp, 12) == 11 + 5 * 12
        assert (h.nx, h.ny, h.device, h.graph, h.G) == (nx, ny, 63, 0, fvlib.wide_groups(nx, ny))
    with pytest.raises(Exception, match="ldc_fv_wide_set_anderson"):
        fvlib.wide_set_anderson(None, A(depth=1, start=1, hist=fake, hist_len=1 << 40, astate=fake), fake, 1 << 40)


def test_launch_counts_of_a_batch_with_and_without_mixing(fvlib):
    L = fvlib.lib()
    b = HostBatch(n=3, maxit=1000, device=63, graph=0)
    bp = C.c_void_p(C.addressof(b))
    assert L.ldc_fv_wide_batch_launches(bp, 12) == 11 + 5 * 12
    b.mixing = 1                                                 # what create sets when a trial has a block
    assert L.ldc_fv_wide_batch_launches(bp, 12) == 11 + 5 * 12 + 3
    assert L.ldc_fv_wide_batch_launches(bp, 4000) == 11 + 5 * 1000 + 3
    assert L.ldc_fv_wide_batch_launches(bp, 0) == E_ARG
    # create reads the blocks of host-side handles and stops at the device
    hs = [_wide(fvlib, 16, 16), _wide(fvlib, 37, 50)]
    A = fvlib.Anderson
    need_h, need_s = fvlib.anderson_hist_len(37, 50, 3), fvlib.wide_anderson_scratch_len(37, 50, 3)
    assert L.ldc_fv_wide_set_anderson(C.c_void_p(C.addressof(hs[1])),
                                      C.byref(A(depth=3, start=2, hist=8, hist_len=need_h, astate=8)), 8, need_s) == 0
    out = C.c_void_p()
    lst = (C.c_void_p * 2)(*[C.addressof(h) for h in hs])
    assert L.ldc_fv_wide_batch_create(lst, 2, 8, 1 << 20, C.byref(out)) in (E_NODEVICE, E_STATE) and not out.value


# ------------------------------------------------------------------------------------------- parameters, launcher
def test_parameter_surface(monkeypatch):
    from solvers.datastructures import FVFSGParameters, FVParameters
    from solvers.fv.batched import BatchedFVSolver
    from solvers.fv.fsg import FVFSGSolver
    from solvers.fv.solver import ACCELERATIONS, FVSolver
    from solvers.spectral import ldc_lib
    assert ACCELERATIONS == ("none", "anderson", "anderson_chip") and FVParameters().acceleration == "none"
    ml = FVParameters(acceleration="anderson_chip", anderson_depth=8, mapping="chip").to_mlflow()
    assert (ml["acceleration"], ml["anderson_depth"], ml["anderson_start"]) == ("anderson_chip", 8, 10)
    assert FVFSGParameters(acceleration="anderson_chip").acceleration == "anderson_chip"        # levels inherit
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)        # every ValueError comes before the device
    base = dict(name="fv", Re=100.0, nx=16, ny=16)
    for bad, word in ((dict(acceleration="anderson_chip"), "mapping"),
                      (dict(acceleration="anderson_chip", mapping="cu"), "anderson_chip.*mapping='cu'"),
                      (dict(acceleration="anderson", mapping="chip"), "anderson"),
                      (dict(acceleration="anderson", mapping="shared"), "anderson.*shared"),
                      (dict(acceleration="anderson_chip", mapping="chip", anderson_depth=17), "anderson_depth"),
                      (dict(acceleration="anderson_chip", mapping="chip", anderson_start=0), "anderson_start"),
                      (dict(acceleration="anderson_wide", mapping="chip"), "acceleration")):
        with pytest.raises(ValueError, match=word):
            FVSolver(**dict(base, **bad))
    for ok in (dict(mapping="chip"), dict(mapping="shared"), dict(mapping="chip", nx=1024, ny=8, anderson_depth=16),
               dict(mapping="shared", nx=300, ny=260)):
        with pytest.raises(ldc_lib.LdcError, match="no CPU fallback"):
            FVSolver(**dict(base, acceleration="anderson_chip", **ok))
    with pytest.raises(ldc_lib.LdcError, match="no CPU fallback"):
        BatchedFVSolver([dict(base, mapping="shared", acceleration="anderson_chip"), dict(base, mapping="shared")])
    for mapping in ("chip", "shared"):
        with pytest.raises(ldc_lib.LdcError, match="no CPU fallback"):
            FVFSGSolver(**dict(base, mapping=mapping, nx=64, ny=64, acceleration="anderson_chip"))
    with pytest.raises(ValueError, match="mapping"):
        FVFSGSolver(**dict(base, nx=64, ny=64, acceleration="anderson_chip"))


def test_launcher_override_composes():
    from utilities.config import compose as Cmp
    comp = Cmp.Composer(PKG / "conf")
    over = ["+solver.mapping=chip", "+solver.acceleration=anderson_chip", "+solver.anderson_depth=10"]
    for solver in ("fv", "fv/fsg"):
        base = Cmp.resolve(Cmp.compose_job(comp, [f"solver={solver}", "N=16"], []))["solver"]
        got = Cmp.resolve(Cmp.compose_job(comp, [f"solver={solver}", "N=16"] + over, []))["solver"]
        assert got == dict(base, mapping="chip", acceleration="anderson_chip", anderson_depth=10)
