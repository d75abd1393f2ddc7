"""Post-processing and prolongation of chip and shared finite-volume trials (ldc_fv_wide_post_enqueue,
ldc_fv_wide_prolong_enqueue, ``vortex_metrics="chip"``), CPU side: the C ABI against the header, argument validation
without a device on host-side stand-ins for the handles, the parameter surface and the routing of ``postprocess`` and
``prolong``."""
import ctypes as C
import re
import sys
from pathlib import Path
from types import SimpleNamespace

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))

from conftest import PKG  # noqa: E402,F401

NEW = ("ldc_fv_wide_post_enqueue", "ldc_fv_wide_post_launches", "ldc_fv_wide_prolong_enqueue")
E_ARG, E_STATE, E_NODEVICE = -1, -2, -3


@pytest.fixture(scope="module")
def fvlib():
    import __graft_entry__ as g
    g.build()
    from solvers.fv import ldc_fv_lib
    return ldc_fv_lib


# ------------------------------------------------------------------------------------------- C ABI
def test_entries_are_declared_exported_and_bound(fvlib):
    hdr = (ROOT / "include" / "ldc_fv.h").read_text()
    L = fvlib.lib()
    for name in NEW:
        assert name in fvlib.EXPORTS and re.search(rf"int {name}\(", hdr), name
        assert getattr(L, name).restype is C.c_int and getattr(L, name).argtypes is not None
    assert len(L.ldc_fv_wide_post_enqueue.argtypes) == 5 and len(L.ldc_fv_wide_prolong_enqueue.argtypes) == 3
    # every function the header declares is exported, and nothing else is listed
    declared = set(re.findall(r"^int (ldc_fv_\w+)\(", hdr, flags=re.M))
    assert declared == set(fvlib.EXPORTS)
    assert int(re.search(r"#define LDC_FV_VERSION (\d+)", hdr).group(1)) == fvlib.VERSION == 2
    assert L.ldc_fv_version() == 2


def test_scratch_macro_matches_its_python_twin(fvlib):
    hdr = (ROOT / "include" / "ldc_fv.h").read_text()
    groups = re.search(r"#define LDC_FV_WIDE_GROUPS\(nx, ny\) (.*)", hdr).group(1)
    scratch = re.search(r"#define LDC_FV_WIDE_POST_SCRATCH_LEN\(nx, ny\) (.*)", hdr).group(1)
    want = {(8, 8): 12, (37, 50): 12 * 8, (1024, 1024): 12 * 256}
    for (nx, ny), n in want.items():
        g = eval(groups.replace("(int64_t)", "").replace("/", "//").replace("?", " and ").replace(":", " or "),
                 dict(nx=nx, ny=ny))
        assert eval(scratch.replace("LDC_FV_WIDE_GROUPS(nx, ny)", str(g))) == fvlib.wide_post_scratch_len(nx, ny) == n


# ------------------------------------------------------------------------------------------- validation, no device
class HostWide(C.Structure):
    """The library's host-side ``struct ldc_fv_wide`` (csrc/ldc_fv_wide.hip): the trial's descriptor, the scratch of the
    solve, the work-groups of a sweep, the device, the graph switch and room for the captured graphs.  Validation reads
    nx, ny, dx, dy and the device; nothing here is ever launched."""
    _fields_ = ([(n, C.c_int) for n in ("nx", "ny", "scheme", "rec_cap", "warmup", "maxit")]
                + [(n, C.c_double) for n in ("dx", "dy", "rho", "mu", "alpha_uv", "alpha_p", "lin_tol", "tol", "lid")]
                + [(n, C.c_void_p) for n in ("ulid", "Qx", "lamx", "Qy", "lamy", "u", "v", "p", "mdot", "work", "rec",
                                             "ctrl", "scr")]
                + [(n, C.c_int) for n in ("G", "pad", "device", "graph")] + [("graphs", C.c_void_p * 4)])


def _handle(fvlib, nx, ny, Lx=1.0, Ly=1.0):
    # device -7: where a device exists the call ends at "not the handle's device", where none does at "no device"
    return HostWide(nx=nx, ny=ny, scheme=1, rec_cap=4, warmup=10, maxit=1000, dx=Lx / nx, dy=Ly / ny, rho=1.0, mu=0.01,
                    alpha_uv=0.4, alpha_p=0.2, lin_tol=1e-9, tol=1e-6, lid=1.0, G=fvlib.wide_groups(nx, ny), device=-7)


def _post(fvlib, **change):
    fake = 8                                                     # never dereferenced: validation comes first
    good = dict(Sx=fake, lamx=fake, Sy=fake, lamy=fake, ix_lt=4, ix_gt=4, jy_lt=4, jy_gt=4, psi=fake, omega=fake,
                result=fake)
    return fvlib.Post(**dict(good, **change))


def test_post_argument_validation_needs_no_device(fvlib):
    L = fvlib.lib()
    fake, big = 8, 1 << 20
    for nx, ny in ((16, 16), (300, 260), (1024, 1024)):
        h = _handle(fvlib, nx, ny)
        hp = C.c_void_p(C.addressof(h))
        need = fvlib.wide_post_scratch_len(nx, ny)
        assert L.ldc_fv_wide_post_enqueue(None, C.byref(_post(fvlib)), fake, big, None) == E_STATE
        assert L.ldc_fv_wide_post_enqueue(hp, None, fake, big, None) == E_ARG
        for bad in (dict(Sx=None), dict(lamx=None), dict(Sy=None), dict(lamy=None), dict(psi=None), dict(omega=None),
                    dict(result=None), dict(ix_lt=-1), dict(ix_gt=-1), dict(jy_lt=-1), dict(jy_gt=-2)):
            assert L.ldc_fv_wide_post_enqueue(hp, C.byref(_post(fvlib, **bad)), fake, big, None) == E_ARG, bad
        assert L.ldc_fv_wide_post_enqueue(hp, C.byref(_post(fvlib)), None, big, None) == E_ARG
        assert L.ldc_fv_wide_post_enqueue(hp, C.byref(_post(fvlib)), fake, need - 1, None) == E_ARG
        assert L.ldc_fv_wide_post_enqueue(hp, C.byref(_post(fvlib)), fake, 0, None) == E_ARG
        # everything the host can check is in order: what is left is the device
        assert L.ldc_fv_wide_post_enqueue(hp, C.byref(_post(fvlib)), fake, need, None) in (E_NODEVICE, E_STATE)
        assert L.ldc_fv_wide_post_launches(hp) == 7                  # omega, four GEMMs, extrema, result
    assert L.ldc_fv_wide_post_launches(None) == E_ARG


def test_prolong_argument_validation_needs_no_device(fvlib):
    L = fvlib.lib()
    c, f = _handle(fvlib, 150, 130), _handle(fvlib, 300, 260)
    cp, fp = C.c_void_p(C.addressof(c)), C.c_void_p(C.addressof(f))
    assert L.ldc_fv_wide_prolong_enqueue(None, fp, None) == E_STATE
    assert L.ldc_fv_wide_prolong_enqueue(cp, None, None) == E_STATE
    assert L.ldc_fv_wide_prolong_enqueue(None, None, None) == E_STATE
    assert L.ldc_fv_wide_prolong_enqueue(fp, fp, None) == E_ARG                      # the same handle twice
    for Lx, Ly in ((2.0, 1.0), (1.0, 0.5), (1.0 + 1e-9, 1.0)):                        # two domains
        w = _handle(fvlib, 40, 40, Lx, Ly)
        assert L.ldc_fv_wide_prolong_enqueue(C.c_void_p(C.addressof(w)), fp, None) == E_ARG, (Lx, Ly)
        assert L.ldc_fv_wide_prolong_enqueue(fp, C.c_void_p(C.addressof(w)), None) == E_ARG, (Lx, Ly)
    # one domain to the rounding of L / n, any two sizes, either direction, equal sizes: what is left is the device
    e = _handle(fvlib, 300, 260)
    for a, b in ((cp, fp), (fp, cp), (C.c_void_p(C.addressof(e)), fp)):
        assert L.ldc_fv_wide_prolong_enqueue(a, b, None) in (E_NODEVICE, E_STATE)
    g = _handle(fvlib, 37, 50, 2.0, 0.5)
    k = _handle(fvlib, 1024, 8, 2.0, 0.5)
    assert L.ldc_fv_wide_prolong_enqueue(C.c_void_p(C.addressof(g)), C.c_void_p(C.addressof(k)), None) in (E_NODEVICE, E_STATE)


# ------------------------------------------------------------------------------------------- parameters
def test_parameter_surface(monkeypatch):
    from solvers.datastructures import FVParameters
    from solvers.fv.solver import VORTEX_METRICS, FVSolver
    from solvers.spectral import ldc_lib
    import torch
    monkeypatch.delenv("LDC_FV_VORTEX_METRICS", raising=False)
    assert VORTEX_METRICS == ("host", "device", "chip")
    assert FVParameters().vortex_metrics == "host"                        # the default did not move
    assert "vortex_metrics" not in FVParameters(vortex_metrics="chip", mapping="chip").to_mlflow()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)        # every ValueError comes before the device
    base = dict(name="fv", Re=100.0, nx=16, ny=16)
    for ok in (dict(mapping="chip", nx=300, vortex_metrics="chip"), dict(mapping="shared", nx=300, vortex_metrics="chip"),
               dict(mapping="chip", vortex_metrics="chip"), dict(mapping="shared", nx=8, ny=1024, vortex_metrics="chip"),
               dict(mapping="chip", nx=1024, ny=1024, vortex_metrics="chip")):
        with pytest.raises(ldc_lib.LdcError, match="no CPU fallback"):
            FVSolver(**dict(base, **ok))
    with pytest.raises(ValueError, match="mapping='cu'"):
        FVSolver(**dict(base, mapping="cu", vortex_metrics="chip"))
    with pytest.raises(ValueError, match="mapping='cu'"):
        FVSolver(**dict(base, vortex_metrics="chip"))
    with pytest.raises(ValueError, match="vortex_metrics"):
        FVSolver(**dict(base, vortex_metrics="gpu"))
    with pytest.raises(ValueError, match="vortex_metrics"):
        FVSolver(**dict(base, mapping="chip", vortex_metrics="gpu"))
    # the refusals of "device" above 256 cells stay
    for mapping in ("chip", "shared"):
        with pytest.raises(ValueError, match="vortex_metrics='device'"):
            FVSolver(**dict(base, mapping=mapping, nx=300, vortex_metrics="device"))
    # the environment chooses where the keyword is not given, and is refused alike
    monkeypatch.setenv("LDC_FV_VORTEX_METRICS", "chip")
    assert FVParameters().vortex_metrics == "chip"
    with pytest.raises(ValueError, match="mapping='cu'"):
        FVSolver(**base)
    with pytest.raises(ldc_lib.LdcError, match="no CPU fallback"):
        FVSolver(**dict(base, mapping="chip", nx=300))
    with pytest.raises(ldc_lib.LdcError, match="no CPU fallback"):
        FVSolver(**dict(base, vortex_metrics="host"))                    # the keyword wins


# ------------------------------------------------------------------------------------------- routing
def _fake(mapping, nx, ny, vortex_metrics="host"):
    """What the routing reads of an FVSolver, as its constructor sets it."""
    chip = mapping in ("chip", "shared")
    return SimpleNamespace(params=SimpleNamespace(vortex_metrics=vortex_metrics, mapping=mapping), chip=chip, nx=nx, ny=ny,
                           _has_cu_handle=not chip or max(nx, ny) <= 256)


def test_postprocess_routing():
    from solvers.fv.solver import post_route
    route = lambda s: post_route(s.params.vortex_metrics, s._has_cu_handle)        # noqa: E731
    # "chip" asks for the chain at every size; a trial without a one-CU handle gets it whatever it asks for
    for mapping in ("chip", "shared"):
        assert route(_fake(mapping, 24, 24, "chip")) == "chip"
        assert route(_fake(mapping, 256, 256, "chip")) == "chip"
        assert route(_fake(mapping, 300, 260, "chip")) == "chip"
        assert route(_fake(mapping, 300, 260, "host")) == "chip"               # streamfunction() / vorticity()
        assert route(_fake(mapping, 8, 257, "host")) == "chip"
        assert route(_fake(mapping, 256, 256, "host")) == "cu"                  # as before
        assert route(_fake(mapping, 24, 24, "device")) == "cu"
    assert route(_fake("cu", 24, 24, "device")) == "cu" and route(_fake("cu", 256, 256, "host")) == "cu"


def test_prolong_routing():
    from solvers.fv.solver import prolong_route
    route = lambda c, f: prolong_route(c._has_cu_handle, f._has_cu_handle, c.chip, f.chip)        # noqa: E731
    small = {m: _fake(m, 128, 128) for m in ("cu", "chip", "shared")}
    big = {m: _fake(m, 512, 512) for m in ("chip", "shared")}
    for c in small.values():                          # both have a one-CU handle: as before, whatever their mapping
        for f in small.values():
            assert route(c, f) == "cu"
    for c in list(big.values()) + [small["chip"], small["shared"]]:
        for f in big.values():
            assert route(c, f) == "chip"              # coarse -> fine, and continuation at equal size
    assert route(big["chip"], small["shared"]) == "chip"        # (a restriction is a prolongation too)
    for c, f in ((small["cu"], big["chip"]), (small["cu"], big["shared"]), (big["chip"], small["cu"])):
        with pytest.raises(ValueError, match="give the coarse trial mapping='chip'"):
            route(c, f)
