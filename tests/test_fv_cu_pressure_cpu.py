"""The consistent pressure equation of one-CU finite-volume trials (pressure_equation="consistent_cu", ldc_fv_set_pressure,
csrc/ldc_fv_cu_pressure.hip), CPU side: the C ABI without a device on a fake host handle, the parameter surface and the
launcher's keys.  The arithmetic has its CPU statement in tests/fv_consistent_numpy.py (tests/test_fv_pressure_cpu.py)."""
import ctypes as C
import re
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent

from conftest import PKG  # noqa: E402

E_ARG, E_STATE = -1, -2


@pytest.fixture(scope="module")
def fvlib():
    import __graft_entry__ as g
    g.build()
    from solvers.fv import ldc_fv_lib
    return ldc_fv_lib


class HostFv(C.Structure):
    """The library's host-side ``struct ldc_fv`` (csrc/ldc_fv_common.inc): the descriptor in the tail of work, ctrl, the
    record ring's rows, the device, the sizes and, at its end, the pressure mode."""
    _fields_ = [("dev", C.c_void_p), ("ctrl", C.c_void_p), ("rec_cap", C.c_int), ("device", C.c_int), ("nx", C.c_int),
                ("ny", C.c_int), ("dx", C.c_double), ("dy", C.c_double), ("pressure_mode", C.c_int)]


def test_set_pressure_is_declared_exported_and_bound(fvlib):
    hdr = (ROOT / "include" / "ldc_fv.h").read_text()
    L = fvlib.lib()
    assert "ldc_fv_set_pressure" in fvlib.EXPORTS and re.search(r"int ldc_fv_set_pressure\(", hdr)
    assert L.ldc_fv_set_pressure.restype is C.c_int and callable(fvlib.set_pressure)
    val = lambda name: int(re.search(rf"#define {name} \(?(-?\d+)", hdr).group(1))        # noqa: E731
    assert val("LDC_FV_PRESSURE_STATS_LEN") == fvlib.PRESSURE_STATS_LEN == 4
    assert val("LDC_FV_VERSION") == fvlib.VERSION == L.ldc_fv_version() == 2
    assert (val("LDC_FV_PRESSURE_REFERENCE"), val("LDC_FV_PRESSURE_CONSISTENT")) == (0, 1)
    assert "csrc/ldc_fv_cu_pressure.hip" in hdr.split(" *\n", 1)[0]            # the unit list at the head
    assert "The consistent pressure equation of a one-CU trial" in hdr
    # the launch function of the new unit is internal: not in the header
    assert "ldc_fv_cu_pressure_launch" not in hdr
    # the new unit is on the build's source list, a unit of its own
    import __graft_entry__ as g
    assert g.SRC_FV_CU_PRESSURE.name == "ldc_fv_cu_pressure.hip" and g.SRC_FV_CU_PRESSURE.exists()


def test_set_pressure_validation_needs_no_device(fvlib):
    L = fvlib.lib()
    P = fvlib.Pressure
    fake = 8                                                     # never dereferenced by a refused call
    call = L.ldc_fv_set_pressure
    assert HostFv.pressure_mode.offset == 48
    good = dict(mode=1, max_iters=200, tol=1e-8)
    assert call(None, C.byref(P(**good)), fake, 4) == E_STATE
    for start in (0, 1):                                         # from either mode: a refused call leaves the mode alone
        h = HostFv(dev=None, ctrl=None, rec_cap=4, device=63, nx=16, ny=16, dx=1 / 16, dy=1 / 16, pressure_mode=start)
        hp = C.c_void_p(C.addressof(h))
        for bad in (dict(mode=2), dict(mode=-1), dict(max_iters=0), dict(max_iters=-3), dict(tol=0.0), dict(tol=1.0),
                    dict(tol=-1e-8), dict(tol=2.0), dict(tol=float("nan"))):
            assert call(hp, C.byref(P(**dict(good, **bad))), fake, 4) == E_ARG, bad
            assert h.pressure_mode == start, bad
        assert call(hp, C.byref(P(**good)), None, 4) == E_ARG and h.pressure_mode == start
        assert call(hp, C.byref(P(**good)), fake, 3) == E_ARG and h.pressure_mode == start
        assert call(hp, C.byref(P(**good)), fake, 0) == E_ARG and h.pressure_mode == start
    # back to the reference kernel: by mode and by NULL, neither touches the device
    h = HostFv(device=63, nx=16, ny=16, rec_cap=4, pressure_mode=1)
    hp = C.c_void_p(C.addressof(h))
    assert call(hp, C.byref(P(mode=0, max_iters=0, tol=0.0)), None, 0) == 0 and h.pressure_mode == 0
    h.pressure_mode = 1
    assert call(hp, None, None, 0) == 0 and h.pressure_mode == 0
    # the debug kernel is the reference iteration: a consistent handle is refused before anything is launched
    h.pressure_mode = 1
    assert L.ldc_fv_step_debug(hp, 0, None, None) == E_ARG


def test_parameter_surface(monkeypatch):
    from solvers.datastructures import FVParameters
    from solvers.fv import solver as S
    from solvers.spectral import ldc_lib
    assert S.PRESSURE_EQUATIONS == ("reference", "consistent", "consistent_cu")
    ml = FVParameters(pressure_equation="consistent_cu", pressure_tol=1e-10).to_mlflow()
    assert (ml["pressure_equation"], ml["pressure_tol"], ml["pressure_max_iters"]) == ("consistent_cu", 1e-10, 200)
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)        # every ValueError comes before the device
    base = dict(name="fv", Re=100.0, nx=16, ny=16)
    for ok in (dict(), dict(mapping="cu"), dict(mapping="cu", acceleration="anderson"), dict(vortex_metrics="device"),
               dict(nx=256, ny=8)):
        with pytest.raises(ldc_lib.LdcError, match="no CPU fallback"):
            S.FVSolver(**dict(base, pressure_equation="consistent_cu", **ok))
    for mapping in ("chip", "shared"):
        with pytest.raises(ValueError, match="'consistent'"):
            S.FVSolver(**dict(base, mapping=mapping, pressure_equation="consistent_cu"))
    with pytest.raises(ValueError, match="'reference', 'consistent' or 'consistent_cu'"):
        S.FVSolver(**dict(base, pressure_equation="exact"))
    for bad, word in ((dict(pressure_tol=0.0), "pressure_tol"), (dict(pressure_max_iters=0), "pressure_max_iters")):
        with pytest.raises(ValueError, match=word):
            S.FVSolver(**dict(base, pressure_equation="consistent_cu", **bad))
    with pytest.raises(ValueError, match="nx, ny"):          # the one-CU kernel's sizes
        S.FVSolver(**dict(base, pressure_equation="consistent_cu", nx=300))
    # sequenced trials carry the mode to every level
    from solvers.fv.fsg import _LEVEL_FIELDS
    assert "pressure_equation" in _LEVEL_FIELDS and "pressure_tol" in _LEVEL_FIELDS


def test_the_launcher_composes_the_key():
    sys.path.insert(0, str(PKG))
    from utilities.config import compose as Cmp
    comp = Cmp.Composer(PKG / "conf")
    plain = Cmp.resolve(Cmp.compose_job(comp, ["solver=fv", "N=16"], []))
    got = Cmp.resolve(Cmp.compose_job(comp, ["solver=fv", "N=16", "+solver.pressure_equation=consistent_cu"], []))
    assert got["solver"] == dict(plain["solver"], pressure_equation="consistent_cu")
    assert "mapping" not in got["solver"]                    # the default mapping: cu
