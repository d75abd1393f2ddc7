"""Anderson acceleration of the finite-volume SIMPLE iteration, CPU side: the NumPy restatement
(tests/fv_anderson_numpy.py) against a least-squares solve, on the 16 x 16 cavity and on a lid at rest, the parameter
surface, and the C ABI of ldc_fv_anderson_enqueue without a device."""
import ctypes as C
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
import fv_anderson_numpy as AA  # noqa: E402
from fv_numpy import FVState  # noqa: E402

from conftest import PKG  # noqa: E402

# the cases tests/test_gpu_fv_anderson.py compares with the restatement: (nx, ny, FVState keywords, depth, iterations)
GPU_CASES = {
    "13x17-tvd": (13, 17, dict(convection_scheme="TVD"), 3, 12),
    "24x16-upwind-saad": (24, 16, dict(convection_scheme="Upwind", corner_treatment="saad"), 3, 12),
    "8x8-depth16": (8, 8, dict(convection_scheme="TVD"), 16, 12),
}
GPU_START = 2
COND_MAX = 1e6


def restated(case):
    nx, ny, kw, depth, K = GPU_CASES[case]
    s = FVState(nx, ny, 100.0, **kw)
    rows, mixer = AA.run(s, K, depth=depth, start=GPU_START)
    return s, rows, mixer


# ------------------------------------------------------------------------------------------- the small system
@pytest.mark.parametrize("m", [1, 3, 5, 16])
@pytest.mark.parametrize("seed", [0, 1])
def test_gamma_is_the_least_squares_solution_of_the_regularised_system(m, seed):
    """(A + lambda I) gamma = b are the normal equations of min |[dF; sqrt(lambda) I] gamma - [f; 0]|.  Gaussian
    columns of 300 entries have cond(A) < 1e2 (asserted), so both solutions carry errors of a few eps cond(A) ~ 1e-13
    relative: 1e-10 leaves three digits."""
    rng = np.random.default_rng(seed)
    dF, f = rng.standard_normal((300, m)), rng.standard_normal(300)
    A, b = AA.regularised(dF, f)
    assert np.linalg.cond(A) < 1e2
    lam = AA.LAMBDA * np.trace(dF.T @ dF) / m
    want = np.linalg.lstsq(np.vstack([dF, np.sqrt(lam) * np.eye(m)]), np.concatenate([f, np.zeros(m)]), rcond=None)[0]
    got = AA.cholesky_solve(A, b)
    err = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
    print(f"m={m} seed={seed}: cond {np.linalg.cond(A):.1f}, max relative difference {err:.2e}")
    assert err <= 1e-10


def test_mixer_solves_that_system_in_ring_order():
    """Seeded histories through the Mixer itself, the ring wrapping twice: every gamma it used is lstsq's on the columns
    it held, in slot order, and the weights of the g's sum to 1 (a constant entry of g stays constant)."""
    rng = np.random.default_rng(5)
    n_cells, depth = 20, 3
    L = 3 * n_cells + 31
    mx = AA.Mixer(n_cells, depth, start=2)
    x = rng.standard_normal(L)
    x[7] = 2.5
    for it in range(1, 10):
        g = 0.5 * x + 0.1 * rng.standard_normal(L)
        g[7] = 2.5
        before = len(mx.gammas)
        x = mx.mix(g, it)
        assert x[2 * n_cells] == 0.0 or it < 3
        assert abs(x[7] - 2.5) < 1e-12
        if len(mx.gammas) > before:
            m = mx.ncol
            dF, f = mx.dF[: 3 * n_cells, :m], mx.fp[: 3 * n_cells]
            lam = AA.LAMBDA * np.trace(dF.T @ dF) / m
            want = np.linalg.lstsq(np.vstack([dF, np.sqrt(lam) * np.eye(m)]), np.concatenate([f, np.zeros(m)]),
                                   rcond=None)[0]
            assert np.max(np.abs(mx.gammas[-1] - want)) <= 1e-9 * np.max(np.abs(want))
    assert len(mx.gammas) == 7 and mx.ncol == depth and mx.fallbacks == 0        # mixed at it = 3 ... 9


def test_a_singular_system_takes_the_fallback():
    A = np.array([[1.0, 1.0], [1.0, 1.0]])
    assert AA.cholesky_solve(A, np.ones(2)) is None
    assert AA.cholesky_solve(np.zeros((2, 2)), np.zeros(2)) is None
    assert AA.cholesky_solve(np.array([[np.nan]]), np.ones(1)) is None
    assert AA.cholesky_solve(np.array([[4.0]]), np.array([2.0]))[0] == 0.5


# ------------------------------------------------------------------------------------------- around the SIMPLE iteration
@pytest.fixture(scope="module")
def runs16():
    """16 x 16, Re = 100, the YAML's settings (TVD, 0.4 / 0.2, 1e-9), tolerance 1e-6: plain and depth 5 from 10."""
    plain, acc = FVState(16, 16, 100.0), FVState(16, 16, 100.0)
    p0 = []
    rows_plain, _ = AA.run(plain, 20000, depth=0, tol=1e-6)
    mixer = AA.Mixer(16 * 16, 5, 10)
    rows = []
    for k in range(20000):                              # AA.run's loop, looking at p[0] after every iteration
        rows.append(acc.step())
        p0.append(acc.p[0, 0])
        if k >= 10 and rows[-1][0] < 1e-6:
            break
        AA.unpack(acc, mixer.mix(AA.pack(acc), k + 1))
        p0.append(acc.p[0, 0])
    return plain, rows_plain, acc, np.array(rows), mixer, np.array(p0)


def test_restatement_halves_the_iterations_at_16(runs16):
    plain, rows_plain, acc, rows, mixer, p0 = runs16
    duv = max(float(np.max(np.abs(acc.u - plain.u))), float(np.max(np.abs(acc.v - plain.v))))
    print(f"16x16 Re=100: plain {len(rows_plain)} iterations, depth 5 {len(rows)}; cond {mixer.cond:.2e}, "
          f"fallbacks {mixer.fallbacks}, max|du|,|dv| {duv:.2e}")
    assert len(rows_plain) < 20000 and rows_plain[-1][0] < 1e-6
    assert len(rows) < 20000 and rows[-1][0] < 1e-6 and np.all(np.isfinite(rows))
    assert 2 * len(rows) <= len(rows_plain)
    assert np.all(p0 == 0.0)
    assert duv < 1e-3                                    # the same fixed point, stopped elsewhere


def test_run_agrees_with_the_loop_of_the_fixture(runs16):
    _, _, acc, rows, _, _ = runs16
    again = FVState(16, 16, 100.0)
    rows2, _ = AA.run(again, 40, depth=5, start=10)
    assert np.array_equal(rows2, rows[:40])


@pytest.mark.parametrize("rest", ["lid_velocity", "profile"])
def test_a_lid_at_rest_takes_the_fallback_without_a_nan(rest):
    """f = 0 from the first iteration: A = 0, lambda = 0, the first pivot is 0.  ``profile``: the lid profile zeroed at
    lid velocity 1, which keeps the viscosity mu = rho U L / Re positive as ldc_fv_create asks (the GPU test's way)."""
    s = FVState(8, 8, 100.0, lid_velocity=0.0) if rest == "lid_velocity" else FVState(8, 8, 100.0)
    s.ulid[:] = 0.0
    rows, mixer = AA.run(s, 30, depth=3, start=2, tol=1e-6)
    assert len(rows) == 11 and rows[-1][0] == 0.0        # the latch fires at the warm-up
    assert mixer.fallbacks == 8 and mixer.ncol == 0      # iterations 3 ... 10: a column, a zero pivot
    assert np.all(np.isfinite(rows[:, :4])) and np.all(AA.pack(s) == 0.0)


@pytest.mark.parametrize("case", sorted(GPU_CASES))
def test_gpu_cases_are_well_conditioned(case):
    """tests/test_gpu_fv_anderson.py allows 1e-9 max(1, cond) max|field|: cond must stay small for that to say much."""
    s, rows, mixer = restated(case)
    nx, ny, _, depth, K = GPU_CASES[case]
    print(f"{case}: cond {mixer.cond:.3e}, fallbacks {mixer.fallbacks}, columns {mixer.ncol}")
    assert mixer.cond <= COND_MAX
    assert mixer.fallbacks == 0 and len(mixer.gammas) == K - 2 and mixer.ncol == min(depth, K - 2)
    assert np.all(np.isfinite(rows)) and np.all(np.isfinite(AA.pack(s))) and s.p[0, 0] == 0.0


# ------------------------------------------------------------------------------------------- parameters, configuration
def test_parameter_surface(monkeypatch):
    from solvers.datastructures import FVFSGParameters, FVParameters
    from solvers.fv.solver import FVSolver
    p = FVParameters()
    assert (p.acceleration, p.anderson_depth, p.anderson_start) == ("none", 5, 10)
    ml = FVParameters(acceleration="anderson", anderson_depth=8).to_mlflow()
    assert (ml["acceleration"], ml["anderson_depth"], ml["anderson_start"]) == ("anderson", 8, 10)
    assert FVFSGParameters(acceleration="anderson").acceleration == "anderson"        # levels inherit
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)                    # ValueError comes before the device
    for bad in (dict(acceleration="aa"), dict(anderson_depth=0), dict(anderson_depth=17), dict(anderson_start=0)):
        with pytest.raises(ValueError, match=next(iter(bad))):
            FVSolver(name="fv", Re=100.0, nx=16, ny=16, **bad)


def test_launcher_override_carries_the_keys():
    from utilities.config import compose as Cmp
    comp = Cmp.Composer(PKG / "conf")
    base = Cmp.resolve(Cmp.compose_job(comp, ["solver=fv", "N=16"], []))["solver"]
    over = ["+solver.acceleration=anderson", "+solver.anderson_depth=8"]
    for solver in ("fv", "fv/fsg"):
        base = Cmp.resolve(Cmp.compose_job(comp, [f"solver={solver}", "N=16"], []))["solver"]
        got = Cmp.resolve(Cmp.compose_job(comp, [f"solver={solver}", "N=16"] + over, []))["solver"]
        assert got == dict(base, acceleration="anderson", anderson_depth=8)


# ------------------------------------------------------------------------------------------- C ABI
@pytest.fixture(scope="module")
def fvlib():
    import __graft_entry__ as g
    g.build()
    from solvers.fv import ldc_fv_lib
    return ldc_fv_lib


def test_anderson_entry_is_declared_exported_and_bound(fvlib):
    hdr = (ROOT / "include" / "ldc_fv.h").read_text()
    assert "ldc_fv_anderson_enqueue" in fvlib.EXPORTS
    assert re.search(r"int ldc_fv_anderson_enqueue\(ldc_fv \*const \*hs, const struct ldc_fv_anderson \*acc, int n, "
                     r"int n_iters, void \*stream\);", hdr)
    L = fvlib.lib()
    assert L.ldc_fv_anderson_enqueue.restype is C.c_int
    val = lambda name: int(re.search(rf"#define {name} (\d+)", hdr).group(1))        # noqa: E731
    assert L.ldc_fv_version() == fvlib.VERSION == val("LDC_FV_VERSION")
    assert fvlib.ANDERSON_LAUNCH_MAX == val("LDC_FV_ANDERSON_LAUNCH_MAX")
    assert fvlib.ANDERSON_MAX_DEPTH == val("LDC_FV_ANDERSON_MAX_DEPTH") == AA.MAX_DEPTH
    assert fvlib.ANDERSON_STATE_LEN == val("LDC_FV_ANDERSON_STATE_LEN")
    assert 32 * fvlib.ANDERSON_LAUNCH_MAX + 4 <= 3600           # the trials' blocks travel as kernel arguments
    body = re.search(r"struct ldc_fv_anderson \{(.*?)\};", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\*?(\w+)\s*;", body) == [f[0] for f in fvlib.Anderson._fields_]
    assert C.sizeof(fvlib.Anderson) == 32
    assert fvlib.anderson_hist_len(13, 17, 3) == 9 * (3 * 13 * 17 + 17 * 14 + 18 * 13)


class HostHandle(C.Structure):
    """The library's host-side ``struct ldc_fv`` (csrc/ldc_fv_common.inc), for the checks that read a handle's record
    capacity and sizes: no device pointer in it is ever followed by validation."""
    _fields_ = [("dev", C.c_void_p), ("ctrl", C.c_void_p), ("rec_cap", C.c_int), ("device", C.c_int), ("nx", C.c_int),
                ("ny", C.c_int), ("dx", C.c_double), ("dy", C.c_double)]


def test_anderson_argument_validation_needs_no_device(fvlib):
    L = fvlib.lib()
    fake = 8                                                     # never dereferenced: these checks come first
    A = fvlib.Anderson
    good = dict(depth=3, start=2, hist=fake, hist_len=1 << 40, astate=fake)
    hs = (C.c_void_p * 2)(fake, fake)
    acc = (A * 2)(A(**good), A(**good))
    call = L.ldc_fv_anderson_enqueue
    assert call(None, acc, 1, 1, None) == -1
    assert call(hs, None, 1, 1, None) == -1
    assert call(hs, acc, 0, 1, None) == -1
    assert call(hs, acc, -2, 1, None) == -1
    assert call(hs, acc, 1, 0, None) == -1
    assert call((C.c_void_p * 2)(None, fake), acc, 2, 1, None) == -2        # a NULL handle: LDC_E_STATE
    # what needs a handle's record capacity and sizes: a host-side handle of 13 x 17 cells, 16 record rows
    h = HostHandle(dev=fake, ctrl=fake, rec_cap=16, device=-7, nx=13, ny=17, dx=1 / 13, dy=1 / 17)
    hs = (C.c_void_p * 2)(C.addressof(h), C.addressof(h))
    need = fvlib.anderson_hist_len(13, 17, 3)
    good = dict(good, hist_len=need)
    for bad in (dict(depth=-1), dict(depth=17), dict(start=0), dict(astate=None), dict(hist=None),
                dict(hist_len=need - 1), dict(depth=4)):
        acc = (A * 2)(A(**good), A(**dict(good, **bad)))
        assert call(hs, acc, 2, 1, None) == -1, bad
    acc = (A * 2)(A(**good), A(depth=0, start=1, hist=None, hist_len=0, astate=fake))      # depth 0 needs no history
    assert call(hs, acc, 2, 17, None) == -1                                                # n_iters > rec_cap
    # in list order, and a trial's handle before its block: trial 0 in order, trial 1 a NULL handle with a bad block
    bad_second = (A * 2)(A(**good), A(**dict(good, depth=17)))
    assert call((C.c_void_p * 2)(C.addressof(h), None), bad_second, 2, 16, None) == -2
    # everything the host can check is in order: what is left is the device (none here: LDC_E_NODEVICE, or a handle of
    # device -7: LDC_E_STATE), before any launch
    assert call(hs, acc, 2, 16, None) in (-2, -3)
    with pytest.raises(ValueError):
        fvlib.anderson_enqueue([fake, fake], [A(**good)], 1, None)
