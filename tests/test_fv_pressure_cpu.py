"""The consistent pressure equation of chip and shared finite-volume trials (pressure_equation="consistent",
ldc_fv_wide_set_pressure), CPU side: the NumPy statement of the CG loop against a direct dense solve, its iteration counts,
mass conservation, the outer iteration counts of the restatement, the reference mode bit for bit, the C ABI without a device,
the parameter surface and the two-budget retry loops on a fake device."""
import ctypes as C
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
from fv_consistent_numpy import FVConsistentState  # noqa: E402
from fv_numpy import FVState  # noqa: E402

from conftest import PKG  # noqa: E402

E_ARG, E_STATE = -1, -2
SHAPES = [(16, 16, 100.0), (24, 16, 400.0)]
KW = dict(linear_solver_tol=1e-9, convection_scheme="TVD")


@pytest.fixture(scope="module")
def fvlib():
    import __graft_entry__ as g
    g.build()
    from solvers.fv import ldc_fv_lib
    return ldc_fv_lib


# ------------------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("nx,ny,Re", SHAPES)
def test_cg_follows_the_direct_solve_and_conserves_mass(nx, ny, Re):
    """CG at 1e-13 and the dense solve of the pinned system give the same 20 iterations to 1e-12 (measured: < 1e-15); no
    solve takes more than 40 CG iterations (measured: <= 28); and after every iteration |div mdot| <= 2 pressure_tol |b|."""
    tol = 1e-13
    cg = FVConsistentState(nx, ny, Re, pressure_solver="cg", pressure_tol=tol, **KW)
    direct = FVConsistentState(nx, ny, Re, pressure_solver="direct", **KW)
    for k in range(20):
        row = cg.step()
        direct.step()
        du, dp = np.max(np.abs(cg.u - direct.u)), np.max(np.abs(cg.p - direct.p))
        bound = 2 * tol * cg.last["bnorm"]
        print(f"{nx}x{ny} iteration {k}: CG {cg.cg_iters[-1]}, |du| {du:.1e}, |dp| {dp:.1e}, |div| {row[3]:.1e} "
              f"(bound {bound:.1e})")
        assert du <= 1e-12 and dp <= 1e-12 and np.max(np.abs(cg.v - direct.v)) <= 1e-12
        assert row[3] <= bound
    assert max(cg.cg_iters) <= 40 and cg.cg_caps == 0 and len(cg.cg_iters) == 20


@pytest.mark.parametrize("nx,ny,Re", SHAPES)
def test_mass_conservation_at_the_default_tolerance(nx, ny, Re):
    o = FVConsistentState(nx, ny, Re, **KW)
    for _ in range(20):
        row = o.step()
        assert row[3] <= 2 * o.pressure_tol * o.last["bnorm"]
    assert max(o.cg_iters) <= 40


def test_dense_operator_is_the_matrix_free_one_and_singular_on_constants():
    o = FVConsistentState(13, 9, 100.0, **KW)
    o.run(3)
    wx, wy = o.last["wx"], o.last["wy"]
    A = o.dense(wx, wy)
    x = np.random.default_rng(0).standard_normal((9, 13))
    assert np.allclose(A @ x.ravel(), o.apply(wx, wy, x).ravel(), rtol=0, atol=1e-14 * np.abs(A).max() * np.abs(x).max() * 8)
    assert np.array_equal(A, A.T) and np.max(np.abs(A @ np.ones(A.shape[0]))) <= 1e-15 * np.abs(A).max() * 8
    assert abs(np.sum(o.last["b"])) <= 1e-15 * np.sum(np.abs(o.last["b"]))            # the compatibility rule


@pytest.mark.parametrize("nx,ny,want", [(8, 8, 410), (16, 16, 660), (24, 16, 625)])
def test_outer_iteration_counts_of_the_restatement(nx, ny, want):
    """Re = 100, TVD, 0.4 / 0.2, tolerance 1e-6, linear_solver_tol 1e-9: the counts of the table in DESIGN.md section 7."""
    o = FVConsistentState(nx, ny, 100.0, **KW)
    rec = o.run(5000, tol=1e-6)
    print(f"{nx}x{ny}: {len(rec)} iterations, CG at most {max(o.cg_iters)}")
    assert len(rec) == want
    assert max(o.cg_iters) <= 40


def test_reference_mode_is_fvstate_bit_for_bit():
    a = FVConsistentState(16, 12, 400.0, pressure_equation="reference", **KW)
    b = FVState(16, 12, 400.0, **KW)
    ra, rb = a.run(15), b.run(15)
    assert np.array_equal(ra, rb)
    for k in ("u", "v", "p", "fx", "fy"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert a.cg_iters == []


def test_a_cap_hit_is_counted_and_the_iterate_accepted():
    o = FVConsistentState(16, 16, 100.0, pressure_max_iters=3, **KW)
    rec = o.run(5)
    assert o.cg_iters == [3] * 5 and o.cg_caps == 5 and np.all(np.isfinite(rec))


# ------------------------------------------------------------------------------------------- C ABI
class HostWide(C.Structure):
    """The library's host-side ``struct ldc_fv_wide`` (csrc/ldc_fv_wide.hip): the descriptor, the scratch, the work-groups
    of a sweep, pressure_max_iters, the device, the two switches, the mixing block, the (empty) list of captured graphs,
    the pressure block and the pressure budget."""
    _fields_ = ([(n, C.c_int) for n in ("nx", "ny", "scheme", "rec_cap", "warmup", "maxit")]
                + [("rest", C.c_double * 21), ("scr", C.c_void_p), ("G", C.c_int), ("pmax", C.c_int), ("device", C.c_int),
                   ("graph", C.c_short), ("mixing", C.c_short), ("mix", C.c_double * 4), ("graphs", C.c_double * 4),
                   ("tol", C.c_double), ("stats", C.c_void_p), ("pbudget", C.c_int)])


def test_pressure_entries_are_declared_exported_and_bound(fvlib):
    hdr = (ROOT / "include" / "ldc_fv.h").read_text()
    L = fvlib.lib()
    for name in ("ldc_fv_wide_set_pressure", "ldc_fv_wide_set_pressure_budget", "ldc_fv_wide_batch_set_pressure_budget"):
        assert name in fvlib.EXPORTS and re.search(rf"int {name}\(", hdr), name
        assert getattr(L, name).restype is C.c_int
    val = lambda name: int(re.search(rf"#define {name} \(?(-?\d+)", hdr).group(1))        # noqa: E731
    assert val("LDC_FV_WIDE_PRESSURE_LAUNCHES") == fvlib.WIDE_PRESSURE_LAUNCHES == 7
    assert val("LDC_FV_WIDE_PRESSURE_SCRATCH_LEN") == fvlib.WIDE_PRESSURE_SCRATCH_LEN == 4
    assert val("LDC_FV_WIDE_PRESSURE_BUDGET_DEFAULT") == fvlib.WIDE_PRESSURE_BUDGET_DEFAULT
    assert (val("LDC_FV_PRESSURE_REFERENCE"), val("LDC_FV_PRESSURE_CONSISTENT")) == (0, 1)
    assert fvlib.PRESSURE_MODES == dict(reference=0, consistent=1)
    assert C.sizeof(fvlib.Pressure) == 16
    # what does not change: the work vectors, the problem, the table entry
    assert val("LDC_FV_NWORK") == 32 and C.sizeof(fvlib.Problem) == 24 + 72 + 96
    assert val("LDC_FV_WIDE_BATCH_ENTRY_BYTES") == 256


def test_set_pressure_validation_and_launch_counts_need_no_device(fvlib):
    L = fvlib.lib()
    P = fvlib.Pressure
    fake = 8                                                     # never dereferenced: nothing is launched or copied
    call = L.ldc_fv_wide_set_pressure
    assert HostWide.pmax.offset == 204 and HostWide.mix.offset == 216 and HostWide.tol.offset == 280
    h = HostWide(nx=16, ny=16, scheme=1, rec_cap=4, warmup=10, maxit=1000, G=1, device=63, pbudget=12)
    hp = C.c_void_p(C.addressof(h))
    good = dict(mode=1, max_iters=200, tol=1e-8)
    assert call(None, C.byref(P(**good)), fake, 4) == E_STATE
    for bad in (dict(mode=2), dict(mode=-1), dict(max_iters=0), dict(tol=0.0), dict(tol=1.0), dict(tol=-1e-8),
                dict(tol=float("nan"))):
        assert call(hp, C.byref(P(**dict(good, **bad))), fake, 4) == E_ARG, bad
    assert call(hp, C.byref(P(**good)), None, 4) == E_ARG and call(hp, C.byref(P(**good)), fake, 3) == E_ARG
    assert (h.pmax, h.tol, h.stats) == (0, 0.0, None)            # a refused call leaves the handle as it was
    assert L.ldc_fv_wide_launches(hp, 12) == 11 + 5 * 12
    assert L.ldc_fv_wide_set_pressure_budget(hp, 8) == E_ARG     # a reference handle has no such budget
    assert call(hp, C.byref(P(**good)), fake, 4) == 0
    assert (h.pmax, h.tol, h.stats, h.pbudget) == (200, 1e-8, fake, 12)
    # faces | init | np x 7 | pfinish replace faces | gemm x 4
    assert L.ldc_fv_wide_launches(hp, 12) == 9 + 5 * 12 + 7 * 12
    assert L.ldc_fv_wide_set_pressure_budget(hp, 0) == E_ARG and L.ldc_fv_wide_set_pressure_budget(None, 8) == E_STATE
    assert L.ldc_fv_wide_set_pressure_budget(hp, 8) == 0 and L.ldc_fv_wide_launches(hp, 12) == 9 + 5 * 12 + 7 * 8
    assert L.ldc_fv_wide_set_pressure_budget(hp, 4000) == 0 and L.ldc_fv_wide_launches(hp, 12) == 9 + 5 * 12 + 7 * 200
    h.mixing = 1
    assert L.ldc_fv_wide_launches(hp, 2000) == 9 + 5 * 1000 + 7 * 200 + 3
    h.mixing = 0
    # back to the reference equation: by mode, and by NULL
    assert call(hp, C.byref(P(mode=0, max_iters=0, tol=0.0)), None, 0) == 0
    assert (h.pmax, h.stats) == (0, None) and L.ldc_fv_wide_launches(hp, 12) == 11 + 5 * 12
    assert call(hp, C.byref(P(**good)), fake, 4) == 0 and h.pmax == 200
    assert call(hp, None, None, 0) == 0 and h.pmax == 0
    assert L.ldc_fv_wide_batch_set_pressure_budget(None, 8) == E_STATE
    # a batch of consistent trials shares one pressure_max_iters (checked before the device is asked for)
    a, b = (HostWide(nx=16, ny=16, scheme=1, rec_cap=4, warmup=10, maxit=1000, G=1, device=63, pmax=m) for m in (200, 100))
    out = C.c_void_p()
    lst = (C.c_void_p * 2)(C.addressof(a), C.addressof(b))
    assert L.ldc_fv_wide_batch_create(lst, 2, C.c_void_p(fake), 1 << 20, C.byref(out)) == E_ARG
    b.pmax = 0                                                   # a batch may mix both modes
    assert L.ldc_fv_wide_batch_create(lst, 2, C.c_void_p(fake), 1 << 20, C.byref(out)) in (-3, E_STATE)
    assert not out.value


# ------------------------------------------------------------------------------------------- parameters
def test_parameter_surface(monkeypatch):
    from solvers.datastructures import FVParameters
    from solvers.fv.solver import FVSolver
    from solvers.spectral import ldc_lib
    p = FVParameters()
    assert (p.pressure_equation, p.pressure_tol, p.pressure_max_iters, p.pressure_budget) == ("reference", 1e-8, 200, 12)
    ml = FVParameters(mapping="chip", pressure_equation="consistent", pressure_tol=1e-10).to_mlflow()
    assert (ml["pressure_equation"], ml["pressure_tol"], ml["pressure_max_iters"]) == ("consistent", 1e-10, 200)
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)        # every ValueError comes before the device
    base = dict(name="fv", Re=100.0, nx=16, ny=16)
    with pytest.raises(ValueError, match="mapping=chip"):
        FVSolver(**dict(base, pressure_equation="consistent"))
    with pytest.raises(ValueError, match="mapping=chip"):
        FVSolver(**dict(base, mapping="cu", pressure_equation="consistent"))
    for bad, word in ((dict(pressure_equation="exact"), "pressure_equation"), (dict(pressure_tol=0.0), "pressure_tol"),
                      (dict(pressure_tol=2.0), "pressure_tol"), (dict(pressure_max_iters=0), "pressure_max_iters"),
                      (dict(pressure_budget=0), "pressure_budget")):
        with pytest.raises(ValueError, match=word):
            FVSolver(**dict(base, mapping="chip", **bad))
    for ok in (dict(mapping="chip"), dict(mapping="shared"), dict(mapping="chip", nx=1024, ny=8),
               dict(mapping="shared", acceleration="anderson_chip", vortex_metrics="chip")):
        with pytest.raises(ldc_lib.LdcError, match="no CPU fallback"):
            FVSolver(**dict(base, pressure_equation="consistent", **ok))


def test_the_launcher_composes_the_keys():
    sys.path.insert(0, str(PKG))
    from utilities.config import compose as Cmp
    comp = Cmp.Composer(PKG / "conf")
    plain = Cmp.resolve(Cmp.compose_job(comp, ["solver=fv", "N=16"], []))
    over = ["+solver.mapping=chip", "+solver.pressure_equation=consistent", "+solver.pressure_tol=1e-10"]
    got = Cmp.resolve(Cmp.compose_job(comp, ["solver=fv", "N=16"] + over, []))
    assert got["solver"] == dict(plain["solver"], mapping="chip", pressure_equation="consistent", pressure_tol=1e-10)
    assert "pressure_equation" not in plain["solver"]


# ------------------------------------------------------------------------------------------- the retry loops
class FakeDevice:
    """A trial whose iteration i needs ``lin[i]`` BiCGSTAB and ``cg[i]`` CG iterations.  An enqueue completes iterations
    until one needs more than a budget (overflow 1: BiCGSTAB, which comes first; 2: CG; that iteration has changed nothing),
    the latch iteration, or all it was given."""

    def __init__(self, lin, cg, caps=(1000, 200), latch_at=None):
        self.lin, self.cg, self.caps, self.latch_at = list(lin), list(cg), caps, latch_at
        self.total, self.calls = 0, []

    def step(self, m, lin_budget, cg_budget):
        self.calls.append((self.total, m, lin_budget, cg_budget))
        rows, overflow, latch = [], 0, 0
        for _ in range(m):
            if min(lin_budget, self.caps[0]) < min(self.lin[self.total], self.caps[0]):
                overflow = 1
                break
            if min(cg_budget, self.caps[1]) < min(self.cg[self.total], self.caps[1]):
                overflow = 2
                break
            rows.append([float(self.total)] * 8)
            self.total += 1
            if self.latch_at is not None and self.total == self.latch_at:
                latch = 1
                break
        return np.array(rows).reshape(-1, 8), latch, 0, self.total, overflow


def test_two_budget_retry_loop_doubles_the_right_budget_and_loses_nothing():
    from solvers.fv.solver import advance_with_budgets
    d = FakeDevice(lin=[3, 4, 9, 9, 20, 5], cg=[10, 30, 10, 10, 10, 70])
    rows, latch, nan, total, budgets, retries = advance_with_budgets(d.step, 0, 6, (4, 24), (1000, 200))
    assert (latch, nan, total, budgets, retries) == (0, 0, 6, (32, 96), (3, 2))
    assert rows[:, 0].tolist() == [0, 1, 2, 3, 4, 5]                       # every iteration once, in order
    assert d.calls == [(0, 6, 4, 24), (1, 5, 4, 48), (2, 4, 8, 48), (2, 4, 16, 48), (4, 2, 32, 48), (5, 1, 32, 96)]
    # the caps, the latch, and a device that does not keep the protocol
    d = FakeDevice(lin=[2, 2], cg=[5000, 2], caps=(1000, 10))
    _, _, _, total, budgets, retries = advance_with_budgets(d.step, 0, 2, (12, 3), (1000, 10))
    assert (total, budgets, retries) == (2, (12, 10), (0, 2))              # 3 -> 6 -> 10, where the cap hit is accepted
    d = FakeDevice(lin=[2] * 10, cg=[2] * 10, latch_at=4)
    rows, latch, _, total, budgets, retries = advance_with_budgets(d.step, 0, 10, (12, 24), (1000, 200))
    assert (latch, total, budgets, retries, len(rows)) == (1, 4, (12, 24), (0, 0), 4)
    with pytest.raises(RuntimeError, match="pressure budget"):
        advance_with_budgets(lambda m, a, b: (np.zeros((0, 8)), 0, 0, 0, 2), 0, 2, (4, 10), (1000, 10))
    with pytest.raises(RuntimeError, match="linear budget"):
        advance_with_budgets(lambda m, a, b: (np.zeros((0, 8)), 0, 0, 0, 1), 0, 2, (10, 4), (10, 200))
    with pytest.raises(RuntimeError, match="overflow word"):
        advance_with_budgets(lambda m, a, b: (np.zeros((0, 8)), 0, 0, 0, 3), 0, 2, (4, 4), (10, 10))
    with pytest.raises(RuntimeError, match="no progress"):
        advance_with_budgets(lambda m, a, b: (np.zeros((0, 8)), 0, 0, 0, 0), 0, 2, (4, 4), (10, 10))


def test_two_budget_retry_loop_of_a_batch():
    from solvers.fv.solver import advance_batch_with_budgets
    devs = [FakeDevice(lin=[3, 3, 3], cg=[10, 40, 10]), FakeDevice(lin=[3, 20, 3], cg=[10, 10, 10]),
            FakeDevice(lin=[1], cg=[1])]
    calls = []

    def step(quotas, lin_budget, cg_budget):
        calls.append((list(quotas), lin_budget, cg_budget))
        out = []
        for d, k in zip(devs, quotas):
            out.append(d.step(k, lin_budget, cg_budget) if k else (np.zeros((0, 8)), 0, 0, d.total, 0))
        return out

    out = advance_batch_with_budgets(step, [0, 0, 0], [3, 3, 0], [(4, 24), (4, 24), (4, 24)], (1000, 200))
    assert calls == [([3, 3, 0], 4, 24), ([2, 2, 0], 8, 48), ([0, 2, 0], 16, 24), ([0, 2, 0], 32, 24)]
    assert [o[3] for o in out] == [3, 3, 0]
    assert [o[4] for o in out] == [(4, 48), (32, 24), (4, 24)] and [o[5] for o in out] == [(0, 1), (3, 0), (0, 0)]
    for q in (0, 1):
        assert out[q][0][:, 0].tolist() == [0, 1, 2]
    assert devs[2].calls == []                                             # quota 0: never touched
