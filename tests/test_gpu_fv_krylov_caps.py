"""CG and BiCGSTAB iterates accepted at a low cap, on the GPU, on grids up to 1024 x 1024 cells: every mapping of the
finite-volume solver against the NumPy restatement run from the same seeded state (tests/fv_krylov_probe.py).

A converged Krylov solve hides a wrong dot product; an iterate accepted after 1, 2 or 3 iterations is a direct function of
alpha, beta and omega.  The chip and shared mappings sum every dot product from per-work-group slots one launch later
(``wide_slot_put`` / ``wide_slot_sum`` of csrc/ldc_fv_wide.hip, csrc/ldc_fv_wide_pressure.inc), the one-CU mapping inside its
work-group (csrc/ldc_fv_kernel.inc, csrc/ldc_fv_cu_pressure.hip).  tests/test_fv_krylov_probe_cpu.py proves for every case here
that the restatement moves by at most 1e-10 under input rounding and that a sum without the first 1/256 of the cells moves it
by at least 1e-7; the tolerance here is 1e-9.  Every capped test also holds the lost-share mutant of the RESTATEMENT against
the device result and asserts that it misses that tolerance: the test would notice such a sum.  No faulty kernel is built.
The two norms of CG's stop test show in no capped iterate; the last tests here set pressure_tol beside a residual instead.

Each test prints its largest error over the tolerance, the mutant's, and the counters (profiles/fv_krylov_caps.md)."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import fv_krylov_probe as P  # noqa: E402

pytestmark = pytest.mark.gpu

BIG = (1024, 1024)
CHIP = dict(mapping="chip", pressure_equation="consistent")
CHIP_REF = dict(mapping="chip", pressure_equation="reference")
CU = dict(mapping="cu", pressure_equation="consistent_cu")
CU_REF = dict(mapping="cu", pressure_equation="reference")
COUNTERS = ("done", "iterations", "nan", "linear_giveups", "linear_iterations", "momentum_solves", "anderson_fallbacks")
PCOUNTERS = ("pressure_iterations", "pressure_solves", "pressure_caps", "pressure_last")


@pytest.fixture(scope="module")
def fv():
    import __graft_entry__ as g
    g.build()
    from solvers.fv.batched import BatchedFVSolver
    from solvers.fv.solver import FVSolver
    return FVSolver, BatchedFVSolver


def _ids(cases):
    return ["x".join(str(c) for c in case[:2]) + "".join(f"-{c}" for c in case[2:]) for case in cases]


def _seed_of(nx, ny):
    """(u, v, p, mdot) of the seeded state, flattened for ``set_state`` (the formula needs only the sizes)."""
    from fv_numpy import FVState
    return P.seeded(FVState(nx, ny, P.RE, **P.SETTINGS))


def _run_seeded(FVSolver, nx, ny, advances=P.K, **kw):
    """The seed through ``set_state``, ``_begin``, then ``advances`` calls of ``_advance(1)``: (rows, state, counters, the
    counters after every call)."""
    s = FVSolver(**P.solver_kwargs(nx, ny, **kw))
    s.set_state(*_seed_of(nx, ny))
    s._begin(1e-30)
    rows, after = [], []
    for k in range(advances):
        r, done, total = s._advance(1)                 # (a cap hit is accepted: no overflow, no retry of the pressure budget)
        assert total == k + 1 and not done and r.shape == (1, 8)
        rows.append(r)
        after.append(s.counters())
    out = (np.concatenate(rows, axis=0), s.state(), s.counters(), after)
    s.close()
    return out


def _errors(rows, st, ref):
    errs = {k: P.rel(st[k], ref[k]) for k in P.FIELDS}
    errs["rows"] = P.rows_rel(rows[:, P.REC_COLS], ref["rows"][:, P.REC_COLS])
    return errs


def _standard_set(what, rows, st, c, ref, mutants):
    """Fields and record rows within 1e-9 of the reference; every mutant of the restatement misses that on a field."""
    assert rows.shape == ref["rows"].shape and np.all(np.isfinite(rows))
    errs = _errors(rows, st, ref)
    away = {w: max(P.rel(st[k], m[k]) for k in P.FIELDS) for w, m in mutants.items()}
    print(f"{what}: error / tolerance {max(errs.values()) / P.TOL:.2e} ({max(errs, key=errs.get)}), mutants / tolerance "
          f"{ {w: float(f'{a / P.TOL:.2e}') for w, a in away.items()} }, {c}")
    for k, e in errs.items():
        assert e <= P.TOL, (what, k, e)
    assert mutants, what
    for w, a in away.items():
        assert a > P.TOL, (what, w, a)
    assert c["nan"] == 0 and c["done"] == 0 and c["iterations"] == P.K and c["momentum_solves"] == 2 * P.K


def _cg_mutants(nx, ny, cap):
    """The lost-share mutants held against the device result: ``rz`` and ``pq``; at 1024 x 1024 (seconds per run) ``rz``."""
    names = ("rz",) if (nx, ny) == BIG else ("rz", "pq")
    return {w: P.capped_reference(nx, ny, "consistent", cap, None, w) for w in names}


def _bicg_mutants(nx, ny, mode):
    names = ("bicg_rho",) if (nx, ny) == BIG else ("bicg_rho", "bicg_rv", "bicg_ts", "bicg_tt")
    return {w: P.capped_reference(nx, ny, mode, None, P.BICG_CAP, w) for w in names}


def _check_cg_capped(FVSolver, nx, ny, cap, mode):
    ref = P.capped_reference(nx, ny, "consistent", cap)
    rows, st, c, _ = _run_seeded(FVSolver, nx, ny, pressure_max_iters=cap, **mode)
    _standard_set(f"{mode['mapping']} {nx}x{ny} cap {cap}", rows, st, c, ref, _cg_mutants(nx, ny, cap))
    assert (c["pressure_iterations"], c["pressure_solves"], c["pressure_caps"], c["pressure_last"]) == (cap * P.K, P.K, P.K, cap)
    assert c["linear_giveups"] == 0 and c["linear_iterations"] == sum(ref["iters"])
    if "pressure_budget_retries" in c:
        assert c["pressure_budget_retries"] == 0


def _check_bicg_capped(FVSolver, monkeypatch, nx, ny, mode, restated):
    import solvers.fv.solver as S
    monkeypatch.setattr(S, "LINEAR_MAX_ITERATIONS", P.BICG_CAP)
    ref = P.capped_reference(nx, ny, restated, None, P.BICG_CAP)
    rows, st, c, _ = _run_seeded(FVSolver, nx, ny, **mode)
    _standard_set(f"{mode['mapping']} {mode['pressure_equation']} {nx}x{ny} BiCGSTAB cap {P.BICG_CAP}", rows, st, c, ref,
                  _bicg_mutants(nx, ny, restated))
    assert c["linear_giveups"] == ref["exits"].count("cap") == 2 * P.K
    assert c["linear_iterations"] == sum(ref["iters"]) == 2 * P.K * P.BICG_CAP
    if restated == "consistent":                       # the pressure solves converge (restatement: ref["cg_iters"])
        assert c["pressure_solves"] == P.K and c["pressure_caps"] == 0


# ------------------------------------------------------------------------------------------- chip
@pytest.mark.parametrize("nx,ny,cap", P.cg_cases(P.CHIP_SHAPES), ids=_ids(P.cg_cases(P.CHIP_SHAPES)))
def test_chip_cg_iterates_accepted_at_a_cap(fv, nx, ny, cap):
    _check_cg_capped(fv[0], nx, ny, cap, CHIP)


@pytest.mark.parametrize("nx,ny", P.bicg_shapes(P.CHIP_SHAPES, "consistent"), ids=_ids(P.bicg_shapes(P.CHIP_SHAPES, "consistent")))
def test_chip_bicgstab_iterates_accepted_at_a_cap_consistent_equation(fv, monkeypatch, nx, ny):
    _check_bicg_capped(fv[0], monkeypatch, nx, ny, CHIP, "consistent")


@pytest.mark.parametrize("nx,ny", P.bicg_shapes(P.CHIP_SHAPES, "reference"), ids=_ids(P.bicg_shapes(P.CHIP_SHAPES, "reference")))
def test_chip_bicgstab_iterates_accepted_at_a_cap_reference_equation(fv, monkeypatch, nx, ny):
    _check_bicg_capped(fv[0], monkeypatch, nx, ny, CHIP_REF, "reference")


# ------------------------------------------------------------------------------------------- one CU, uniform grid
@pytest.mark.parametrize("nx,ny,cap", P.cg_cases(P.CU_SHAPES), ids=_ids(P.cg_cases(P.CU_SHAPES)))
def test_one_cu_cg_iterates_accepted_at_a_cap(fv, nx, ny, cap):
    """``fv_cu_pressure_kernel``."""
    _check_cg_capped(fv[0], nx, ny, cap, CU)


@pytest.mark.parametrize("nx,ny", P.CU_SHAPES, ids=_ids(P.CU_SHAPES))
def test_one_cu_bicgstab_iterates_accepted_at_a_cap_consistent_equation(fv, monkeypatch, nx, ny):
    """``fv_cu_pressure_kernel``."""
    _check_bicg_capped(fv[0], monkeypatch, nx, ny, CU, "consistent")


@pytest.mark.parametrize("nx,ny", P.CU_SHAPES, ids=_ids(P.CU_SHAPES))
def test_one_cu_bicgstab_iterates_accepted_at_a_cap_reference_equation(fv, monkeypatch, nx, ny):
    """``fv_kernel``."""
    _check_bicg_capped(fv[0], monkeypatch, nx, ny, CU_REF, "reference")


# ------------------------------------------------------------------------------------------- shared batch
def _snapshot(s):
    return dict(s.state(), history=np.array(s.history), ctrl=s.t["ctrl"].cpu().numpy().copy(), counters=s.counters())


@pytest.mark.parametrize("cap", [1, 3, P.UNCAPPED], ids=["cap1", "cap3", "uncapped"])
def test_a_shared_batch_of_552_work_groups_is_its_lone_chip_runs_bit_for_bit(fv, cap):
    """272 x 260, 1024 x 72 and 8 x 1024 with the consistent equation and 37 x 50 with the reference's, seeded, two iterations
    in the launches of ONE batch: 256 + 256 + 32 + 8 = 552 work-groups per sweep launch.  Every trial is its lone chip run bit
    for bit (fields, history, ctrl, counters); at cap 1 and cap 3 the consistent trials are also within 1e-9 of the capped
    restatement, and its ``rz`` mutant is not.  The library takes ONE ``pressure_max_iters`` per batch (``ldc_fv_wide_batch_create``
    refuses a mix), so the caps are three batches of the same four trials, not one batch with three caps."""
    FVSolver, BatchedFVSolver = fv
    shapes = [((272, 260), "consistent"), ((37, 50), "reference"), ((1024, 72), "consistent"), ((8, 1024), "consistent")]
    trials = [P.solver_kwargs(nx, ny, pressure_equation=eq, max_iterations=P.K,
                              **(dict(pressure_max_iters=cap) if eq == "consistent" else {})) for (nx, ny), eq in shapes]
    batch = BatchedFVSolver([dict(t, mapping="shared") for t in trials])
    for s in batch.solvers:
        s.set_state(*_seed_of(s.nx, s.ny))
    batch.solve()
    assert batch.errors == {} and len(batch) == 4
    for q, (s, t) in enumerate(zip(batch.solvers, trials)):
        got = _snapshot(s)
        lone = FVSolver(**dict(t, mapping="chip"))
        lone.set_state(*_seed_of(lone.nx, lone.ny))
        lone.solve()
        want = _snapshot(lone)
        lone.close()
        assert got["history"].shape == (P.K, 8)
        for k in P.FIELDS + ("history", "ctrl"):
            assert np.array_equal(got[k], want[k]), (q, k)
        for k in COUNTERS + (PCOUNTERS if s.consistent else ()):
            assert got["counters"][k] == want["counters"][k], (q, k)
        what = f"shared {s.nx}x{s.ny} {t['pressure_equation']} cap {cap}"
        if s.consistent and cap != P.UNCAPPED:
            ref = P.capped_reference(s.nx, s.ny, "consistent", cap)
            _standard_set(what, got["history"], got, got["counters"], ref,
                          dict(rz=P.capped_reference(s.nx, s.ny, "consistent", cap, None, "rz")))
            c = got["counters"]
            assert (c["pressure_iterations"], c["pressure_solves"], c["pressure_caps"], c["pressure_last"]) == (cap * P.K, P.K, P.K, cap)
        else:
            print(what, got["counters"])
            assert got["counters"]["nan"] == 0 and got["counters"].get("pressure_caps", 0) == 0
    batch.close()


# ------------------------------------------------------------------------------------------- converged counts
def _check_counts(FVSolver, nx, ny, mode):
    """Uncapped, pressure_tol 1e-13: after each of three ``_advance(1)`` calls ``pressure_last`` is the restatement's count of
    that solve within max(1, 10 x the restatement's own sensitivity); a wrong |r|^2 moves the stop."""
    ref = P.converged_reference(nx, ny)
    bound = P.count_bound(nx, ny)
    rows, st, c, after = _run_seeded(FVSolver, nx, ny, advances=P.COUNT_K, **mode)
    last = [a["pressure_last"] for a in after]
    errs = {k: P.rel(st[k], ref[k]) for k in P.FIELDS}
    print(f"{mode['mapping']} {nx}x{ny}: CG counts {last}, restatement {list(ref['cg_iters'])}, bound {bound}; BiCGSTAB "
          f"{c['linear_iterations']}, restatement {sum(ref['iters'])}; fields / tolerance {max(errs.values()) / P.TOL:.2e}; {c}")
    for k, (got, want) in enumerate(zip(last, ref["cg_iters"])):
        assert abs(got - want) <= bound, (k, got, want)
    assert c["pressure_caps"] == 0 and c["pressure_solves"] == P.COUNT_K and c["nan"] == 0 and c["linear_giveups"] == 0
    assert c["pressure_iterations"] == sum(last) and np.all(np.isfinite(rows))


@pytest.mark.parametrize("nx,ny", P.CHIP_COUNT_SHAPES, ids=_ids(P.CHIP_COUNT_SHAPES))
def test_chip_converged_cg_counts_are_the_restatements(fv, nx, ny):
    _check_counts(fv[0], nx, ny, CHIP)


@pytest.mark.parametrize("nx,ny", P.CU_COUNT_SHAPES, ids=_ids(P.CU_COUNT_SHAPES))
def test_one_cu_converged_cg_counts_are_the_restatements(fv, nx, ny):
    _check_counts(fv[0], nx, ny, CU)


# ------------------------------------------------------------------------------------------- the stop test at a threshold
def _check_threshold(FVSolver, nx, ny, mode):
    """|r|^2 and |b|^2 enter only the stop test: no capped iterate shows them, and a share of 1/256 does not move the counts of
    a run converged to 1e-13.  With pressure_tol set beside |r_5| / |b| of the first solve (``threshold_case``: at least 1e-6
    away, relative, where the device's fields follow the restatement to 1e-9) the whole sums stop at iteration 5 and |b| without
    a share goes on (``bb``), or go on where |r_5| without a share stops (``rr``): the device's count is the restatement's
    exactly, and not the mutant's."""
    case = P.threshold_case(nx, ny)
    for which in ("rr", "bb"):
        want, mutant = P.threshold_count(nx, ny, which), P.threshold_count(nx, ny, which, which)
        _, _, c, _ = _run_seeded(FVSolver, nx, ny, advances=1, pressure_tol=case["tol_" + which], **mode)
        print(f"{mode['mapping']} {nx}x{ny} pressure_tol {case['tol_' + which]:.6e} ({which}): CG count {c['pressure_last']}, "
              f"restatement {want}, its {which} mutant {mutant}")
        assert want != mutant and P.THRESHOLD_K in (want, mutant)
        assert c["pressure_last"] == want and c["pressure_caps"] == 0 and c["pressure_solves"] == 1 and c["nan"] == 0


@pytest.mark.parametrize("nx,ny", P.CHIP_COUNT_SHAPES, ids=_ids(P.CHIP_COUNT_SHAPES))
def test_chip_cg_stops_where_the_whole_norms_say(fv, nx, ny):
    _check_threshold(fv[0], nx, ny, CHIP)


@pytest.mark.parametrize("nx,ny", P.CU_COUNT_SHAPES, ids=_ids(P.CU_COUNT_SHAPES))
def test_one_cu_cg_stops_where_the_whole_norms_say(fv, nx, ny):
    _check_threshold(fv[0], nx, ny, CU)
