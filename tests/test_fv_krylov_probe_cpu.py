"""The references of tests/test_gpu_fv_krylov_caps.py can carry its assertions (CPU, NumPy only; tests/fv_krylov_probe.py).

For every (shape, cap) the GPU file uses: the restatement from the seeded state is finite and ends every capped solve at its
cap; restating it with linear_solver_tol 1e-13 instead of 1e-12 moves u, v, p, mdot by at most 1e-10 (relative to each field's
largest entry); every lost-share mutant of a dot product that enters the iterate moves one of them by at least 1e-7.  The GPU
tolerance of 1e-9 lies between the two.  The dot products that enter only a stop test (``STOP_ONLY``: ``rr`` and ``bb`` of CG and
the three norms of BiCGSTAB) cannot show in an iterate accepted at a cap: their mutants leave a capped run unchanged bit for bit,
which is asserted.  They do not move the counts of a converged run either (printed below); the CG pair is caught by the threshold
cases of the last test here.  Each test prints its figures (profiles/fv_krylov_caps.md).

At 1024 x 1024 a run takes seconds, so the mutants there are ``rz`` and ``pq`` for CG and ``bicg_rho`` and ``bicg_ts`` for
BiCGSTAB (one dot product of alpha and one of beta / omega each), and the stop-only mutants are left to the other shapes."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import fv_krylov_probe as P  # noqa: E402
from fv_consistent_numpy import FVConsistentState  # noqa: E402
from fv_numpy import FVState  # noqa: E402

ALL_SHAPES = P.CHIP_SHAPES + [s for s in P.CU_SHAPES if s not in P.CHIP_SHAPES]
BIG = (1024, 1024)


def _ids(cases):
    return ["x".join(str(c) for c in case[:2]) + "".join(f"-{c}" for c in case[2:]) for case in cases]


def _finite(r):
    return all(np.all(np.isfinite(r[k])) for k in P.FIELDS) and np.all(np.isfinite(r["rows"]))


# ------------------------------------------------------------------------------------------- the seed and the copies
def test_the_seed_is_developed_and_every_face_flux_takes_both_signs():
    o = FVState(37, 50, P.RE, **P.SETTINGS)
    u, v, p, mdot = P.seeded(o)
    assert p[0] == 0.0 and np.max(np.abs(u)) > 0.4 and np.max(np.abs(v)) > 0.3
    fx, fy = o.fx, o.fy
    assert np.all(fx[:, 0] == 0.0) and np.all(fx[:, -1] == 0.0) and np.all(fy[0, :] == 0.0) and np.all(fy[-1, :] == 0.0)
    for f in (fx[:, 1:-1], fy[1:-1, :]):
        assert (f > 0).any() and (f < 0).any()
    assert np.linalg.norm(o.divergence(fx, fy)) > 1e-3                       # non-solenoidal: the pressure solve has work
    assert np.array_equal(mdot, np.concatenate([fx.ravel(), fy.ravel()]))    # the [fx | fy] layout of include/ldc_fv.h


@pytest.mark.parametrize("nx,ny", [(37, 50), (272, 260)])
def test_the_copied_loops_with_every_sum_whole_are_the_restatement_bit_for_bit(nx, ny):
    """``lost_share(cls, None)``: the copies of ``pcg`` and ``bicgstab`` that the mutants are cut from."""
    for mode, cg_cap, bicg_cap in (("consistent", 3, None), ("consistent", None, P.BICG_CAP), ("reference", None, P.BICG_CAP),
                                   ("consistent", None, None)):
        ref = P.capped_reference(nx, ny, mode, cg_cap, bicg_cap)
        copy = P.capped_reference(nx, ny, mode, cg_cap, bicg_cap, None)
        for k in P.FIELDS + ("rows",):
            assert np.array_equal(copy[k], ref[k]), (mode, cg_cap, bicg_cap, k)
        for k in ("iters", "exits", "cg_iters", "cg_caps"):
            assert copy[k] == ref[k], (mode, cg_cap, bicg_cap, k)


# ------------------------------------------------------------------------------------------- CG accepted at a cap
@pytest.mark.parametrize("nx,ny,cap", P.cg_cases(ALL_SHAPES), ids=_ids(P.cg_cases(ALL_SHAPES)))
def test_cg_capped_references_carry_the_gpu_tolerance(nx, ny, cap):
    ref = P.capped_reference(nx, ny, "consistent", cap)
    assert _finite(ref)
    assert ref["cg_caps"] == P.K and ref["cg_iters"] == (cap,) * P.K          # every pressure solve accepted at the cap
    assert "cap" not in ref["exits"] and len(ref["iters"]) == 2 * P.K         # (the momentum solves converge)
    tight = P.capped_reference(nx, ny, "consistent", cap, None, "none", 1e-13)
    sens = P.distance(tight, ref)
    line = f"cg {nx}x{ny} cap {cap}: sensitivity {max(sens.values()):.1e}"
    assert max(sens.values()) <= P.SENSITIVITY_BOUND, sens
    for which in ("rz", "pq"):
        d = P.distance(P.capped_reference(nx, ny, "consistent", cap, None, which), ref)
        line += f", {which} {max(d.values()):.1e}"
        assert max(d.values()) >= P.MUTANT_BOUND, (which, d)
    if (nx, ny) != BIG:
        for which in ("rr", "bb"):                                              # only the stop test reads them
            m = P.capped_reference(nx, ny, "consistent", cap, None, which)
            assert all(np.array_equal(m[k], ref[k]) for k in P.FIELDS) and m["cg_iters"] == ref["cg_iters"], which
    print(line)


# ------------------------------------------------------------------------------------------- BiCGSTAB ended at a cap
BICG_CASES = [(nx, ny, mode) for mode in ("consistent", "reference") for nx, ny in P.bicg_shapes(ALL_SHAPES, mode)]


@pytest.mark.parametrize("nx,ny,mode", BICG_CASES, ids=_ids(BICG_CASES))
def test_bicgstab_capped_references_carry_the_gpu_tolerance(nx, ny, mode):
    ref = P.capped_reference(nx, ny, mode, None, P.BICG_CAP)
    assert _finite(ref)
    assert ref["exits"] == ("cap",) * (2 * P.K) and ref["iters"] == (P.BICG_CAP,) * (2 * P.K)
    if mode == "consistent":
        assert ref["cg_caps"] == 0 and len(ref["cg_iters"]) == P.K            # (the pressure solves converge)
    tight = P.capped_reference(nx, ny, mode, None, P.BICG_CAP, "none", 1e-13)
    sens = P.distance(tight, ref)
    line = f"bicgstab {mode} {nx}x{ny} cap {P.BICG_CAP}: sensitivity {max(sens.values()):.1e}"
    assert max(sens.values()) <= P.SENSITIVITY_BOUND, sens
    moving = [w for w in P.BICG_MUTANTS if w not in P.STOP_ONLY]
    for which in (("bicg_rho", "bicg_ts") if (nx, ny) == BIG else moving):
        d = P.distance(P.capped_reference(nx, ny, mode, None, P.BICG_CAP, which), ref)
        line += f", {which[5:]} {max(d.values()):.1e}"
        assert max(d.values()) >= P.MUTANT_BOUND, (which, d)
    if (nx, ny) != BIG:
        for which in ("bicg_rr", "bicg_ss", "bicg_bb"):
            m = P.capped_reference(nx, ny, mode, None, P.BICG_CAP, which)
            assert all(np.array_equal(m[k], ref[k]) for k in P.FIELDS) and m["iters"] == ref["iters"], which
    print(line)


def test_the_mutants_are_doubles_of_the_restatement_classes():
    assert issubclass(P.lost_share(FVConsistentState, "rz"), FVConsistentState)
    assert issubclass(P.lost_share(FVState, "bicg_rho"), FVState)
    with pytest.raises(ValueError):
        P.lost_share(FVState, "rz")
    with pytest.raises(ValueError):
        P.lost_share(FVConsistentState, "zz")


# ------------------------------------------------------------------------------------------- converged counts
COUNT_SHAPES = P.CHIP_COUNT_SHAPES + [s for s in P.CU_COUNT_SHAPES if s not in P.CHIP_COUNT_SHAPES]


@pytest.mark.parametrize("nx,ny", COUNT_SHAPES, ids=_ids(COUNT_SHAPES))
def test_converged_counts_and_their_own_sensitivity(nx, ny):
    """The uncapped runs of the count tests: no solve capped, and how far the restatement's own per-solve CG counts move
    between linear_solver_tol 1e-13 and 1e-12 (the GPU bound is max(1, 10 x that)).  Printed beside it, without an assertion:
    what a lost share in |r|^2 (``rr``), ``rz`` or ``pq`` does to the counts."""
    ref = P.converged_reference(nx, ny)
    assert _finite(ref) and ref["cg_caps"] == 0 and "cap" not in ref["exits"]
    assert len(ref["cg_iters"]) == P.COUNT_K and all(1 <= c < P.UNCAPPED for c in ref["cg_iters"])
    sens = P.counts_sensitivity(nx, ny)
    assert sens <= 1                        # ten times more would make the GPU bound wider than the counts themselves vary
    shifts = {w: tuple(P.capped_reference(nx, ny, "consistent", None, None, w, 1e-12, P.COUNT_K)["cg_iters"])
              for w in P.CG_MUTANTS}
    print(f"counts {nx}x{ny}: CG {ref['cg_iters']}, BiCGSTAB {ref['iters']}, sensitivity {sens}, bound "
          f"{P.count_bound(nx, ny)}; mutants {shifts}")


# ------------------------------------------------------------------------------------------- the stop test at a threshold
@pytest.mark.parametrize("nx,ny", COUNT_SHAPES, ids=_ids(COUNT_SHAPES))
def test_a_threshold_beside_the_fifth_residual_tells_a_lost_share_in_either_norm(nx, ny):
    """pressure_tol set beside |r_5| / |b| (``threshold_case``): the restatement stops at 5 where the ``bb`` mutant goes on, and
    goes on where the ``rr`` mutant stops at 5; both settings lie at least THRESHOLD_MARGIN from the residual, and the counts
    do not move when linear_solver_tol goes from 1e-12 to 1e-13."""
    c = P.threshold_case(nx, ny)
    assert 0.0 < c["tol_rr"] < c["rho"] < c["tol_bb"] < 1.0
    assert 0.5 * c["d_rr"] >= P.THRESHOLD_MARGIN and 0.5 * c["d_bb"] >= P.THRESHOLD_MARGIN, c
    got = {(w, lost): P.threshold_count(nx, ny, w, lost) for w in ("rr", "bb") for lost in ("none", w)}
    print(f"threshold {nx}x{ny}: rho {c['rho']:.3e}, lost share of |r_5| {c['d_rr']:.1e}, of |b| {c['d_bb']:.1e}; counts {got}")
    assert got["bb", "none"] == P.THRESHOLD_K and got["bb", "bb"] > P.THRESHOLD_K
    assert got["rr", "none"] > P.THRESHOLD_K and got["rr", "rr"] == P.THRESHOLD_K
    for w in ("rr", "bb"):
        assert P.threshold_count(nx, ny, w, "none", 1e-13) == got[w, "none"], w
