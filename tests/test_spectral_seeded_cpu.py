"""The seeded-state matrix of tests/test_gpu_spectral_seeded.py, qualified on the CPU: for every case (size, ny, pressure
mode, parameters, K) the oracle's own rounding floor lies a hundred times below the GPU tolerances, and every arithmetic
fault of spectral_seed.MutantSG moves the end state a hundred times above them.  And the gap this closes, pinned: from
rest the same faults stay below the state tolerance."""
import numpy as np
import pytest

from oracle import ldc_oracle as orc
from spectral_seed import KINDS, MutantSG, ReorderedSG, cpu_cases, oracle_rows
from test_gpu_xcd import rel

ALL = cpu_cases()
_REF = {}


def reference(c):
    """The unmutated oracle's end state and records of a case: computed once, shared, never modified."""
    if c.id not in _REF:
        o, _ = c.oracle()
        rows = oracle_rows(o, c.K, c.diagnostics)
        for a in (o.u, o.v, o.p, rows):
            a.setflags(write=False)
        _REF[c.id] = (o.u, o.v, o.p, rows)
    return _REF[c.id]


def test_the_matrix_names_every_case_once():
    ids = [c.id for c in ALL]
    assert len(ids) == len(set(ids)) and len({c.seed for c in ALL}) == len(ALL)


@pytest.mark.parametrize("c", [ALL[0], ALL[20], ALL[-1]], ids=lambda c: c.id)
def test_mutant_without_a_fault_is_the_oracle_bit_for_bit(c):
    """spectral_seed._residual restates OracleSG.residual term by term: with no fault it must be the same arithmetic."""
    u, v, p, rows = reference(c)
    m, _ = c.oracle(MutantSG)
    got = oracle_rows(m, c.K, c.diagnostics)
    assert np.array_equal(m.u, u) and np.array_equal(m.v, v) and np.array_equal(m.p, p) and np.array_equal(got, rows)


@pytest.mark.parametrize("c", ALL, ids=lambda c: c.id)
def test_rounding_floor_is_a_hundredth_of_the_gpu_tolerances(c):
    """Every contraction summed in reversed order: state <= 1e-14 absolute, every record column <= 1e-12 relative."""
    u, v, p, rows = reference(c)
    r, _ = c.oracle(ReorderedSG)
    got = oracle_rows(r, c.K, c.diagnostics)
    assert rows.shape == (c.K, 8) and np.all(np.isfinite(rows)) and np.all(np.isfinite(got))
    floor = max(np.max(np.abs(r.u - u)), np.max(np.abs(r.v - v)), np.max(np.abs(r.p - p)))
    recs = max(rel(got[:, col], rows[:, col]) for col in range(8))
    print(f"{c.id}: state floor {floor:.2e}, record floor {recs:.2e}")
    assert floor <= 1e-14
    assert recs <= 1e-12


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("c", ALL, ids=lambda c: c.id)
def test_every_fault_moves_the_state_a_hundred_tolerances(c, kind):
    u, v, p, _ = reference(c)
    m, _ = c.oracle(MutantSG)
    m.kind = kind
    for _ in range(c.K):
        m.step()
    moved = max(np.max(np.abs(m.u - u)), np.max(np.abs(m.v - v)), np.max(np.abs(m.p - p)))
    print(f"{c.id} {kind}: {moved:.2e}")
    assert moved >= 1e-10


def test_from_rest_the_same_faults_stay_below_the_state_tolerance():
    """The gap: at N = 96, 14 iterations from rest (what test_short_run_records_vs_oracle runs), dropping the convective terms
    on the whole lower half of the cavity, or v u_y in a centre tile, changes u and v by less than the 1e-12 a GPU test allows
    -- the flow still sits under the lid.  From-rest tests cannot see such a kernel; the seeded ones above see it by 1e-10 at
    the least."""
    N, Re, K = 96, 400.0, 14
    o = orc.OracleSG(N, Re)
    for _ in range(K):
        o.step()
    for kind in ("noconv_lower", "vuy_tile"):
        m = MutantSG(N, Re)
        m.kind = kind
        for _ in range(K):
            m.step()
        du, dv = np.max(np.abs(m.u - o.u)), np.max(np.abs(m.v - o.v))
        print(f"from rest {kind}: u {du:.2e} v {dv:.2e}")
        assert du < 1e-12 and dv < 1e-12, kind
