"""CPU checks of the finite-volume batch (solvers/fv/batched.py) and of how the launcher forms FV batches (main.py):
the chunk loop with a fake ``step``, the sharing key, and the cap arithmetic.  No GPU, no library."""
import importlib.util

import numpy as np
import pytest

from solvers.fv.batched import run_chunks

from conftest import PKG

SG, FSG, FV = "solvers.spectral.sg.SGSolver", "solvers.spectral.fsg.FSGSolver", "solvers.fv.solver.FVSolver"


class FakeKernel:
    """Stands in for ldc_fv_batch_enqueue + the copies: trial q latches at ``latch[q]`` iterations and reports a NaN at
    ``nan[q]``; row k of a trial is [q, k, 0...].  ``calls`` keeps (live, k) of every step."""

    def __init__(self, n, latch=None, nan=None):
        self.iters = [0] * n
        self.latch, self.nan = latch or {}, nan or {}
        self.calls = []

    def step(self, live, k):
        self.calls.append((list(live), k))
        out = []
        for q in live:
            rows, done, bad = [], 0, 0
            for _ in range(k):
                row = np.zeros(8)
                row[0], row[1] = q, self.iters[q]
                rows.append(row)
                self.iters[q] += 1
                if self.nan.get(q) == self.iters[q]:
                    bad = 1
                    break
                if self.latch.get(q) == self.iters[q]:
                    done = 1
                    break
            out.append((np.array(rows).reshape(-1, 8), done, bad, self.iters[q]))
        return out


def _rows_ok(q, rows, n):
    return rows.shape == (n, 8) and rows[:, 0].tolist() == [q] * n and rows[:, 1].tolist() == list(range(n))


# ------------------------------------------------------------------------------------------------------- chunk loop
def test_caps_are_honoured_exactly_and_chunks_follow_the_smallest_ring_and_remaining_cap():
    k = FakeKernel(3)
    out = run_chunks([8, 8, 8], [5, 20, 13], k.step)
    assert [c[1] for c in k.calls] == [5, 8, 7]                      # 13 is no multiple of the chunk: 5 + 8, then 7 to 20
    assert [c[0] for c in k.calls] == [[0, 1, 2], [1, 2], [1]]
    assert [(latch, nan, total) for latch, nan, total, _ in out] == [(0, 0, 5), (0, 0, 20), (0, 0, 13)]
    assert all(_rows_ok(q, out[q][3], n) for q, n in enumerate((5, 20, 13)))


def test_chunk_length_is_the_smallest_ring_of_the_live_trials():
    k = FakeKernel(2, latch={0: 3})
    out = run_chunks([4, 16], [100, 30], k.step)
    # trial 0 (ring 4) latches in the first chunk; from then on the chunk is trial 1's ring, then its remaining cap
    assert k.calls == [([0, 1], 4), ([1], 16), ([1], 10)]
    assert (out[0][0], out[0][2]) == (1, 3) and (out[1][0], out[1][2]) == (0, 30)
    assert _rows_ok(0, out[0][3], 3) and _rows_ok(1, out[1][3], 30)


def test_latched_capped_and_nan_trials_leave_and_are_never_stepped_again():
    k = FakeKernel(4, latch={0: 11}, nan={2: 3})
    out = run_chunks([8] * 4, [40, 16, 40, 27], k.step)
    lives = [c[0] for c in k.calls]
    assert lives == [[0, 1, 2, 3], [0, 1, 3], [3], [3]]
    assert [c[1] for c in k.calls] == [8, 8, 8, 3]
    assert [(latch, nan, total) for latch, nan, total, _ in out] == [(1, 0, 11), (0, 0, 16), (0, 1, 3), (0, 0, 27)]
    assert all(_rows_ok(q, out[q][3], n) for q, n in enumerate((11, 16, 3, 27)))


def test_a_nan_trial_does_not_stop_the_others():
    k = FakeKernel(3, nan={1: 2}, latch={0: 30, 2: 21})
    out = run_chunks([8, 8, 8], [100, 100, 100], k.step)
    assert out[1][:3] == (0, 1, 2) and len(out[1][3]) == 2
    assert out[0][:3] == (1, 0, 30) and out[2][:3] == (1, 0, 21)
    assert all(1 not in live for live, _ in k.calls[1:])


def test_a_cap_of_zero_is_never_launched_and_no_progress_raises():
    k = FakeKernel(2)
    out = run_chunks([8, 8], [0, 4], k.step)
    assert k.calls == [([1], 4)] and out[0][:3] == (0, 0, 0) and out[0][3].shape == (0, 8)
    with pytest.raises(RuntimeError, match="no progress"):
        run_chunks([8], [4], lambda live, n: [(np.zeros((0, 8)), 0, 0, 0)])


# ------------------------------------------------------------------------------------------------------- launcher
@pytest.fixture(scope="module")
def main():
    spec = importlib.util.spec_from_file_location("ldc_main_fv_batched_under_test", PKG / "main.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _cfg(main, *overrides):
    from utilities.config import compose as C
    return C.resolve(C.compose_job(C.Composer(PKG / "conf"), list(overrides), []))


def test_fv_trials_share_one_key_whatever_their_size_and_parameters(main):
    a = _cfg(main, "solver=fv", "N=32", "Re=100")
    b = _cfg(main, "solver=fv", "N=128", "Re=1000", "solver.convection_scheme=Upwind", "solver.ny=64")
    assert a["solver"]["_target_"] == FV
    assert main.batch_key(a) == main.batch_key(b) == (FV,)
    assert main.batch_key(a) != main.batch_key(_cfg(main, "solver=spectral/sg", "N=32", "Re=100"))


def test_spectral_keys_are_the_tuple_run_group_has_always_built(main):
    for ov in (["solver=spectral/sg", "N=48", "Re=400"], ["solver=spectral/fsg", "N=64", "Re=1000"],
               ["solver=spectral/sg", "N=32", "solver.ny=24"]):
        c = _cfg(main, *ov)
        sv = c["solver"]
        assert sv["_target_"] in (SG, FSG)
        assert main.batch_key(c) == (sv["_target_"], int(c["N"]), int(sv.get("n_levels", 0)), bool(sv.get("diagnostics", True)),
                                     int(sv.get("nx", c["N"])), int(sv.get("ny", c["N"])))
    assert main.batch_key(_cfg(main, "solver=spectral/sg", "N=32")) != main.batch_key(_cfg(main, "solver=spectral/sg", "N=48"))


def test_fv_batches_are_cut_at_256_or_at_the_users_cap(main):
    none = main.batch_limit({}, env={})
    assert none == (64, False)
    assert main.batch_sizes((FV,), 600, *none) == [256, 256, 88]
    assert main.FV_LAUNCH_MAX == 256
    from solvers.fv import ldc_fv_lib as F
    assert main.FV_LAUNCH_MAX == F.LAUNCH_MAX
    cap64 = main.batch_limit({}, env={"LDC_MAX_BATCH": "64"})
    assert cap64 == (64, True)
    assert main.batch_sizes((FV,), 600, *cap64) == [64] * 9 + [24]
    assert main.batch_sizes((FV,), 600, *main.batch_limit({"batch_trials": 300}, env={})) == [300, 300]
    assert main.batch_sizes((FV,), 600, *main.batch_limit({"batch_trials": 300}, env={"LDC_MAX_BATCH": "1"})) == []
    assert main.batch_sizes((FV,), 1, *none) == [] and main.batch_sizes((FV,), 2, *none) == [2]
    assert main.batch_sizes((FV,), 257, *none) == [256, 1]


def test_spectral_batches_are_cut_as_before(main):
    none, cap8 = (64, False), (8, True)
    assert main.batch_sizes((SG, 32, 0, True, 32, 32), 600, *none) == [256, 256, 88]       # M = 33 <= 44: the trial-per-CU kernel
    assert main.batch_sizes((SG, 64, 0, True, 64, 64), 150, *none) == [64, 64, 22]
    assert main.batch_sizes((FSG, 64, 2, True, 64, 64), 20, *cap8) == [8, 8, 4]
    assert main.batch_sizes((SG, 32, 0, True, 32, 32), 20, *cap8) == [8, 8, 4]
    assert main.batch_sizes((SG, 32, 0, True, 32, 32), 20, 1, True) == []
    assert main.batch_sizes(("some.other.Solver", 32, 0, True, 32, 32), 20, *none) == []
