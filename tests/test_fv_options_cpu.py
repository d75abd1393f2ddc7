"""What FVSolver and FVFSGSolver answer to their options, combination by combination, against the record of
tests/golden/g18_fv_options.npz (tests/golden/make_golden_fv_options.py: made from the commit before the checks moved to
solvers/fv/options.py).  The first check that fails decides the message, so the order of the checks is pinned with them."""
import importlib.util
import json

import numpy as np
import pytest

from conftest import GOLDEN


@pytest.fixture(scope="module")
def recorder():
    spec = importlib.util.spec_from_file_location("make_golden_fv_options", GOLDEN / "make_golden_fv_options.py")
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


@pytest.fixture(scope="module")
def recomputed(recorder):
    return recorder.tables()


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN / "g18_fv_options.npz") as z:
        return {name: z[name] for name in z.files}


def _first_difference(cases, got, want):
    for case, g, w in zip(cases, got, want):
        if g != w:
            return f"{case[0]}(**{case[1]!r})\n  now:      {g}\n  recorded: {w}"
    return None


def test_the_record_is_of_these_axes(recorder, golden):
    assert json.loads(str(golden["axes"])) == json.loads(json.dumps([recorder.CLASSES, recorder.FIXED, recorder.AXES]))
    assert str(golden["singles"]) == recorder.singles_json()
    sizes = [len(values) for _, values in recorder.AXES]
    assert len(golden["codes"]) == 2 * int(np.prod(sizes)) == 124416


def test_cross_product_of_the_enumerated_options(recorder, recomputed, golden):
    got = recomputed[0]
    want = [str(o) for o in golden["outcomes"][golden["codes"]]]
    assert len(got) == len(want)
    diff = _first_difference(recorder.combinations(), got, want)
    if diff:
        print(diff)
    assert diff is None, diff
    accepted = [o for o in set(got) if o.startswith("LdcError")]
    assert len(accepted) == 1 and "no CPU fallback" in accepted[0]      # every other outcome is a refusal
    assert all(o.startswith("ValueError: ") for o in set(got) - set(accepted))


def test_single_keys(recorder, recomputed, golden):
    got, want = recomputed[1], [str(o) for o in golden["single_outcomes"]]
    assert len(got) == len(want) == len(recorder.SINGLES)
    diff = _first_difference(recorder.SINGLES, got, want)
    if diff:
        print(diff)
    assert diff is None, diff
