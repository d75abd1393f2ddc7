"""Writes tests/golden/g18_fv_options.npz: what ``FVSolver`` and ``FVFSGSolver`` answer to their options before they touch
the device, which tests/test_fv_options_cpu.py recomputes and compares combination by combination.  The first check that
fails decides the message, so the ORDER of the checks is part of what is pinned.

Table 1 is the cross product of the twelve enumerated options at two sizes (``AXES``, in ``itertools.product`` order) for
both classes; table 2 is one key at a time on an accepted base (``SINGLES``): a bad value of every enumeration, and every
scalar check.  An outcome is the exception's type name and full message; ``torch.cuda.is_available`` is patched to False,
so an accepted combination ends in the ``LdcError`` "no CPU fallback" of ``ldc_lib.require_device`` and every ``ValueError``
comes before it.  (``FVFSGSolver`` checks ``n_levels`` and ``coarse_tolerance_factor`` after ``FVSolver.__init__`` returns,
so without a device their rows record the ``LdcError``: that order is pinned too.)

Recorded once, from the commit before the option checks moved to solvers/fv/options.py:
    python tests/golden/make_golden_fv_options.py"""
import itertools
import json
import sys
from pathlib import Path
from unittest import mock

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent / "02689-advancednumericalalgorithmp3_amd" / "src"))

CLASSES = ("FVSolver", "FVFSGSolver")
FIXED = dict(ny=16, Re=100.0, name="fv")
AXES = (("mapping", ("cu", "chip", "shared")),
        ("grid", ("uniform", "tanh")),
        ("chip_grid", ("uniform", "tables")),
        ("transfer", ("uniform", "tables")),
        ("chip_transfer", ("uniform", "tables")),
        ("pressure_equation", ("reference", "consistent", "consistent_cu")),
        ("pressure_preconditioner", ("laplacian", "separable")),
        ("chip_preconditioner", ("laplacian", "separable")),
        ("acceleration", ("none", "anderson", "anderson_chip")),
        ("streamfunction", ("reference", "wall", "wall_stretched")),
        ("vortex_metrics", ("host", "device", "chip")),
        ("vortex_refine", ("none", "quadratic")),
        ("nx", (16, 512)))

_BASE = dict(FIXED, nx=16, vortex_metrics="host")
_TANH = dict(_BASE, grid="tanh")
SINGLES = tuple(
    [("FVSolver", dict(_BASE, **{key: "no-such-value"})) for key, _ in AXES[:-1]]
    + [("FVSolver", dict(_BASE, convection_scheme="no-such-value")),
       ("FVSolver", dict(_BASE, convection_scheme="TVD", limiter="no-such-value")),
       ("FVSolver", dict(_BASE, limiter="no-such-value")),
       ("FVSolver", dict(_BASE, anderson_depth=0)), ("FVSolver", dict(_BASE, anderson_depth=17)),
       ("FVSolver", dict(_BASE, anderson_start=0)),
       ("FVSolver", dict(_BASE, linear_budget=0)),
       ("FVSolver", dict(_BASE, pressure_tol=0.0)), ("FVSolver", dict(_BASE, pressure_tol=2.0)),
       ("FVSolver", dict(_BASE, pressure_max_iters=0)), ("FVSolver", dict(_BASE, pressure_budget=0)),
       ("FVSolver", dict(_TANH, grid_stretch=-1.0)), ("FVSolver", dict(_TANH, grid_stretch=float("nan"))),
       ("FVSolver", dict(_TANH, grid_stretch=float("inf"))), ("FVSolver", dict(_BASE, grid_stretch=-1.0))]
    + [("FVSolver", dict(_BASE, mapping=mapping, **{axis: n}))
       for mapping in ("cu", "chip", "shared") for axis in ("nx", "ny") for n in (7, 257, 1025)]
    + [("FVFSGSolver", dict(_BASE, n_levels=0)), ("FVFSGSolver", dict(_BASE, coarse_tolerance_factor=0.0)),
       ("FVFSGSolver", dict(_BASE, mapping="chip", nx=512)), ("FVFSGSolver", dict(_BASE, mapping="chip", nx=7))])


def outcome(cls, kwargs) -> str:
    try:
        cls(**kwargs)
    except Exception as exc:                  # (an accepted combination: the LdcError of require_device)
        return f"{type(exc).__name__}: {exc}"
    return "constructed"


def _classes():
    from solvers.fv.fsg import FVFSGSolver
    from solvers.fv.solver import FVSolver
    return dict(FVSolver=FVSolver, FVFSGSolver=FVFSGSolver)


def combinations():
    """Every (class name, keyword dict) of table 1, in the order of the recorded codes."""
    names = [name for name, _ in AXES]
    for cls in CLASSES:
        for values in itertools.product(*(vals for _, vals in AXES)):
            yield cls, dict(FIXED, **dict(zip(names, values)))


def tables():
    """(outcomes of table 1, outcomes of table 2), one string per combination, with no device in sight."""
    import torch
    classes = _classes()
    with mock.patch.object(torch.cuda, "is_available", lambda: False):
        return ([outcome(classes[cls], kw) for cls, kw in combinations()],
                [outcome(classes[cls], kw) for cls, kw in SINGLES])


def singles_json() -> str:
    return json.dumps([[cls, {k: repr(v) for k, v in kw.items()}] for cls, kw in SINGLES])


if __name__ == "__main__":
    cross, singles = tables()
    distinct = sorted(set(cross))
    codes = np.array([distinct.index(o) for o in cross], dtype=np.uint8 if len(distinct) < 256 else np.uint16)
    print(len(cross), "combinations,", len(distinct), "distinct outcomes;", len(singles), "single keys")
    np.savez_compressed(HERE / "g18_fv_options.npz", axes=np.array(json.dumps([CLASSES, FIXED, AXES])),
                        outcomes=np.array(distinct), codes=codes, singles=np.array(singles_json()),
                        single_outcomes=np.array(singles))
