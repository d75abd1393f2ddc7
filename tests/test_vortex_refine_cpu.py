"""Sub-grid vortex centres (``ldc_vortex_refine``, ``SpectralParameters.vortex_refine``) without a device: the NumPy
statement of the algorithm (tests/vortex_refine_numpy.py) on exact quadratics, on a synthetic cavity, on the inputs that
must fall back and on the converged fixtures; the parameter surface; the C ABI's argument checks.

Every comparison prints its largest error / bound (run with -s): profiles/spectral_refine.md keeps the table."""
import ctypes as C
import json
import re
from pathlib import Path

import numpy as np
import pytest

import spectral_post_numpy as P
import vortex_refine_numpy as R
from oracle import ldc_oracle as orc
from solvers import validation as V
from types import SimpleNamespace

ROOT = Path(__file__).resolve().parent.parent
KINDS = ("chebyshev", "legendre")


def _grids(kind, nx, ny):
    x, wx, Dx = R.grid(kind, nx + 1)
    y, wy, Dy = R.grid(kind, ny + 1)
    return x, y, wx, wy, Dx, Dy


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("size", R.QUADRATIC_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_exact_quadratics(kind, size):
    """The interpolant of a quadratic is the quadratic: the restatement finds (x0, y0) with status 0 within the derived
    bound -- evaluation and stop rule (vortex_refine_numpy.bounds, with the rounding of the field's own entries), plus what
    the first-derivative matrices as handed over are off the exact derivative of THIS field at the solution, measured in
    long double (|H^-1| |a (D psi - psi') b|: the operator's own error, no part of the algorithm's)."""
    x, y, wx, wy, Dx, Dy = _grids(kind, *size)
    W = np.cos(3 * x)[:, None] * np.sin(2 * y)[None, :]
    ld = lambda a: np.asarray(a, dtype=R.LDBL)          # noqa: E731
    for x0, y0, s in R.QUADRATICS:
        Psi, err, _, _ = R.quadratic(x, y, x0, y0, s)
        q = R.quadratic_start(x, y, x0, y0, Psi.shape[1])
        e = 0 if s > 0 else 1 + [(0.8640, 0.1118), (0.0833, 0.0781)].index((x0, y0))
        out, _ = R.refine_one(Psi, W, x, y, wx, wy, Dx, Dy, e, q, Psi.shape[1])
        assert int(out[0]) == R.REFINED, (x0, y0, out)
        assert 1 <= int(out[5]) <= R.MAX_STEPS
        loc, _, _ = R.bounds(Psi, W, x, y, wx, wy, Dx, Dy, x0, y0, psi_err=err)
        psi_l, _, px, py = R.quadratic(x, y, x0, y0, s, dtype=R.LDBL)
        a, _, _, b, _, _ = R.evaluate(psi_l, ld(x), ld(y), ld(wx), ld(wy), ld(Dx), ld(Dy), R.LDBL(x0), R.LDBL(y0))
        defect = np.abs(np.array([a @ (ld(Dx) @ psi_l - px) @ b, a @ (psi_l @ ld(Dy).T - py) @ b], dtype=float))
        H = float(s) * np.array([[2.0, 0.3], [0.3, 4.0]])
        loc = loc + P.SLACK * (np.abs(np.linalg.inv(H)) @ defect)
        miss = np.abs(out[1:3] - np.array([x0, y0]))
        print(f"quadratic {kind} {size[0]}x{size[1]} ({x0}, {y0}): steps {int(out[5])}, |dz| = {miss.max():.2e}, "
              f"error / bound = {np.max(miss / loc):.4f}")
        assert np.all(miss <= loc), (miss, loc)


def _cavity_job(kind, size):
    x, y, wx, wy, Dx, Dy = _grids(kind, *size)
    Psi, W = R.cavity(x, y)
    _, idx = P.extrema(Psi, W, x, y)
    return Psi, W, x, y, wx, wy, Dx, Dy, idx


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("size", R.CAVITY_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_synthetic_cavity(kind, size):
    """All four extrema refine (status 0) in fp64 and in long double, and fp64 agrees with long double within the bounds."""
    job = _cavity_job(kind, size)
    got, want = R.refine(*job), R.refine(*job, dtype=R.LDBL)
    assert [int(v) for v in got[0::8]] == [0, 0, 0, 0] == [int(v) for v in want[0::8]], (got[0::8], want[0::8])
    assert np.all(np.abs(got[5::8] - want[5::8].astype(float)) <= 1)
    ratio = R.compare(got, want, *job[:8])
    print(f"cavity {kind} {size[0]}x{size[1]}: steps {got[5::8].astype(int).tolist()}, error / bound = {ratio:.4f}, "
          f"TL at ({got[25]:.8f}, {got[26]:.8f})")
    assert ratio <= 1.0
    if size == (96, 64):
        assert abs(got[25] - 0.06238859) < 1e-8 and abs(got[26] - 0.90546036) < 1e-8


def _fallback_cases():
    """[(name, job arrays, extremum, flat start index, expected status)] on N = 16 Chebyshev grids."""
    x, y, wx, wy, Dx, Dy = _grids("chebyshev", 16, 16)
    X, Y = x[:, None], y[None, :]
    W = np.cos(3 * X) * np.sin(2 * Y)
    M = y.size
    cases = []
    for name, Psi in (("linear", X + Y), ("saddle", (X - 0.4) ** 2 - (Y - 0.6) ** 2)):
        cases.append((name, Psi, 0, int(np.argmin(Psi)), R.INDEFINITE))
    bowl = (X - 0.52) ** 2 + (Y - 0.52) ** 2
    cases.append(("clipped", bowl, 0, 3 * M + 3, R.CLIPPED))
    cases.append(("no_candidate", bowl, 0, -1, R.NO_CANDIDATE))
    bad = bowl.copy()
    bad[10, 2] = np.nan
    cases.append(("nan", bad, 0, int(np.nanargmin(bad)), R.NOT_FINITE))
    return [(n, (Psi, W, x, y, wx, wy, Dx, Dy), e, q, st) for n, Psi, e, q, st in cases]


FALLBACKS = ["linear", "saddle", "clipped", "no_candidate", "nan"]


@pytest.mark.parametrize("name", FALLBACKS)
def test_fallback_inputs_keep_the_node(name):
    """The expected status and the node's values bit for bit, in both precisions.  (The Hessian of x + y is identically
    zero: what an evaluation sees of it is its own rounding, which the definiteness rule's floor rejects in any
    precision and summation order.)"""
    arrays, e, q, status = next(c[1:] for c in _fallback_cases() if c[0] == name)
    Psi, W, x, y = arrays[:4]
    for dtype in (np.float64, R.LDBL):
        out, _ = R.refine_one(*arrays, e, q, Psi.shape[1], dtype)
        assert int(out[0]) == status, out
        if q < 0:
            assert np.all(out[1:] == 0)
        else:
            i, j = divmod(q, Psi.shape[1])
            assert P.same_bits(np.asarray(out[1:5], float), [x[i], y[j], Psi[i, j], W[i, j]])


# the table of the issue that asked for the refinement: (x, y, psi, omega) of the primary vortex at the stationary point
FIXTURES = {"g7_converged_N32_Re100": (32, 100, (0.61857, 0.73669, -0.1031693, -3.1713), (5e-6, 5e-6, 5e-8, 5e-5)),
            "g7_converged_N64_Re400": (64, 400, (0.56199, 0.60965, -0.1101060, -2.3163), (5e-6, 5e-6, 5e-8, 5e-5))}


def _fixture_job(golden_dir, name):
    N = FIXTURES[name][0]
    g = np.load(golden_dir / f"{name}.npz")
    o = orc.OracleSG(N, float(FIXTURES[name][1]))
    o.u, o.v = g["u"].reshape(N + 1, N + 1).copy(), g["v"].reshape(N + 1, N + 1).copy()
    Psi, W = o.streamfunction(), o.vorticity()
    x, y, wx, wy, Dx, Dy = _grids("chebyshev", N, N)
    assert np.array_equal(x, o.ax.x)
    _, idx = P.extrema(Psi, W, x, y)
    return Psi, W, x, y, wx, wy, Dx, Dy, idx


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_fixtures_match_the_table(golden_dir, name):
    """The refined primary vortex of the converged fixtures equals the recorded table to its printed digits (half a unit of
    the last one) plus the restatement's bound; at N = 32, Re = 100 the Botella objective falls."""
    job = _fixture_job(golden_dir, name)
    got = R.refine(*job)
    want, half = FIXTURES[name][2], FIXTURES[name][3]
    assert int(got[0]) == R.REFINED and 3 <= int(got[5]) <= 6
    loc, dpsi, domega = R.bounds(*job[:8], got[1], got[2])
    tol = np.array(half) + np.array([loc[0], loc[1], dpsi, domega])
    print(f"{name}: refined primary {got[1:5]}, steps {int(got[5])}, bounds {loc}, {dpsi:.2e}, {domega:.2e}")
    assert np.all(np.abs(got[1:5] - np.array(want)) <= tol), (got[1:5], want)
    if name == "g7_converged_N32_Re100":
        meta = json.loads((golden_dir / f"{name}.json").read_text())["metrics"]
        node = SimpleNamespace(**{k: meta[k] for k in ("psi_min", "psi_min_x", "psi_min_y")})
        fine = SimpleNamespace(psi_min=got[3], psi_min_x=got[1], psi_min_y=got[2])
        on_grid, refined = (V.compute_botella_vortex_objective(m, 100) for m in (node, fine))
        print(f"Botella objective at N = 32, Re = 100: grid {on_grid:.3e}, refined {refined:.3e}")
        assert refined < on_grid
        assert abs(on_grid - 1.26e-2) < 1e-4 and abs(refined - 2.0e-3) < 1e-4


# ------------------------------------------------------------------------------------------------ parameter surface
def test_parameter_surface():
    from solvers.datastructures import SpectralParameters
    from solvers.spectral.sg import SGSolver
    p = SpectralParameters(name="spectral", nx=16, ny=16)
    assert p.vortex_refine == "none" and p.to_mlflow()["vortex_refine"] == "none"
    assert SpectralParameters(name="spectral", nx=16, ny=16, vortex_refine="newton").to_mlflow()["vortex_refine"] == "newton"
    with pytest.raises(ValueError, match="vortex_refine"):          # before the device is asked for: no LdcError here
        SGSolver(name="spectral", Re=100.0, nx=16, ny=16, vortex_refine="spline")


def test_yaml_composes_with_the_override():
    from dataclasses import fields
    from conftest import PKG
    from solvers.datastructures import SpectralParameters
    from utilities.config import compose as Cc
    comp = Cc.Composer(PKG / "conf")
    for opt in ("spectral/sg", "spectral/fsg"):
        cfg = Cc.resolve(Cc.compose_job(comp, [f"solver={opt}"], []))
        assert "vortex_refine" not in cfg["solver"]                      # the YAML files are unchanged
        cfg = Cc.resolve(Cc.compose_job(comp, [f"solver={opt}", "+solver.vortex_refine=newton"], []))
        assert cfg["solver"]["vortex_refine"] == "newton"
        kw = {k: v for k, v in cfg["solver"].items() if k != "_target_"}
        assert set(kw) <= {f.name for f in fields(SpectralParameters)}
        assert SpectralParameters(**kw).vortex_refine == "newton"


def test_barycentric_weights_interpolate():
    """Both families: the basis of the weights reproduces a polynomial of full degree at an off-node point."""
    for kind in KINDS:
        for M in (5, 33, 257):
            x, w, _ = R.grid(kind, M)
            z = 0.3712
            a = R.basis(x.astype(R.LDBL), w.astype(R.LDBL), R.LDBL(z))
            assert abs(float(np.sum(a)) - 1.0) < 1e-15
            f = lambda t: (2 * t - 1) ** 4 - 0.3 * t          # noqa: E731
            assert abs(float(a @ f(x.astype(R.LDBL))) - f(z)) < 1e-13, (kind, M)


# ------------------------------------------------------------------------------------------------ C ABI
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from solvers.spectral import ldc_lib
    return ldc_lib


def test_header_exports_and_constants_agree(lib):
    hdr = (ROOT / "include" / "ldc_hip.h").read_text()
    assert "ldc_vortex_refine" in set(re.findall(r"\b(ldc_[a-z_0-9]+)\s*\(", hdr)) & set(lib.EXPORTS)
    assert hasattr(lib.lib(), "ldc_vortex_refine")
    val = lambda name: int(re.search(rf"#define {name} (\d+)", hdr).group(1))        # noqa: E731
    assert (val("LDC_REFINE_OUT_LEN"), val("LDC_REFINE_MAX_STEPS"), val("LDC_REFINE_MAX_M")) == \
        (lib.REFINE_OUT_LEN, lib.REFINE_MAX_STEPS, lib.REFINE_MAX_M) == (R.OUT_LEN, R.MAX_STEPS, R.MAX_M)
    assert C.sizeof(lib.RefineJob) == 10 * 8 + 4 * 4 and len(lib.REFINE_STATUS) == 7
    assert lib.lib().ldc_version() == 7


POINTERS = ("Psi", "W", "x", "y", "wx", "wy", "Dx", "Dy", "idx", "out")


def _job(lib, **over):
    j = lib.RefineJob()
    for n in POINTERS:
        setattr(j, n, 8)                              # never dereferenced: validation comes first
    j.Mx, j.My, j.LD, j.LDD = 33, 17, 48, 48
    for k, v in over.items():
        setattr(j, k, v)
    return j


REFUSED = [{n: None} for n in POINTERS] + [dict(Mx=2), dict(My=2), dict(Mx=258, LD=272, LDD=272), dict(My=258, LD=272, LDD=272),
                                           dict(LD=16), dict(LDD=32), dict(Mx=17, My=33, LDD=32)]


def test_refused_arguments_need_no_device(lib):
    import torch
    L = lib.lib()
    assert L.ldc_vortex_refine(None, 1, None) == -1
    assert L.ldc_vortex_refine(C.byref(_job(lib)), 0, None) == -1
    for over in REFUSED:
        assert L.ldc_vortex_refine(C.byref(_job(lib, **over)), 1, None) == -1, over
        pair = (lib.RefineJob * 2)(_job(lib), _job(lib, **over))          # the second job of a call is checked too
        assert L.ldc_vortex_refine(pair, 2, None) == -1, over
    if not torch.cuda.is_available():
        assert L.ldc_vortex_refine(C.byref(_job(lib)), 1, None) == -3          # LDC_E_NODEVICE: everything else in order
