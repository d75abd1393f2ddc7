"""``ldc_vortex_refine`` (csrc/ldc_vortex_refine.hip) on the device: the entry called directly against the long-double
statement of tests/vortex_refine_numpy.py within its derived bounds, the inputs that must fall back, the independence of
the jobs of a call, and the solvers' ``vortex_refine="newton"`` -- lone, off the square grid, Legendre, FSG, batched and
through the launcher.

Every comparison prints its largest error / bound (run with -s): profiles/spectral_refine.md keeps the table."""
import functools
import math

import numpy as np
import pytest

import spectral_post_numpy as P
import vortex_refine_numpy as R
from test_vortex_refine_cpu import FALLBACKS, FIXTURES, _fallback_cases

pytestmark = pytest.mark.gpu

KINDS = ("chebyshev", "legendre")
VORTEX_KEYS = ("psi_min", "psi_min_x", "psi_min_y", "omega_center", "omega_max", "omega_max_x", "omega_max_y") + tuple(
    f"{a}_{n}{b}" for n in ("BR", "BL", "TL") for a, b in (("psi", ""), ("omega", ""), ("psi", "_x"), ("psi", "_y")))


def _axes(kind, Mx, My):
    x, wx, Dx = R.grid(kind, Mx)
    y, wy, Dy = R.grid(kind, My)
    return x, y, wx, wy, Dx, Dy


@functools.lru_cache(maxsize=None)
def _entry_jobs(kind, Mx, My):
    """[(name, job arrays with idx, psi_err or None)] of one shape: the four quadratics, each from its grid extremum (the
    other extrema without a candidate), from 25 nodes per axis on the synthetic cavity with all four extrema, and at
    5 x 5 the quadratic at (0.0833, 0.0781) started at the boundary nodes (1, 0) and (0, 0)."""
    x, y, wx, wy, Dx, Dy = _axes(kind, Mx, My)
    W = np.cos(3 * x)[:, None] * np.sin(2 * y)[None, :]
    jobs = []

    def quad(x0, y0, s, start=None):
        Psi, err, _, _ = R.quadratic(x, y, x0, y0, s)
        e = 0 if s > 0 else 1 + [(0.8640, 0.1118), (0.0833, 0.0781)].index((x0, y0))
        idx = np.full(5, -1, dtype=np.int64)
        idx[R.IDX_SLOT[e]] = R.quadratic_start(x, y, x0, y0, My) if start is None else start[0] * My + start[1]
        jobs.append((f"quadratic({x0}, {y0}){'' if start is None else start}", (Psi, W, x, y, wx, wy, Dx, Dy, idx), err))
    for x0, y0, s in R.QUADRATICS:
        quad(x0, y0, s)
    if (Mx, My) == (5, 5):
        quad(0.0833, 0.0781, -1.0, start=(1, 0))
        quad(0.0833, 0.0781, -1.0, start=(0, 0))
    if min(Mx, My) >= 25:
        Psi, Wc = R.cavity(x, y)
        jobs.append(("cavity", (Psi, Wc, x, y, wx, wy, Dx, Dy, P.extrema(Psi, Wc, x, y)[1]), None))
    return jobs


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", R.GPU_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_entry_against_long_double(kind, shape):
    """x, y, psi, omega of every refined extremum within the derived bounds of the long-double statement; the status equal
    to the fp64 statement's, the step count equal or one off; the arrays beyond the live block hold NaN, which a read
    out of bounds would carry into the result."""
    jobs = _entry_jobs(kind, *shape)
    outs = R.device_call([j[1] for j in jobs])
    for (name, arrays, err), got in zip(jobs, outs):
        f64, want = R.refine(*arrays), R.refine(*arrays, dtype=R.LDBL)
        assert [int(v) for v in got[0::8]] == [int(v) for v in f64[0::8]], (name, got[0::8], f64[0::8])
        assert np.all(np.abs(got[5::8] - f64[5::8]) <= 1), (name, got[5::8], f64[5::8])
        assert np.all(got[7::8] == 0.0)
        live = [e for e in range(4) if int(got[8 * e]) != R.NO_CANDIDATE]
        assert live and all(int(got[8 * e]) == R.REFINED for e in live), (name, got[0::8])      # no case here may fall back
        for e in range(4):
            if e not in live:
                assert np.all(got[8 * e + 1: 8 * e + 8] == 0.0)
        ratio = R.compare(got, want, *arrays[:8], psi_err=err)
        print(f"{kind} {shape[0]}x{shape[1]} {name}: statuses {got[0::8].astype(int).tolist()}, steps "
              f"{got[5::8].astype(int).tolist()}, error / bound = {ratio:.4f}")
        assert ratio <= 1.0, name


@pytest.mark.parametrize("name", FALLBACKS)
def test_fallback_inputs(name):
    """The status of each input that must fall back, and the node's x, y, psi, omega bit for bit (zeros without a node)."""
    arrays, e, q, status = next(c[1:] for c in _fallback_cases() if c[0] == name)
    Psi, W, x, y = arrays[:4]
    idx = np.full(5, -1, dtype=np.int64)
    idx[R.IDX_SLOT[e]] = q
    got = R.device_call([arrays + (idx,)])[0]
    print(f"fallback {name}: {got[8 * e: 8 * e + 8]}")
    assert int(got[8 * e]) == status, got
    if q < 0:
        assert np.all(got[8 * e + 1: 8 * e + 8] == 0.0)
    else:
        i, j = divmod(q, Psi.shape[1])
        assert P.same_bits(got[8 * e + 1: 8 * e + 5], [x[i], y[j], Psi[i, j], W[i, j]])
    others = [k for k in range(4) if k != e]
    assert all(int(got[8 * k]) == R.NO_CANDIDATE for k in others)


def _mixed_jobs(n):
    shapes = [(9, 13), (33, 33), (48, 25), (5, 5), (51, 51), (26, 65)]
    pool = []
    for k in range(n):
        kind, shape = KINDS[k % 2], shapes[k % len(shapes)]
        cands = _entry_jobs(kind, *shape)
        pool.append(cands[(k // 2) % len(cands)][1])
    return pool


def test_jobs_of_a_call_are_independent():
    """Three jobs of different sizes in one call equal three calls of one job; forty jobs -- more than a launch holds --
    equal forty single calls; a repeated call repeats its bits."""
    three = [_entry_jobs("chebyshev", 33, 33)[-1][1], _entry_jobs("legendre", 9, 13)[1][1], _entry_jobs("chebyshev", 129, 48)[-1][1]]
    together = R.device_call(three)
    for job, got in zip(three, together):
        assert np.array_equal(R.device_call([job])[0], got)
    forty = _mixed_jobs(40)
    together = R.device_call(forty)
    again = R.device_call(forty)
    assert len(together) == 40
    for k, (job, got) in enumerate(zip(forty, together)):
        assert not np.any(got == -7.0), k                       # every block was written
        assert np.array_equal(again[k], got), k
        assert np.array_equal(R.device_call([job])[0], got), k


# ------------------------------------------------------------------------------------------------ through the solvers
def make(cls=None, **kw):
    from solvers.spectral.sg import SGSolver
    args = dict(name="spectral", Re=100.0, lid_velocity=1.0, Lx=1.0, Ly=1.0, nx=24, ny=24, tolerance=1e-6,
                max_iterations=1000, basis_type="chebyshev", CFL=1.5, beta_squared=5.0, corner_treatment="smoothing",
                corner_smoothing=0.15, multigrid="none", check_every=64, graph_iters=8)
    args.update(kw)
    return (cls or SGSolver)(**args)


def seed(s, iterations=30):
    """A developed flow as the solver's state: a primary vortex of psi = -0.1 off the centre and a positive eddy in each of
    the three corners, u = psi_y and v = -psi_x by the solver's own matrices, the boundary values imposed, then
    ``iterations`` iterations, which make it a state of the solver."""
    X, Y = s.x_full, s.y_full

    def eddy(x0, x1, y0, y1):
        inside = (X > x0) & (X < x1) & (Y > y0) & (Y < y1)
        return np.where(inside, (np.sin(np.pi * (X - x0) / (x1 - x0)) * np.sin(np.pi * (Y - y0) / (y1 - y0))) ** 2, 0.0)
    psi = -0.1 * (np.sin(np.pi * X ** 1.3) * np.sin(np.pi * Y ** 1.6)) ** 2
    psi += 0.005 * (eddy(0.7, 1.0, 0.0, 0.3) + eddy(0.0, 0.25, 0.0, 0.25)) + 0.02 * eddy(0.0, 0.3, 0.6, 0.9)
    u, v = psi @ s.Dy_1d.T, -(s.Dx_1d @ psi)
    u[0, :] = u[-1, :] = v[0, :] = v[-1, :] = 0.0
    u[:, 0] = v[:, 0] = v[:, -1] = 0.0
    u[:, -1] = s.u_lid
    s.set_state(u=u, v=v, p=np.zeros(s.shape_inner))
    if iterations:
        s.run_iterations(iterations)


def check_against_statement(s, vm, label):
    """The refined dict of solver s against the long-double statement applied to the psi and omega the solver left on the
    device, within the bounds; returns the statuses."""
    Mx, My = s.Mx, s.My
    Psi, W = s.d["S4"][:Mx, :My].cpu().numpy(), s.d["W"][:Mx, :My].cpu().numpy()
    x, wx, Dx = R.grid(s.params.basis_type, Mx)
    y, wy, Dy = R.grid(s.params.basis_type, My)
    assert np.array_equal(x, s.x_nodes) and np.array_equal(Dx, s.Dx_1d) and np.array_equal(Dy, s.Dy_1d)
    val, idx = P.extrema(Psi, W, x, y)
    arrays = (Psi, W, x, y, wx, wy, Dx, Dy)
    f64, want = R.refine(*arrays, idx), R.refine(*arrays, idx, dtype=R.LDBL)
    status = s.vortex_refine_status
    assert list(status) == [int(v) for v in f64[0::8]], (label, status, f64[0::8])
    got = f64.copy()                                            # (status and steps of the statement; values of the solver)
    got[1:5] = vm["psi_min_x"], vm["psi_min_y"], vm["psi_min"], vm["omega_center"]
    for e, n in ((1, "BR"), (2, "BL"), (3, "TL")):
        got[8 * e + 1: 8 * e + 5] = vm[f"psi_{n}_x"], vm[f"psi_{n}_y"], vm[f"psi_{n}"], vm[f"omega_{n}"]
    for e in range(4):
        if status[e] != R.REFINED:                              # a fallback or no candidate: the node's values, or zeros, exactly
            assert P.same_bits(got[8 * e + 1: 8 * e + 5], f64[8 * e + 1: 8 * e + 5]), (label, e)
    ratio = R.compare(got, want, *arrays)
    print(f"{label}: statuses {list(status)}, primary ({vm['psi_min_x']:.8f}, {vm['psi_min_y']:.8f}) psi {vm['psi_min']:.9f}, "
          f"error / bound = {ratio:.4f}")
    assert ratio <= 1.0, label
    assert vm["omega_max"] == val[1]
    return status


def newton_none_default(build, prepare):
    """The three solvers of one comparison, prepared alike: vortex_refine="newton", "none", and not given."""
    out = []
    for kw in (dict(vortex_refine="newton"), dict(vortex_refine="none"), {}):
        s = build(**kw)
        prepare(s)
        out.append((s, s.compute_vortex_metrics()))
    return out


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_solver_on_the_converged_fixtures(golden_dir, name):
    """``set_state`` from the fixture: with "newton" the dict equals the statement applied to the downloaded psi and omega
    within the bounds, and the primary vortex is the recorded one; omega_max* equals the "none" run bit for bit; "none"
    equals a solver built without the keyword bit for bit."""
    N, Re, table, half = FIXTURES[name]
    g = np.load(golden_dir / f"{name}.npz")

    def prepare(s):
        s.set_state(u=g["u"], v=g["v"])
    (sn, vn), (s0, v0), (sd, vd) = newton_none_default(lambda **kw: make(nx=N, ny=N, Re=float(Re), **kw), prepare)
    status = check_against_statement(sn, vn, name)
    assert status[0] == R.REFINED
    assert set(vn) == set(v0) == set(vd) == set(VORTEX_KEYS)
    assert all(P.same_bits(v0[k], vd[k]) for k in VORTEX_KEYS) and s0.vortex_refine_status is None
    assert all(P.same_bits(vn[k], v0[k]) for k in ("omega_max", "omega_max_x", "omega_max_y"))
    got = np.array([vn["psi_min_x"], vn["psi_min_y"], vn["psi_min"], vn["omega_center"]])
    # the table was taken from the oracle's psi; the device's psi differs from it by 1e-10 max|psi| at the most
    assert np.all(np.abs(got - np.array(table)) <= np.array(half) + 1e-8), (got, table)
    assert vn["psi_min"] <= v0["psi_min"]
    for s in (sn, s0, sd):
        s.close()


def _fsg(**kw):
    from solvers.spectral.fsg import FSGSolver
    return make(FSGSolver, multigrid="fsg", n_levels=2, **kw)


@pytest.mark.parametrize("label,build", [("20x28", lambda **kw: make(nx=20, ny=28, **kw)),
                                         ("legendre", lambda **kw: make(basis_type="legendre", **kw)),
                                         ("fsg", _fsg)], ids=["20x28", "legendre", "fsg"])
def test_solver_on_a_developed_state(label, build):
    """The same three comparisons off the square grid, on Legendre nodes and on an FSGSolver's fine level, from a seeded
    developed flow with a primary vortex and three corner eddies."""
    (sn, vn), (s0, v0), (sd, vd) = newton_none_default(build, seed)
    status = check_against_statement(sn, vn, label)
    assert status[0] == R.REFINED and vn["psi_min"] <= v0["psi_min"]
    assert all(P.same_bits(v0[k], vd[k]) for k in VORTEX_KEYS)
    assert all(P.same_bits(vn[k], v0[k]) for k in ("omega_max", "omega_max_x", "omega_max_y"))
    for s in (sn, s0, sd):
        s.close()


def test_batched_trials_equal_their_lone_runs():
    """Three N = 16 trials advanced 30 iterations in one batch: every vortex key of every trial equals the trial's lone
    solve bit for bit, and so do the statuses."""
    from solvers.spectral.batched import BatchedSGSolver
    trials = [dict(Re=100.0, corner_smoothing=0.15), dict(Re=400.0, corner_smoothing=0.10), dict(Re=50.0, corner_smoothing=0.30)]
    trials = [dict(nx=16, ny=16, max_iterations=30, vortex_refine="newton", **t) for t in trials]
    b = BatchedSGSolver([make(cls=dict, **t) for t in trials])
    ms = b.solve()
    for t, s, m in zip(trials, b.solvers, ms):
        one = make(**t)
        one.solve()
        assert m.iterations == one.metrics.iterations == 30
        assert s.vortex_refine_status is not None and s.vortex_refine_status == one.vortex_refine_status
        for k in VORTEX_KEYS:
            assert P.same_bits(getattr(m, k), getattr(one.metrics, k)), (k, getattr(m, k), getattr(one.metrics, k))
        assert m.psi_min < 0
        one.close()
    b.close()


def test_launcher_takes_the_override(tmp_path, monkeypatch):
    import importlib.util
    import json
    from conftest import PKG
    spec = importlib.util.spec_from_file_location("ldc_main", PKG / "main.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    recs = {}
    for mode, extra in (("none", []), ("newton", ["+solver.vortex_refine=newton"])):
        d = tmp_path / mode
        d.mkdir()
        monkeypatch.chdir(d)
        mod.main(["solver=spectral", "N=16", "Re=100", "max_iterations=400"] + extra)
        recs[mode] = json.loads(next(d.rglob("results.json")).read_text())
    assert recs["newton"]["params"]["vortex_refine"] == "newton" and recs["none"]["params"]["vortex_refine"] == "none"
    node, fine = recs["none"]["metrics"], recs["newton"]["metrics"]
    x = R.grid("chebyshev", 17)[0]
    assert node["psi_min_x"] in x and node["psi_min_y"] in x
    assert fine["psi_min_x"] not in x and fine["psi_min_y"] not in x and fine["psi_min"] < node["psi_min"] < 0
    assert abs(fine["psi_min_x"] - node["psi_min_x"]) < 0.2 and abs(fine["psi_min_y"] - node["psi_min_y"]) < 0.2
    assert all(fine[k] == node[k] for k in ("omega_max", "omega_max_x", "omega_max_y", "iterations", "final_energy"))
    assert math.isfinite(fine["omega_center"])
