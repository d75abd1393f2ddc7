"""Finite-volume streamfunction and vortex metrics on the device (ldc_fv_post_enqueue, ``vortex_metrics="device"``).
The yardstick is always the host path of the same solver object (``_vorticity``, ``_streamfunction``, the host branch
of ``compute_vortex_metrics``) and the long-double solve of tests/fv_post_numpy.py, never the device path itself."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"
sys.path.insert(0, str(Path(__file__).resolve().parent))
import fv_post_numpy as P  # noqa: E402
from fv_post_numpy import EPS, LD  # noqa: E402

from conftest import PKG  # noqa: E402

pytestmark = pytest.mark.gpu

YAML = dict(name="fv", convection_scheme="TVD", alpha_uv=0.4, alpha_p=0.2, linear_solver_tol=1e-9)      # conf/solver/fv.yaml
PSI_KEYS = ("psi_min", "psi_BR", "psi_BL", "psi_TL")
OMEGA_KEYS = ("omega_center", "omega_max")


@pytest.fixture(scope="module")
def fv():
    import __graft_entry__ as g
    g.build()
    from solvers.fv.batched import BatchedFVSolver
    from solvers.fv.solver import FVSolver
    return FVSolver, BatchedFVSolver


def _solver(FVSolver, nx, ny, Lx=1.0, Ly=1.0, **kw):
    return FVSolver(**dict(YAML, Re=100.0, nx=nx, ny=ny, Lx=Lx, Ly=Ly, vortex_metrics="device", **kw))


def _set(s, u, v):
    s.set_state(u, v, np.zeros(s.n_cells), np.zeros(s.t["mdot"].numel()))
    s._finalize_fields()


def _metrics(s, mode):
    """``compute_vortex_metrics`` of the current state by the host or the device branch."""
    keep = s.params.vortex_metrics
    s.params.vortex_metrics = mode
    try:
        return s.compute_vortex_metrics()
    finally:
        s.params.vortex_metrics = keep


def _bounds(s, psi_ref):
    u, v = s.fields.u, s.fields.v
    return (P.omega_bound(u, v, s.params.lid_velocity, s.dx_min, s.dy_min),
            P.psi_bound(psi_ref, s.nx, s.ny, s.dx_min, s.dy_min))


def _assert_metrics_close(dev, host, bw, bp, what=""):
    assert set(dev) == set(host), what
    for k in host:
        if k in PSI_KEYS:
            assert abs(dev[k] - host[k]) <= bp, (what, k, dev[k], host[k])
        elif k in OMEGA_KEYS:
            assert abs(dev[k] - host[k]) <= bw, (what, k, dev[k], host[k])
        else:                                   # x, y: taken from the same xs, ys by index
            assert dev[k] == host[k], (what, k, dev[k], host[k])


# ------------------------------------------------------------------------------------------- a, b. fields and metrics
@pytest.fixture(scope="module")
def seeded(fv):
    """Per shape, computed once: the solver holding the seeded state, the host omega and psi, the long-double psi."""
    FVSolver, _ = fv
    cases = {}

    def get(shape):
        if shape not in cases:
            nx, ny, Lx, Ly = shape
            s = _solver(FVSolver, nx, ny, Lx, Ly)
            _set(s, *P.random_state(nx, ny))
            omega = s._vorticity()
            cases[shape] = (s, omega, s._streamfunction(omega), P.psi_solve(omega, s.dx_min, s.dy_min, LD))
        return cases[shape]
    yield get
    for s, *_ in cases.values():
        s.close()


@pytest.mark.parametrize("shape", P.GPU_SHAPES, ids=P.shape_id)
def test_fields_against_the_host_path_and_long_double(seeded, shape):
    """omega within 4 eps max(|u|, |v|, lid)(1/dx + 1/dy) of ``_vorticity``; psi within 4 eps kappa max|psi| of the
    long-double solve; the psi ring exactly 0.0.  Measured shares of eps kappa max|psi| on an MI355X, in the order of
    the shapes: see profiles/fv_perf.md."""
    s, omega, _, psi_ld = seeded(shape)
    bw, bp = _bounds(s, psi_ld)
    w = s.vorticity()
    psi = s.streamfunction()
    assert w.shape == psi.shape == (s.ny, s.nx)
    ew = float(np.max(np.abs(w - omega)))
    ep = float(np.max(np.abs(psi.astype(LD) - psi_ld)))
    k = P.kappa(s.nx, s.ny, s.dx_min, s.dy_min)
    print(f"FVPOST {s.nx}x{s.ny}: omega err {ew:.2e} (bound {bw:.2e}); psi err {ep:.2e}, kappa {k:.2e}, "
          f"share of eps kappa max|psi| {ep / (EPS * k * float(np.max(np.abs(psi_ld)))):.3f} (bound 4)")
    assert np.all(np.isfinite(w)) and np.all(np.isfinite(psi))
    assert ew <= bw
    assert ep <= bp
    for ring in (psi[0], psi[-1], psi[:, 0], psi[:, -1]):
        assert np.all(ring == 0.0) and not np.any(np.signbit(ring))


@pytest.mark.parametrize("shape", P.GPU_SHAPES, ids=P.shape_id)
def test_metrics_against_the_host_branch(seeded, shape):
    s, omega, psi, psi_ld = seeded(shape)
    bw, bp = _bounds(s, psi_ld)
    host = _metrics(s, "host")
    # precondition, on the host values: no extremum can move to another cell inside the bounds
    gaps = P.runner_up_gaps(psi, omega, s._mask_bounds)
    assert gaps["omega_max"] > 2 * bw and all(gaps[k] > 2 * bp for k in PSI_KEYS)
    if s.params.Ly > 0.5:
        assert min(host[k] for k in PSI_KEYS[1:]) > 2 * bp
    dev = _metrics(s, "device")
    _assert_metrics_close(dev, host, bw, bp, shape)
    assert dev == P.extrema(s.streamfunction(), s.vorticity(), s._mask_bounds,
                            *P.cell_centres(s.nx, s.ny, s.params.Lx, s.params.Ly))


# ------------------------------------------------------------------------------------------- c. ties, the zero branch
def test_ties_and_the_zero_branch(fv):
    FVSolver, _ = fv
    nx, ny = 13, 17
    s = _solver(FVSolver, nx, ny)
    xs, ys = P.cell_centres(nx, ny, 1.0, 1.0)
    X = np.meshgrid(xs, ys)[0].ravel()
    zeros = {f"psi_{r}{t}": 0.0 for r in ("BR", "BL", "TL") for t in ("", "_x", "_y")}
    # all zero: omega is 0 below the lid row (the lid's ghost cells make it -lid / dy there, at every cell of the row:
    # a tie), so psi == 0 everywhere, its minimum at cell 0, all corners on the zero branch
    _set(s, np.zeros(nx * ny), np.zeros(nx * ny))
    dev = _metrics(s, "device")
    w, psi = s.vorticity(), s.streamfunction()
    assert np.all(psi == 0.0) and not np.any(np.signbit(psi)) and np.all(w[:-1] == 0.0) and np.all(w[-1] == -1.0 / s.dy_min)
    assert dev == _metrics(s, "host")
    assert dev == dict(zeros, psi_min=0.0, psi_min_x=xs[0], psi_min_y=ys[0], omega_center=0.0,
                       omega_max=-1.0 / s.dy_min, omega_max_x=xs[0], omega_max_y=ys[-1])
    # u = 0, v = -x: omega < 0 in the interior, psi < 0 there, all corners zero
    _set(s, np.zeros(nx * ny), -X)
    w, psi = s.vorticity(), s.streamfunction()
    assert np.all(w[1:-1, 1:-1] < 0) and np.all(psi[1:-1, 1:-1] < 0)
    dev, host = _metrics(s, "device"), _metrics(s, "host")
    _assert_metrics_close(dev, host, *_bounds(s, s._streamfunction(s._vorticity())))
    assert {k: dev[k] for k in zeros} == zeros and dev["psi_min"] < 0
    # omega = 10 ... 11 in the rows j <= 3 and -2 ... -3 above: a positive corner value in BR and BL, none in TL,
    # where the largest psi is the 0.0 of the ring
    rng = np.random.default_rng(7)
    rows = np.arange(ny)[:, None] * np.ones((1, nx))
    omega = np.where(rows <= 3, 10.0 + rng.random((ny, nx)), -2.0 - rng.random((ny, nx)))
    v = np.zeros((ny, nx))                      # (v[:, i+1] - v[:, i-1]) / (2 dx) = omega[:, i] in the interior
    for i in range(1, nx - 1):
        v[:, i + 1] = v[:, i - 1] + 2 * s.dx_min * omega[:, i]
    _set(s, np.zeros(nx * ny), v.ravel())
    dev, host = _metrics(s, "device"), _metrics(s, "host")
    print("corner case:", {k: dev[k] for k in ("psi_BR", "psi_BL", "psi_TL", "psi_min")})
    assert host["psi_BR"] > 0.05 and host["psi_BL"] > 0.05 and host["psi_TL"] == 0.0
    _assert_metrics_close(dev, host, *_bounds(s, s._streamfunction(s._vorticity())))
    s.close()


# ------------------------------------------------------------------------------------------- d. golden
def _kwargs(m, **kw):
    args = dict(name="fv", Re=m["Re"], nx=m["nx"], ny=m["ny"], corner_treatment=m.get("lid", "none"),
                alpha_uv=m.get("alpha_uv", 0.4), alpha_p=m.get("alpha_p", 0.2),
                linear_solver_tol=m["linear_solver_tol"], convection_scheme=m["convection_scheme"],
                Lx=m.get("Lx", 1.0), Ly=m.get("Ly", 1.0), lid_velocity=m.get("lid_velocity", 1.0),
                tolerance=m.get("tolerance", 1e-30), max_iterations=10**6, check_every=256)
    args.update(kw)
    return args


@pytest.fixture(scope="module")
def converged_case():
    return json.loads((GOLD / "g15_fv_converged.json").read_text()), np.load(GOLD / "g15_fv_converged.npz")


VORTEX_GOLDEN = ("psi_min", "psi_min_x", "psi_min_y", "omega_center", "omega_max", "psi_BR", "psi_BL")


def test_converged_reference_state_gives_the_reference_metrics(fv, converged_case):
    """The reference's converged 13 x 17 fields, set as the state: the device metrics against the metrics the reference
    stored (tolerance of test_solve_stops_at_the_reference_iteration)."""
    FVSolver, _ = fv
    meta, g = converged_case
    s = FVSolver(**_kwargs(meta, vortex_metrics="device"))
    s.set_state(g["u"], g["v"], g["p"], g["mdot"])
    s._finalize_fields()
    dev = s.compute_vortex_metrics()
    for key in VORTEX_GOLDEN:
        print(key, dev[key], meta["metrics"][key])
        assert dev[key] == pytest.approx(meta["metrics"][key], rel=1e-7, abs=1e-10), key
    s.close()


# ------------------------------------------------------------------------------------------- e. the trial is left alone
def test_postprocessing_leaves_the_trial_alone(fv, converged_case):
    FVSolver, _ = fv
    from solvers.fv.solver import postprocess
    meta, _ = converged_case
    a, b = (FVSolver(**_kwargs(meta, vortex_metrics="device", tolerance=1e-30)) for _ in range(2))
    rows = {}
    for s in (a, b):
        s._begin(1e-30)
        rows[s] = [s._advance(20)[0]]
    postprocess([a])
    assert a._post is not None and a._post[0] < 0 and b._post is None
    for s in (a, b):
        rows[s].append(s._advance(20)[0])
    sa, sb = a.state(), b.state()
    for k in ("u", "v", "p", "mdot"):
        assert np.array_equal(sa[k], sb[k]), k
    assert np.array_equal(np.concatenate(rows[a]), np.concatenate(rows[b])) and np.concatenate(rows[a]).shape == (40, 8)
    assert a.counters() == b.counters() and a.counters()["iterations"] == 40
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------- f. solve()
def _same_solve(x, y, what):
    """Fields, history, counters bit-equal; returns the two metrics dicts without the wall time."""
    assert np.array_equal(x.history, y.history), what
    sx, sy = x.state(), y.state()
    for k in ("u", "v", "p", "mdot"):
        assert np.array_equal(sx[k], sy[k]), (what, k)
    assert x.counters() == y.counters(), what
    mx, my = x.metrics.as_dict(), y.metrics.as_dict()
    mx.pop("wall_time_seconds"), my.pop("wall_time_seconds")
    return mx, my


def _assert_solve_metrics_close(dev_solver, md, mh, what=""):
    s = dev_solver
    psi = s._streamfunction(s._vorticity())
    bw, bp = _bounds(s, psi)
    assert set(md) == set(mh)
    for k in mh:
        if k in PSI_KEYS:
            assert abs(md[k] - mh[k]) <= bp, (what, k)
        elif k in OMEGA_KEYS:
            assert abs(md[k] - mh[k]) <= bw, (what, k)
        else:
            assert md[k] == mh[k], (what, k, md[k], mh[k])


def test_solve_in_device_mode_equals_host_mode(fv, converged_case):
    FVSolver, _ = fv
    meta, _ = converged_case
    dev, host = FVSolver(**_kwargs(meta, vortex_metrics="device")), FVSolver(**_kwargs(meta))
    assert host.params.vortex_metrics == "host"
    dev.solve()
    host.solve()
    assert dev.metrics.iterations == host.metrics.iterations == 280 and dev.metrics.converged
    md, mh = _same_solve(dev, host, "13x17")
    assert mh["psi_min"] < 0 and md["psi_min"] < 0
    _assert_solve_metrics_close(dev, md, mh)
    assert "psi" in dev.t and "psi" not in host.t
    dev.close()
    host.close()


# ------------------------------------------------------------------------------------------- g. batches
def test_batch_in_device_mode_equals_lone_device_solves(fv):
    FVSolver, BatchedFVSolver = fv
    common = dict(YAML, tolerance=1e-5, max_iterations=20000, check_every=256, vortex_metrics="device")
    trials = [dict(common, nx=16, ny=16, Re=100.0),
              dict(common, nx=24, ny=16, Re=400.0),
              dict(common, nx=20, ny=20, Re=100.0),
              dict(common, nx=24, ny=24, Re=400.0, corner_treatment="saad"),
              dict(common, nx=16, ny=16, Re=100.0, convection_scheme="Upwind"),
              dict(common, nx=13, ny=17, Re=100.0, max_iterations=300, vortex_metrics="host")]
    batch = BatchedFVSolver(trials)
    batch.solve()
    assert batch.errors == {}
    for q, (b, t) in enumerate(zip(batch.solvers, trials)):
        lone = FVSolver(**t)
        lone.solve()
        mb, ml = _same_solve(b, lone, q)
        assert mb == ml and mb["psi_min"] < 0, (q, mb, ml)                  # bit for bit, vortex metrics included
        if q == 0:                                                          # and the host-mode solve within the bounds
            host = FVSolver(**dict(t, vortex_metrics="host"))
            host.solve()
            _assert_solve_metrics_close(b, mb, _same_solve(b, host, "host")[1], "host")
            host.close()
        lone.close()
    assert "psi" not in batch.solvers[5].t                                  # the host-mode trial was not post-processed
    batch.close()


def test_more_trials_than_one_post_launch_takes(fv, monkeypatch):
    """260 trials of 8 x 8 cells (0.05 / 0.05 relaxation, 40 iterations, as test_more_trials_than_one_launch_takes):
    two post launches, 256 + 4, one copy of the result blocks."""
    FVSolver, BatchedFVSolver = fv
    from solvers.fv import ldc_fv_lib as F
    n = 260
    trials = [dict(YAML, alpha_uv=0.05, alpha_p=0.05, nx=8, ny=8, Re=100.0 + 900.0 * q / (n - 1), tolerance=1e-30,
                   max_iterations=40, check_every=64, vortex_metrics="device") for q in range(n)]
    batch = BatchedFVSolver(trials)
    launches = []
    real = F.post_enqueue
    monkeypatch.setattr(F, "post_enqueue", lambda hs, posts, stream: (launches.append(len(hs)), real(hs, posts, stream))[1])
    batch.solve()
    monkeypatch.setattr(F, "post_enqueue", real)
    assert batch.errors == {} and launches == [256, 4]
    assert all(s.metrics.psi_min < 0 for s in batch.solvers)
    for q in (0, 1, 63, 128, 254, 255, 256, 257, 258, 259):
        lone = FVSolver(**trials[q])
        lone.solve()
        mb, ml = _same_solve(batch.solvers[q], lone, q)
        assert mb == ml, q
        lone.close()
    batch.close()


def test_a_nan_trial_is_not_postprocessed_and_its_neighbours_are(fv):
    FVSolver, BatchedFVSolver = fv
    common = dict(YAML, tolerance=1e-5, max_iterations=2000, check_every=256, vortex_metrics="device")
    trials = [dict(common, nx=16, ny=16, Re=100.0),
              dict(common, nx=16, ny=16, Re=1000.0, alpha_uv=1.0, alpha_p=1.0),
              dict(common, nx=24, ny=16, Re=400.0)]
    batch = BatchedFVSolver(trials)
    out = batch.solve()
    assert list(batch.errors) == [1] and out[1] is None
    assert "psi" not in batch.solvers[1].t and batch.solvers[1]._post is None
    for q in (0, 2):
        lone = FVSolver(**trials[q])
        lone.solve()
        mb, ml = _same_solve(batch.solvers[q], lone, q)
        assert mb == ml and mb["psi_min"] < 0 and "psi" in batch.solvers[q].t, q
        lone.close()
    batch.close()


# ------------------------------------------------------------------------------------------- h. launcher
def test_launcher_takes_the_override(tmp_path):
    recs = {}
    for mode, extra in (("host", []), ("device", ["+solver.vortex_metrics=device"])):
        d = tmp_path / mode
        d.mkdir()
        r = subprocess.run([sys.executable, str(PKG / "main.py"), "solver=fv", "N=16", "Re=100", "tolerance=1e-5"] + extra,
                           cwd=d, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        recs[mode] = json.loads(next(d.rglob("results.json")).read_text())["metrics"]
    h, d = recs["host"], recs["device"]
    assert h["iterations"] == d["iterations"] and h["converged"] == d["converged"] == 1 and h["psi_min"] < 0
    # bounds of (a) at 16 x 16 with |u|, |v| <= lid = 1: omega 4 eps (16 + 16); psi 4 eps kappa max|psi|, max|psi| = |psi_min|
    bw = 4 * EPS * 32
    bp = 4 * EPS * P.kappa(16, 16, 1 / 16, 1 / 16) * abs(h["psi_min"])
    for k in h:
        if k == "wall_time_seconds":
            continue
        if k in PSI_KEYS:
            assert abs(d[k] - h[k]) <= bp, k
        elif k in OMEGA_KEYS:
            assert abs(d[k] - h[k]) <= bw, k
        else:
            assert d[k] == h[k], (k, d[k], h[k])
