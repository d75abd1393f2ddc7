"""Post-processing and prolongation of chip and shared finite-volume trials on the GPU (ldc_fv_wide_post_enqueue,
``vortex_metrics="chip"``, ldc_fv_wide_prolong_enqueue).  Up to 256 cells per axis the yardstick is the one-CU kernel, bit
for bit; above, the host path of the same solver object, the long-double solve of tests/fv_post_numpy.py and the NumPy
prolongation of tests/fv_prolong_numpy.py, with the bounds of tests/test_gpu_fv_post.py and tests/test_gpu_fv_prolong.py."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import fv_post_numpy as P  # noqa: E402
import fv_prolong_numpy as PR  # noqa: E402
from fv_numpy import FVState  # noqa: E402
from fv_post_numpy import LD  # noqa: E402

from conftest import PKG  # noqa: E402

pytestmark = pytest.mark.gpu

YAML = dict(name="fv", convection_scheme="TVD", alpha_uv=0.4, alpha_p=0.2, linear_solver_tol=1e-9)      # conf/solver/fv.yaml
PSI_KEYS = ("psi_min", "psi_BR", "psi_BL", "psi_TL")
OMEGA_KEYS = ("omega_center", "omega_max")
STATE = ("u", "v", "p", "mdot")
# 8 x 8: one partial tile, K no multiple of 4; 19 x 19: one tile + 1; 37 x 50: eight work-groups, several slots to merge;
# 256 x 256: G at its cap, exactly one pass
SMALL = [(8, 8, 1.0, 1.0), (19, 19, 1.0, 1.0), (37, 50, 2.0, 0.5), (9, 250, 1.0, 1.0), (256, 256, 1.0, 1.0)]
# 300 x 260: 78 000 cells, a second grid-stride pass at G = 256
LARGE = [(300, 260, 1.0, 1.0), (8, 300, 1.0, 1.0), (300, 9, 1.0, 1.0)]


@pytest.fixture(scope="module")
def fv():
    import __graft_entry__ as g
    g.build()
    from solvers.fv import ldc_fv_lib as F
    from solvers.fv import solver as S
    return S, F


def _solver(S, nx, ny, Lx=1.0, Ly=1.0, mapping="chip", **kw):
    return S.FVSolver(**dict(dict(YAML, Re=100.0, nx=nx, ny=ny, Lx=Lx, Ly=Ly, mapping=mapping, vortex_metrics="chip"), **kw))


def _set(s, u, v):
    s.set_state(u, v, np.zeros(s.n_cells), np.zeros(s.t["mdot"].numel()))
    s._finalize_fields()


def _metrics(s, mode):
    keep = s.params.vortex_metrics
    s.params.vortex_metrics = mode
    try:
        return s.compute_vortex_metrics()
    finally:
        s.params.vortex_metrics = keep


def _post(S, s, mode):
    """(psi, omega, result block) of the current state by ``postprocess`` in ``mode``, into poisoned arrays."""
    keep = s.params.vortex_metrics
    s.params.vortex_metrics = mode
    try:
        for name in ("psi", "omega"):
            if name in s.t:
                s.t[name].fill_(float("nan"))
        s.t["work"][: 32 * s.n_cells].fill_(float("nan"))        # (work vectors carry nothing between launches)
        S.postprocess([s])
        r, s._post = s._post, None
        return s.t["psi"].cpu().numpy().copy(), s.t["omega"].cpu().numpy().copy(), r
    finally:
        s.params.vortex_metrics = keep


# ------------------------------------------------------------------------------------------- 1. the one-CU kernel's bits
@pytest.mark.parametrize("shape", SMALL, ids=P.shape_id)
def test_chip_chain_leaves_the_bits_of_the_one_cu_kernel(fv, shape):
    S, F = fv
    nx, ny, Lx, Ly = shape
    s = _solver(S, nx, ny, Lx, Ly)
    _set(s, *P.random_state(nx, ny))
    assert S.post_route("chip", s._has_cu_handle) == "chip" and S.post_route("device", s._has_cu_handle) == "cu"
    psi_c, om_c, r_c = _post(S, s, "chip")
    psi_d, om_d, r_d = _post(S, s, "device")
    assert np.all(np.isfinite(psi_d)) and np.all(np.isfinite(om_d)) and r_d[F.POST_NONFINITE] == 0 and r_d[F.POST_PSI_MIN] < 0
    assert np.array_equal(om_c, om_d)
    assert np.array_equal(psi_c, psi_d)
    assert r_c.shape == (F.POST_RESULT_LEN,) and np.array_equal(r_c, r_d), (r_c, r_d)
    assert _metrics(s, "chip") == _metrics(s, "device")
    s.close()


# ------------------------------------------------------------------------------------------- 2. above 256 cells
@pytest.mark.parametrize("shape", LARGE, ids=P.shape_id)
def test_above_256_cells_against_the_host_path_and_long_double(fv, shape):
    """omega within 4 eps max(|u|, |v|, lid)(1/dx + 1/dy) of ``_vorticity``; psi within 4 eps kappa max|psi| of the
    long-double solve; the ring exactly 0.0; the metrics are the extrema rule on the device's own fields and within the
    same bounds of the host branch."""
    S, F = fv
    nx, ny, Lx, Ly = shape
    with pytest.raises(ValueError, match="vortex_metrics='device'"):        # the one-CU route stays closed here
        _solver(S, nx, ny, Lx, Ly, vortex_metrics="device")
    s = _solver(S, nx, ny, Lx, Ly)
    assert s.handle is None
    _set(s, *P.random_state(nx, ny))
    omega = s._vorticity()
    psi_host = s._streamfunction(omega)
    psi_ld = P.psi_solve(omega, s.dx_min, s.dy_min, LD)
    bw = P.omega_bound(s.fields.u, s.fields.v, s.params.lid_velocity, s.dx_min, s.dy_min)
    bp = P.psi_bound(psi_ld, nx, ny, s.dx_min, s.dy_min)
    w, psi = s.vorticity(), s.streamfunction()
    assert w.shape == psi.shape == (ny, nx)
    ew, ep = float(np.max(np.abs(w - omega))), float(np.max(np.abs(psi.astype(LD) - psi_ld)))
    print(f"FVWIDEPOST {nx}x{ny}: omega err {ew:.2e} (bound {bw:.2e}); psi err {ep:.2e} (bound {bp:.2e}), "
          f"kappa {P.kappa(nx, ny, s.dx_min, s.dy_min):.2e}")
    assert np.all(np.isfinite(w)) and np.all(np.isfinite(psi))
    assert ew <= bw
    assert ep <= bp
    for ring in (psi[0], psi[-1], psi[:, 0], psi[:, -1]):
        assert np.all(ring == 0.0) and not np.any(np.signbit(ring))
    # precondition, on the host values: no extremum can move to another cell inside the bounds
    gaps = P.runner_up_gaps(psi_host, omega, s._mask_bounds)
    assert gaps["omega_max"] > 2 * bw and all(gaps[k] > 2 * bp for k in PSI_KEYS), gaps
    host = _metrics(s, "host")
    dev = _metrics(s, "chip")
    assert dev == P.extrema(psi, w, s._mask_bounds, *P.cell_centres(nx, ny, Lx, Ly))
    assert set(dev) == set(host)
    for k in host:
        if k in PSI_KEYS:
            assert abs(dev[k] - host[k]) <= bp, (k, dev[k], host[k])
        elif k in OMEGA_KEYS:
            assert abs(dev[k] - host[k]) <= bw, (k, dev[k], host[k])
        else:
            assert dev[k] == host[k], (k, dev[k], host[k])
    s.close()


# ------------------------------------------------------------------------------------------- 3. ties, the zero branch
def test_ties_and_the_zero_branch_across_work_groups(fv):
    """20 x 26 cells are three work-groups, and the lid row (cells 500 ... 519) lies in the second and the third: the tie
    of |omega| along it, and that of psi == 0 over all cells, go to the lowest cell whichever slot holds it."""
    S, F = fv
    nx, ny = 20, 26
    s = _solver(S, nx, ny)
    assert F.wide_groups(nx, ny) == 3 and (ny - 1) * nx < 512 < nx * ny
    xs, ys = P.cell_centres(nx, ny, 1.0, 1.0)
    X = np.meshgrid(xs, ys)[0].ravel()
    zeros = {f"psi_{r}{t}": 0.0 for r in ("BR", "BL", "TL") for t in ("", "_x", "_y")}
    _set(s, np.zeros(nx * ny), np.zeros(nx * ny))
    dev = _metrics(s, "chip")
    w, psi = s.vorticity(), s.streamfunction()
    assert np.all(psi == 0.0) and not np.any(np.signbit(psi)) and np.all(w[:-1] == 0.0) and np.all(w[-1] == -1.0 / s.dy_min)
    assert dev == _metrics(s, "host") == _metrics(s, "device")
    assert dev == dict(zeros, psi_min=0.0, psi_min_x=xs[0], psi_min_y=ys[0], omega_center=0.0,
                       omega_max=-1.0 / s.dy_min, omega_max_x=xs[0], omega_max_y=ys[-1])
    # u = 0, v = -x: omega < 0 in the interior, psi < 0 there, all corners zero
    _set(s, np.zeros(nx * ny), -X)
    w, psi = s.vorticity(), s.streamfunction()
    assert np.all(w[1:-1, 1:-1] < 0) and np.all(psi[1:-1, 1:-1] < 0)
    dev = _metrics(s, "chip")
    assert dev == _metrics(s, "device")
    assert {k: dev[k] for k in zeros} == zeros and dev["psi_min"] < 0
    # omega = 10 ... 11 in the rows j <= 3 and -2 ... -3 above: a positive corner value in BR and BL, none in TL
    rng = np.random.default_rng(7)
    rows = np.arange(ny)[:, None] * np.ones((1, nx))
    omega = np.where(rows <= 3, 10.0 + rng.random((ny, nx)), -2.0 - rng.random((ny, nx)))
    v = np.zeros((ny, nx))
    for i in range(1, nx - 1):
        v[:, i + 1] = v[:, i - 1] + 2 * s.dx_min * omega[:, i]
    _set(s, np.zeros(nx * ny), v.ravel())
    dev, host = _metrics(s, "chip"), _metrics(s, "host")
    assert host["psi_BR"] > 0 and host["psi_BL"] > 0 and host["psi_TL"] == 0.0
    assert dev == _metrics(s, "device")
    assert dev["psi_BR"] > 0 and dev["psi_BL"] > 0 and (dev["psi_TL"], dev["psi_TL_x"], dev["psi_TL_y"]) == (0.0, 0.0, 0.0)
    bp = P.psi_bound(s._streamfunction(s._vorticity()), nx, ny, s.dx_min, s.dy_min)
    for k in PSI_KEYS:
        assert abs(dev[k] - host[k]) <= bp, k
    s.close()


# ------------------------------------------------------------------------------------------- 4. a NaN
@pytest.mark.parametrize("shape", [(37, 50), (300, 9)], ids=lambda z: f"{z[0]}x{z[1]}")
def test_a_nan_in_u_sets_the_not_finite_word(fv, shape):
    S, F = fv
    nx, ny = shape
    s = _solver(S, nx, ny)
    u, v = P.random_state(nx, ny)
    u[nx * (ny // 2) + nx // 3] = np.nan
    _set(s, u, v)
    S.postprocess([s])
    assert s._post is not None and s._post[F.POST_NONFINITE] != 0
    with pytest.raises(FloatingPointError):
        s.compute_vortex_metrics()
    s.close()


# ------------------------------------------------------------------------------------------- 5. the trial is left alone
def _left_alone(S, make, advance):
    runs = {}
    for post in (True, False):
        ss = make()
        for s in ss:
            s._begin(1e-30)
        rows = [advance(ss)]
        if post:
            S.postprocess(ss)
            assert all(s._post is not None and s._post[0] < 0 for s in ss)
        rows.append(advance(ss))
        runs[post] = ([s.state() for s in ss], [np.concatenate([a[q] for a in rows]) for q in range(len(ss))],
                      [s.t["ctrl"].cpu().numpy().copy() for s in ss], [s.counters() for s in ss])
        for s in ss:
            s.close()
    (sa, ra, ca, na), (sb, rb, cb, nb) = runs[True], runs[False]
    for q in range(len(sa)):
        for k in STATE:
            assert np.array_equal(sa[q][k], sb[q][k]), (q, k)
        assert ra[q].shape == (40, 8) and np.array_equal(ra[q], rb[q]), q
        assert np.array_equal(ca[q], cb[q]) and na[q] == nb[q] and na[q]["iterations"] == 40, q


def test_postprocessing_leaves_a_chip_trial_alone(fv):
    S, F = fv
    _left_alone(S, lambda: [_solver(S, 37, 50, tolerance=1e-30, check_every=64)], lambda ss: [ss[0]._advance(20)[0]])


def test_postprocessing_leaves_a_shared_batch_alone(fv):
    S, F = fv
    batches = []

    def make():
        ss = [_solver(S, 37, 50, mapping="shared", tolerance=1e-30, check_every=64, Re=Re) for Re in (100.0, 400.0)]
        batches.append(S.SharedBatch(ss))
        return ss

    _left_alone(S, make, lambda ss: [out[0] for out in batches[-1].advance([20, 20])])
    for b in batches:
        b.close()


# ------------------------------------------------------------------------------------------- 6. solve()
def _solve_metrics(s):
    m = s.metrics.as_dict()
    m.pop("wall_time_seconds")
    return m


def test_solve_in_chip_mode_gives_the_metrics_of_device_mode(fv):
    S, F = fv
    common = dict(tolerance=1e-5, max_iterations=20000, check_every=256)
    chip, dev = _solver(S, 24, 24, **common), _solver(S, 24, 24, vortex_metrics="device", **common)
    chip.solve()
    dev.solve()
    assert chip.metrics.converged and np.array_equal(chip.history, dev.history)
    mc, md = _solve_metrics(chip), _solve_metrics(dev)
    assert mc == md and mc["psi_min"] < 0, (mc, md)
    assert "psi" in chip.t and "post_scratch" in chip.t and "post_scratch" not in dev.t
    chip.close(), dev.close()
    # a batch of shared trials post-processes its "chip"-mode trials in the same call as its "device"-mode ones
    from solvers.fv.batched import BatchedFVSolver
    trials = [dict(YAML, Re=100.0, nx=24, ny=24, mapping="shared", vortex_metrics=vm, **common) for vm in ("chip", "device", "host")]
    batch = BatchedFVSolver(trials)
    batch.solve()
    assert batch.errors == {}
    mb = [_solve_metrics(s) for s in batch.solvers]
    assert mb[0] == mb[1] == mc and "psi" in batch.solvers[0].t and "psi" not in batch.solvers[2].t
    batch.close()


def test_launcher_takes_the_override(fv, tmp_path):
    sys.path.insert(0, str(PKG))
    from utilities.config import compose as Cmp
    args = ["solver=fv", "N=24", "Re=100", "tolerance=1e-5", "+solver.mapping=chip"]
    r = subprocess.run([sys.executable, str(PKG / "main.py")] + args + ["+solver.vortex_metrics=chip"], cwd=tmp_path,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads(next(tmp_path.rglob("results.json")).read_text())["metrics"]
    cfg = Cmp.resolve(Cmp.compose_job(Cmp.Composer(PKG / "conf"), args + ["+solver.vortex_metrics=device"], []))
    s = Cmp.instantiate(dict(cfg["solver"]))
    assert s.params.mapping == "chip" and s.params.vortex_metrics == "device"
    s.solve()
    want = json.loads(json.dumps(s.metrics.to_mlflow()))
    s.close()
    assert got["converged"] == 1 and got["psi_min"] < 0
    for k in want:
        if k != "wall_time_seconds":
            assert got[k] == want[k], (k, got[k], want[k])


# ------------------------------------------------------------------------------------------- 7. prolongation
def _trial(S, size, iters=0, Re=100.0, **kw):
    s = _solver(S, size[0], size[1], Re=Re, tolerance=1e-30, check_every=16, vortex_metrics="host", **kw)
    if iters:
        s._begin(1e-30)
        s._advance(iters)
    return s


def _poison(s):
    s.set_state(*(np.full(s.t[k].numel(), np.nan) for k in STATE))


def _wide_prolong(F, c, f):
    import torch
    F.wide_prolong_enqueue(c._wide, f._wide, torch.cuda.current_stream(f.device).cuda_stream)
    torch.cuda.current_stream(f.device).synchronize()


@pytest.mark.parametrize("coarse,fine", [((24, 24), (40, 40)), ((13, 17), (37, 50))], ids=["24-40", "13x17-37x50"])
def test_chip_prolongation_leaves_the_bits_of_the_one_cu_kernel(fv, coarse, fine):
    S, F = fv
    c, a, b = _trial(S, coarse, iters=6), _trial(S, fine, iters=2), _trial(S, fine, iters=2)
    _poison(a), _poison(b)
    keep = {k: b.t[k].cpu().numpy().copy() for k in ("ctrl", "rec", "work", "scratch")}
    before = c.state()
    assert S.prolong_route(c._has_cu_handle, a._has_cu_handle, c.chip, a.chip) == "cu"
    S.prolong([(c, a)])                           # ldc_fv_prolong_enqueue
    _wide_prolong(F, c, b)                        # ldc_fv_wide_prolong_enqueue
    sa, sb = a.state(), b.state()
    for k in STATE:
        assert np.all(np.isfinite(sa[k])) and np.max(np.abs(sa[k])) > 0 and np.array_equal(sa[k], sb[k]), k
    for k, was in keep.items():                   # nothing else written
        assert np.array_equal(was, b.t[k].cpu().numpy(), equal_nan=True), k
    after = c.state()
    assert all(np.array_equal(before[k], after[k]) for k in STATE)
    for s in (c, a, b):
        s.close()


def _restated(coarse, fine):
    c = FVState(coarse.nx, coarse.ny, 100.0)
    c.set_state(**coarse.state())
    c.ulid = coarse.t["ulid"].cpu().numpy()
    f = FVState(fine.nx, fine.ny, 100.0)
    PR.prolong(c, f)
    return dict(u=f.u.ravel(), v=f.v.ravel(), p=f.p.ravel(), mdot=PR.mdot(f))


def test_prolongation_above_256_cells_matches_the_restatement(fv):
    S, F = fv
    c, f = _trial(S, (150, 140), iters=6), _trial(S, (300, 280))
    _poison(f)
    assert f.handle is None and S.prolong_route(c._has_cu_handle, f._has_cu_handle, c.chip, f.chip) == "chip"
    S.prolong([(c, f)])
    got, want = f.state(), _restated(c, f)
    for k in STATE:
        scale, diff = float(np.max(np.abs(want[k]))), float(np.max(np.abs(got[k] - want[k])))
        print("150x140 -> 300x280", k, "max|field|", scale, "max|device - restatement|", diff)
        assert np.all(np.isfinite(got[k])) and scale > 0 and diff <= 1e-13 * scale, k
    assert got["p"][0] == 0.0
    nx, ny = 300, 280
    fx, fy = got["mdot"][: ny * (nx + 1)].reshape(ny, nx + 1), got["mdot"][ny * (nx + 1):].reshape(ny + 1, nx)
    for wall in (fx[:, 0], fx[:, -1], fy[0, :], fy[-1, :]):
        assert np.all(wall == 0.0) and not np.any(np.signbit(wall))
    # a one-CU coarse trial cannot feed a trial that has no one-CU handle
    cu = _trial(S, (150, 140), mapping="cu")
    with pytest.raises(ValueError, match="give the coarse trial mapping='chip'"):
        S.prolong([(cu, f)])
    for s in (c, f, cu):
        s.close()


def test_start_from_above_256_cells(fv):
    S, F = fv
    a, b = _trial(S, (300, 260), iters=4), _trial(S, (300, 260), Re=400.0)
    _poison(b)
    b.start_from(a)                               # continuation in Re at equal size: the identity on u and v
    sa, sb = a.state(), b.state()
    assert np.max(np.abs(sa["u"])) > 0 and np.array_equal(sa["u"], sb["u"]) and np.array_equal(sa["v"], sb["v"])
    assert sb["p"][0] == 0.0 and np.all(np.isfinite(sb["p"])) and np.all(np.isfinite(sb["mdot"]))
    # a coarser trial to start from, then the fine trial goes on
    c = _trial(S, (150, 130), iters=8)
    _poison(b)
    b.start_from(c)
    b._begin(1e-30)
    rows, done, total = b._advance(10)
    assert rows.shape == (10, 8) and total == 10 and np.all(np.isfinite(rows)) and not done
    assert all(np.all(np.isfinite(x)) for x in b.state().values())
    for s in (a, b, c):
        s.close()
