"""A spectral trial started from a finite-volume solution on the GPU: ``ldc_fv_sample_nodes`` against the NumPy
restatement (tests/fv_sample_numpy.py), the packing of jobs into launches, ``SGSolver.start_from`` on every kernel
mapping against ``OracleSG`` stepped from the restatement's transferred state, ``initial_guess="fv"`` end to end, in a
batch, and with a seed that fails.  Every comparison prints its figures before it asserts (run with -s)."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import fv_sample_numpy as S  # noqa: E402
from fv_numpy import FVState, lid_profile  # noqa: E402
from fv_post_numpy import random_state  # noqa: E402
from oracle import ldc_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu

# (FV cells nx, ny, Lx, Ly) -> (nodes Mx, My, basis)
SHAPES = [((8, 8, 1.0, 1.0), (5, 5, "chebyshev")),
          ((13, 17, 1.0, 1.0), (25, 41, "chebyshev")),
          ((37, 50, 2.0, 0.5), (17, 17, "legendre")),
          ((256, 256, 1.0, 1.0), (33, 33, "chebyshev")),
          ((300, 260, 1.0, 1.0), (129, 65, "chebyshev"))]
SG = dict(name="spectral", basis_type="chebyshev", CFL=1.5, beta_squared=5.0, corner_treatment="smoothing",
          corner_smoothing=0.15, multigrid="none", max_iterations=200000, check_every=256, graph_iters=16)


@pytest.fixture(scope="module")
def mods():
    import __graft_entry__ as g
    g.build()
    import torch
    from solvers.fv import ldc_fv_lib as F
    from solvers.fv.solver import FVSolver
    from solvers.spectral import warm_start as W
    from solvers.spectral.batched import BatchedSGSolver
    from solvers.spectral.sg import SGSolver
    return dict(torch=torch, F=F, FVSolver=FVSolver, SGSolver=SGSolver, BatchedSGSolver=BatchedSGSolver, W=W)


def _source(nx, ny, Lx, Ly, seed=None):
    """A seeded FV state as ``fv_post_numpy.random_state`` seeds its fields (p: the same generator, one seed further)."""
    u, v = random_state(nx, ny, seed)
    p, _ = random_state(nx, ny, (1000 * nx + ny if seed is None else seed) + 1)
    return dict(u=u.reshape(ny, nx), v=v.reshape(ny, nx), p=p.reshape(ny, nx), ulid=lid_profile(nx, Lx, 1.0, "saad"),
                dx=Lx / nx, dy=Ly / ny)


def _target(Mx, My, kind, Lx, Ly):
    x, y = orc.Axis(Mx - 1, Lx, kind).x, orc.Axis(My - 1, Ly, kind).x
    return dict(x=x, y=y, ulid_nodes=orc.lid_profile(x, "smoothing", 0.15, 1.0, Lx))


def _restated(src, tgt):
    return S.sample(src["u"], src["v"], src["p"], src["ulid"], src["dx"], src["dy"], tgt["x"], tgt["y"], tgt["ulid_nodes"])


def _device_call(mods, cases, one_by_one=False):
    """``ldc_fv_sample_nodes`` on (source, target) pairs: ONE call for all of them, or one call each; outputs start as NaN."""
    torch, F = mods["torch"], mods["F"]
    dev = torch.device("cuda:0")
    up = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=np.float64).ravel(), dtype=torch.float64, device=dev)  # noqa: E731
    keep, jobs, outs = [], [], []
    for src, tgt in cases:
        ny, nx = src["u"].shape
        Mx, My = tgt["x"].size, tgt["y"].size
        t = {k: up(src[k]) for k in ("u", "v", "p", "ulid")}
        t.update({k: up(tgt[k]) for k in ("x", "y", "ulid_nodes")})
        U, V = (torch.full((Mx * My,), float("nan"), dtype=torch.float64, device=dev) for _ in range(2))
        Pi = torch.full(((Mx - 2) * (My - 2),), float("nan"), dtype=torch.float64, device=dev)
        keep.append(t)
        outs.append((U, V, Pi, Mx, My))
        jobs.append(F.SampleJob(u=t["u"].data_ptr(), v=t["v"].data_ptr(), p=t["p"].data_ptr(), ulid=t["ulid"].data_ptr(),
                                nx=nx, ny=ny, dx=src["dx"], dy=src["dy"], x=t["x"].data_ptr(), y=t["y"].data_ptr(),
                                ulid_nodes=t["ulid_nodes"].data_ptr(), Mx=Mx, My=My, U=U.data_ptr(), V=V.data_ptr(),
                                P=Pi.data_ptr()))
    stream = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        if one_by_one:
            for j in jobs:
                F.sample_nodes([j], stream)
        else:
            F.sample_nodes(jobs, stream)
        torch.cuda.current_stream(dev).synchronize()
    return [(U.cpu().numpy().reshape(Mx, My), V.cpu().numpy().reshape(Mx, My), Pi.cpu().numpy().reshape(Mx - 2, My - 2))
            for U, V, Pi, Mx, My in outs]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _check_against_restatement(tag, got, want, tgt):
    for name, g, w in zip(("U", "V", "P"), got, want):
        assert g.shape == w.shape and np.all(np.isfinite(g)), (tag, name)
        inner = (slice(1, -1), slice(1, -1)) if name != "P" else (slice(None), slice(None))
        scale, diff = float(np.max(np.abs(w[inner]))), float(np.max(np.abs(g[inner] - w[inner])))
        print(f"SAMPLE {tag} {name}: max|field| {scale:.3e}, max|device - restatement| {diff:.3e}")
        assert diff <= 1e-13 * scale, (tag, name, diff, scale)
    U, V, _ = got
    for f in (U, V):                                    # the three walls: == 0.0
        assert np.all(f[0, :-1] == 0.0) and np.all(f[-1, :-1] == 0.0) and np.all(f[:, 0] == 0.0)
    assert np.all(V[:, -1] == 0.0)
    assert np.array_equal(_bits(U[:, -1]), _bits(tgt["ulid_nodes"]))          # the lid, top corners included: the target's bits


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("cells,nodes", SHAPES, ids=lambda s: "x".join(str(v) for v in s[:2]))
def test_kernel_matches_the_restatement(mods, cells, nodes):
    nx, ny, Lx, Ly = cells
    Mx, My, kind = nodes
    src, tgt = _source(nx, ny, Lx, Ly), _target(Mx, My, kind, Lx, Ly)
    got = _device_call(mods, [(src, tgt)])[0]
    _check_against_restatement(f"{nx}x{ny}->{Mx}x{My}", got, _restated(src, tgt), tgt)


def test_nodes_on_cell_centres_and_on_the_walls(mods):
    """Interior nodes exactly on a cell centre (weight 0.0 at its own node), on x = 0 and x = Lx, y = 0 and y = Ly (the
    ring itself: the first and the last interval of the extended axis), and one ulp either side of a centre."""
    nx, ny, Lx, Ly = 16, 12, 2.0, 0.5
    src = _source(nx, ny, Lx, Ly)
    xc, yc = (np.arange(nx) + 0.5) * src["dx"], (np.arange(ny) + 0.5) * src["dy"]
    x = np.array([0.0, 0.0, xc[0], np.nextafter(xc[3], 0.0), xc[3], np.nextafter(xc[3], 9.0), 0.77, xc[15], Lx, Lx])
    y = np.array([0.0, 0.0, yc[0], yc[5], 0.3, yc[11], Ly, Ly])
    tgt = dict(x=x, y=y, ulid_nodes=np.linspace(0.25, 1.0, x.size))
    got = _device_call(mods, [(src, tgt)])[0]
    want = _restated(src, tgt)
    _check_against_restatement("centres and walls", got, want, tgt)
    U, V, Pi = got
    assert U[4, 3] == src["u"][5, 3] and V[4, 3] == src["v"][5, 3] and Pi[3, 2] == src["p"][5, 3]      # on a centre: the cell
    assert np.all(U[1, 1:-1] == 0.0) and np.all(U[-2, 1:-1] == 0.0) and np.all(V[1:-1, 1] == 0.0)       # on a wall: the ring
    assert np.abs(U[2:8, -2]).min() > 0.0                                                             # on y = Ly: the FV lid
    assert np.all(Pi[0, :] == Pi[1, :]) and np.all(Pi[:, 0] == Pi[:, 1])                                 # p: zero gradient


# ------------------------------------------------------------------------------------------------ packing
def test_more_jobs_than_a_launch_holds_equal_the_jobs_one_by_one(mods):
    """70 jobs of three shapes and seventy seeds in ONE call (launches of 32, 32 and 6) against seventy calls of one."""
    F = mods["F"]
    shapes = [((9, 10, 1.0, 1.0), (7, 12, "chebyshev")), ((24, 16, 2.0, 0.5), (33, 17, "legendre")),
              ((40, 40, 1.0, 1.0), (21, 21, "chebyshev"))]
    n = 2 * F.SAMPLE_LAUNCH_MAX + 6
    cases = []
    for q in range(n):
        (nx, ny, Lx, Ly), (Mx, My, kind) = shapes[q % 3]
        cases.append((_source(nx, ny, Lx, Ly, seed=77 + q), _target(Mx, My, kind, Lx, Ly)))
    together = _device_call(mods, cases)
    alone = _device_call(mods, cases, one_by_one=True)
    for q, (a, b) in enumerate(zip(together, alone)):
        for name, fa, fb in zip("UVP", a, b):
            assert np.all(np.isfinite(fa)) and np.array_equal(_bits(fa), _bits(fb)), (q, name)
    # a job does not change with its neighbours: job 5 among others, and among other others
    again = _device_call(mods, [cases[40], cases[5], cases[12]])
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(again[1], together[5]))
    for q in (0, 31, 32, 63, 64, n - 1):                # both sides of every launch boundary against the restatement
        _check_against_restatement(f"job {q}", together[q], _restated(*cases[q]), cases[q][1])


# ------------------------------------------------------------------------------------------------ SGSolver.start_from
FV_YAML = dict(name="fv", convection_scheme="TVD", alpha_uv=0.4, alpha_p=0.2, linear_solver_tol=1e-9)


def _developed_fv(mods, nx, ny, mapping, Re=100.0, iters=40, **kw):
    extra = dict(pressure_equation="consistent") if mapping != "cu" else {}
    fv = mods["FVSolver"](**dict(FV_YAML, nx=nx, ny=ny, Re=Re, corner_treatment="smoothing", tolerance=1e-30,
                                 check_every=64, mapping=mapping, **extra, **kw))
    fv._begin(1e-30)
    fv._advance(iters)
    return fv


def _restated_fv(fv, Lx=1.0, Ly=1.0):
    st = fv.state()
    s = FVState(fv.nx, fv.ny, 100.0, Lx=Lx, Ly=Ly)
    s.set_state(**st)
    s.ulid = fv.t["ulid"].cpu().numpy()
    return s


# launch path (N = 20), the one-XCD kernel at M - 1 a multiple of 16 (N = 32: the tail layout, _prime must not refuse),
# the chip-wide kernel (N = 96); the source trial in each of its mappings
START_FROM = [(20, 0, "cu", "legendre"), (32, 3, "chip", "chebyshev"), (96, 5, "shared", "chebyshev")]


@pytest.mark.parametrize("N,mode,mapping,kind", START_FROM, ids=lambda v: str(v))
def test_start_from_then_thirty_iterations_vs_oracle(mods, N, mode, mapping, kind):
    fv = _developed_fv(mods, 32, 24, mapping)
    s = mods["SGSolver"](**dict(SG, Re=100.0, nx=N, ny=N, tolerance=1e-6, persistent=mode, basis_type=kind))
    s.start_from(fv)
    o = S.put(orc.OracleSG(N, 100.0, basis_type=kind), _restated_fv(fv))
    u0 = s.arrays.u.reshape(N + 1, N + 1)
    print(f"START_FROM N={N}: transferred max|u| {np.abs(o.u[1:-1, 1:-1]).max():.3e}, max|u - restatement| "
          f"{np.abs(u0 - o.u).max():.3e}")
    assert np.abs(o.u[1:-1, 1:-1]).max() > 0.05 and np.abs(o.v).max() > 0.01 and np.abs(o.p).max() > 1e-3      # developed
    assert np.array_equal(_bits(u0[:, -1]), _bits(s.u_lid)) and not u0[0].any() and not u0[-1, :-1].any()
    rec = s.run_iterations(30)
    assert s.kernel_mode == mode and (mode != 3 or s.tail == 1)
    for _ in range(30):
        o.step()
    du = float(np.max(np.abs(s.arrays.u.reshape(N + 1, N + 1) - o.u)))
    dv = float(np.max(np.abs(s.arrays.v.reshape(N + 1, N + 1) - o.v)))
    dp = float(np.max(np.abs(s.arrays.p.reshape(N - 1, N - 1) - o.p)))
    print(f"START_FROM N={N} mode {mode}: after 30 iterations max|du| {du:.2e} max|dv| {dv:.2e} max|dp| {dp:.2e}")
    assert rec.shape == (30, 8) and np.all(np.isfinite(rec))
    assert du < 1e-11 and dv < 1e-11 and dp < 1e-11, (du, dv, dp)
    s.close(), fv.close()


def test_two_domains_are_refused_before_any_launch(mods):
    fv = _developed_fv(mods, 16, 16, "cu", iters=3, Lx=2.0)
    s = mods["SGSolver"](**dict(SG, Re=100.0, nx=16, ny=16, tolerance=1e-6))
    before = s.arrays.u.copy()
    with pytest.raises(ValueError, match="two domains"):
        s.start_from(fv)
    assert np.array_equal(before, s.arrays.u)
    s.close(), fv.close()


# ------------------------------------------------------------------------------------------------ initial_guess="fv"
def test_end_to_end_the_seed_cuts_the_iteration_count(mods):
    """N = 24, Re = 100, tolerance 1e-6.  The restatement's ratio at N = 16 is 8 528 / 14 155 = 0.6025, above 0.6, so the
    test runs at N = 24, where the restatement gives 13 383 / 32 333 = 0.41 with the product's default seed (24 x 24 cells
    with the trial's own lid profile, 138 FV iterations to 1e-4)."""
    kw = dict(SG, Re=100.0, nx=24, ny=24, tolerance=1e-6)
    rest = mods["SGSolver"](**kw)
    rest.solve()
    s = mods["SGSolver"](**kw, initial_guess="fv")
    s.solve()
    info = s.initial_guess_info
    print(f"END TO END N=24: from rest {rest.metrics.iterations}, from the seed {s.metrics.iterations} "
          f"(ratio {s.metrics.iterations / rest.metrics.iterations:.3f}); seed {info}")
    assert rest.metrics.converged and rest.initial_guess_info is None
    assert s.metrics.converged and info["used"] and info["converged"] and info["cells"] == (24, 24)
    assert 10 < info["iterations"] < 2000 and info["wall_time_seconds"] > 0
    assert s.metrics.wall_time_seconds > info["wall_time_seconds"]
    assert s.metrics.iterations <= 0.7 * rest.metrics.iterations
    # The same fixed point by two paths, each ended by the stop rule.  On the restatement the from-rest field sits 3.9e-4 and
    # the seeded one 4.4e-4 (maximum norm, the larger of u and v) from the field converged to 1e-9: at most 8.3e-4 apart by
    # the triangle inequality; the device's seed differs from the restatement's at rounding level, twice that is allowed.
    d = max(float(np.max(np.abs(s.fields.u - rest.fields.u))), float(np.max(np.abs(s.fields.v - rest.fields.v))))
    print(f"END TO END N=24: max|seeded - from rest| over u, v {d:.2e}")
    assert d < 2 * 8.3e-4
    rest.close(), s.close()


def test_a_batch_equals_its_lone_solves_bit_for_bit(mods):
    """Three trials on one unequal grid (16 x 20), two Re and two lid profiles, seeded together (one shared FV batch, one
    transfer call) against three lone solves (a chip FV trial each).  (Re = 200, not 400: 16 x 20 nodes do not hold
    Re = 400, the spectral iteration leaves the finite numbers after 2 010 iterations from rest too.)"""
    base = dict(SG, nx=16, ny=20, tolerance=1e-5, persistent=3, initial_guess="fv")
    trials = [dict(base, Re=100.0), dict(base, Re=200.0), dict(base, Re=100.0, corner_smoothing=0.1)]
    batch = mods["BatchedSGSolver"](trials)
    batch.solve()
    for q, (t, b) in enumerate(zip(trials, batch.solvers)):
        lone = mods["SGSolver"](**t)
        lone.solve()
        print(f"BATCH trial {q}: iterations {b.metrics.iterations} / {lone.metrics.iterations}, seed "
              f"{b.initial_guess_info['iterations']} / {lone.initial_guess_info['iterations']}")
        assert b.initial_guess_info["used"] and lone.initial_guess_info["used"]
        assert b.initial_guess_info["cells"] == lone.initial_guess_info["cells"] == (16, 20)
        assert b.initial_guess_info["iterations"] == lone.initial_guess_info["iterations"]
        assert b.metrics.converged and b.metrics.iterations == lone.metrics.iterations
        for name in ("u", "v", "p"):
            assert np.array_equal(_bits(getattr(b.arrays, name)), _bits(getattr(lone.arrays, name))), (q, name)
        lone.close()
    batch.close()


def test_a_failed_seed_starts_from_rest(mods):
    """8 x 8 cells at Re = 1000 with relaxation 0.9 / 0.9 diverge (tests/test_fv_sample_cpu.py shows it on the restatement):
    a numerical divergence in a healthy kernel.  The trial then is the from-rest trial: its count and its fields."""
    kw = dict(SG, Re=1000.0, nx=16, ny=16, tolerance=1e-4, max_iterations=30000)
    rest = mods["SGSolver"](**kw)
    rest.solve()
    s = mods["SGSolver"](**kw, initial_guess="fv", initial_guess_cells=8, initial_guess_alpha_uv=0.9, initial_guess_alpha_p=0.9)
    s.solve()
    info = s.initial_guess_info
    print(f"FAILED SEED: {info}; iterations {s.metrics.iterations} / from rest {rest.metrics.iterations}")
    assert not info["used"] and info["reason"] and info["cells"] == (8, 8)
    assert s.metrics.iterations == rest.metrics.iterations and s.metrics.converged == rest.metrics.converged
    for name in ("u", "v", "p"):
        assert np.array_equal(_bits(getattr(s.arrays, name)), _bits(getattr(rest.arrays, name))), name
    rest.close(), s.close()


def test_the_launcher_takes_the_key_for_lone_trials_and_batches(tmp_path):
    """``python main.py -m solver=spectral/sg +solver.initial_guess=fv``: two Re at one N form a batch (one shared FV
    batch seeds both); every record carries the seed, and the counts are those of the lone trial of the same keys."""
    from conftest import PKG
    r = subprocess.run([sys.executable, str(PKG / "main.py"), "-m", "solver=spectral/sg", "+solver.initial_guess=fv",
                        "+solver.persistent=3", "N=16", "Re=50,100", "tolerance=1e-5", "max_iterations=100000"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    recs = sorted((json.loads(f.read_text()) for f in tmp_path.rglob("results.json")), key=lambda x: x["Re"])
    assert [x["Re"] for x in recs] == [50, 100], r.stderr[-3000:]
    from solvers.spectral.sg import SGSolver
    for x in recs:
        assert x["params"]["initial_guess"] == "fv" and x["metrics"]["converged"] == 1 and x["solve_batch_size"] == 2
        seed = x["initial_guess"]
        assert seed["used"] and seed["cells"] == [16, 16] and seed["iterations"] > 10
        lone = SGSolver(**dict(SG, Re=float(x["Re"]), nx=16, ny=16, tolerance=1e-5, max_iterations=100000, persistent=3,
                               initial_guess="fv"))
        lone.solve()
        print(f"LAUNCHER Re={x['Re']}: iterations {x['metrics']['iterations']} / lone {lone.metrics.iterations}, seed "
              f"{seed['iterations']} / {lone.initial_guess_info['iterations']}")
        assert x["metrics"]["iterations"] == lone.metrics.iterations
        assert seed["iterations"] == lone.initial_guess_info["iterations"]
        lone.close()
    log = r.stdout + r.stderr + "".join(f.read_text() for f in tmp_path.rglob("*.log"))
    assert "initial guess: finite-volume seed of 16 x 16 cells" in log, log[-3000:]
