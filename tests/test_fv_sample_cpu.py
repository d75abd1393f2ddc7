"""A spectral trial started from a finite-volume solution (``initial_guess="fv"``, ``ldc_fv_sample_nodes``) without a
device: the NumPy restatement of the transfer (tests/fv_sample_numpy.py) and the iteration counts it gives with the
project's two CPU solvers, the C entry's argument checks, the keys of ``SpectralParameters``, and the plumbing of the
seeds of a lone trial and of a batch with fake solvers."""
import ctypes as C
import re
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import fv_prolong_numpy as P  # noqa: E402
import fv_sample_numpy as S  # noqa: E402
from fv_numpy import FVState  # noqa: E402
from oracle.ldc_oracle import OracleSG  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent

# The counts of DESIGN.md 3 (CPU restatement, tolerance 1e-6, CFL 1.5, Re = 100).  That table seeded with the FV
# restatement's default lid (corner_treatment "none", 32 x 32 cells: 409 iterations); the product's seed takes the spectral
# trial's corner treatment (smoothing 0.15: 408 iterations, 12 574 spectral iterations, measured with the same script).
N24_FROM_REST, N24_FROM_32 = 32333, 12379


# ------------------------------------------------------------------------------------------------ the restatement
def _state(nx, ny, Lx=1.0, Ly=1.0, seed=0):
    s = FVState(nx, ny, 100.0, Lx=Lx, Ly=Ly, corner_treatment="saad")
    rng = np.random.default_rng(seed)
    s.u, s.v, s.p = (rng.normal(size=(ny, nx)) for _ in range(3))
    return s


def test_boundary_nodes_take_the_targets_values_bit_for_bit():
    s = _state(13, 17)
    o = OracleSG(24, 100.0, ny=40)
    U, V, Pi = S.sample_state(s, o.ax.x, o.ay.x, o.u_lid)
    assert U.shape == V.shape == (25, 41) and Pi.shape == (23, 39)
    assert np.array_equal(U[:, -1], o.u_lid) and not V[:, -1].any()
    for f in (U, V):
        assert not f[0, :-1].any() and not f[-1, :-1].any() and not f[:, 0].any()
    want_u, want_v = U.copy(), V.copy()
    o.apply_bc(want_u, want_v)                       # the oracle's own boundary values change nothing
    assert np.array_equal(want_u, U) and np.array_equal(want_v, V)
    assert np.all(np.isfinite(Pi)) and np.abs(U[1:-1, 1:-1]).max() > 0.1


def test_the_restatement_is_the_prolongation_at_cell_centres():
    """Nodes on the centres of a fine FV grid (plus the two walls): U, V are the prolongation's bits, P is its p before the
    shift by the value at cell 0."""
    c, f = _state(12, 9, Lx=2.0, Ly=0.5, seed=3), FVState(25, 17, 100.0, Lx=2.0, Ly=0.5)
    x = np.concatenate([[0.0], (np.arange(f.nx) + 0.5) * f.dx, [f.nx * f.dx]])
    y = np.concatenate([[0.0], (np.arange(f.ny) + 0.5) * f.dy, [f.ny * f.dy]])
    U, V, Pi = S.sample_state(c, x, y, np.zeros(x.size))
    P.prolong(c, f)
    assert np.array_equal(U[1:-1, 1:-1], f.u.T) and np.array_equal(V[1:-1, 1:-1], f.v.T)
    assert np.max(np.abs((Pi - Pi[0, 0]) - f.p.T)) <= 4 * np.finfo(float).eps * np.max(np.abs(Pi))


def test_a_linear_pressure_is_reproduced_between_the_cell_centres():
    """Bilinear interpolation is exact on a + b x + c y wherever all four neighbours are cells (the ring repeats p)."""
    s = _state(16, 20)
    xc, yc = (np.arange(16) + 0.5) * s.dx, (np.arange(20) + 0.5) * s.dy
    s.p = 0.3 + 2.0 * xc[None, :] - 1.5 * yc[:, None]
    o = OracleSG(20, 100.0, basis_type="legendre")
    _, _, Pi = S.sample_state(s, o.ax.x, o.ay.x, o.u_lid)
    X, Y = np.meshgrid(o.ax.x[1:-1], o.ay.x[1:-1], indexing="ij")
    inside = (X >= xc[0]) & (X <= xc[-1]) & (Y >= yc[0]) & (Y <= yc[-1])
    assert inside.sum() > 100
    assert np.max(np.abs(Pi - (0.3 + 2.0 * X - 1.5 * Y))[inside]) < 1e-14
    k, t = S.locate_at(16, s.dx, np.array([0.0, xc[4], 1.0]))           # the wall, a centre, the other wall
    assert k.tolist() == [0, 5, 16] and t.tolist() == [0.0, 0.0, 1.0]


def test_counts_of_the_design_table():
    """N = 24, Re = 100: 32 333 iterations from rest, 12 379 from the 32 x 32 seed (409 FV iterations), with ``OracleSG`` and
    ``FVConsistentState`` as the table of DESIGN.md 3 was taken."""
    seed, fv_its, ok = S.fv_seed(100.0, 32, 32, 1e-6, corner_treatment="none")
    assert ok and fv_its == 409
    its, conv, _ = S.put(OracleSG(24, 100.0), seed).solve(1e-6)
    print("N = 24 from the 32 x 32 seed:", its)
    assert conv and its == N24_FROM_32
    its, conv, _ = OracleSG(24, 100.0).solve(1e-6)
    print("N = 24 from rest:", its)
    assert conv and its == N24_FROM_REST


def test_the_failed_seed_of_the_gpu_test_diverges_on_the_restatement():
    """8 x 8 cells, Re = 1000, relaxation 0.9 / 0.9: not finite after about two hundred iterations."""
    s, its, ok = S.fv_seed(1000.0, 8, 8, 1e-4, alpha_uv=0.9, alpha_p=0.9, max_iter=2000, corner_treatment="smoothing")
    print("the 8 x 8 seed at Re = 1000, 0.9 / 0.9 stops after", its)
    assert not ok and its < 2000 and not np.all(np.isfinite(s.u))


# ------------------------------------------------------------------------------------------------ C ABI
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from solvers.fv import ldc_fv_lib
    return ldc_fv_lib


POINTERS = ("u", "v", "p", "ulid", "x", "y", "ulid_nodes", "U", "V", "P")


def _job(F, **over):
    j = F.SampleJob()
    for n in POINTERS:
        setattr(j, n, 8)                              # never dereferenced: validation comes first
    j.nx, j.ny, j.dx, j.dy, j.Mx, j.My = 32, 20, 1.0 / 32, 1.0 / 20, 25, 17
    for k, v in over.items():
        setattr(j, k, v)
    return j


REFUSED = [{n: None} for n in POINTERS] + [dict(nx=7), dict(ny=7), dict(nx=1025), dict(ny=1025), dict(nx=0), dict(ny=-3),
                                           dict(Mx=2), dict(My=2), dict(Mx=-1), dict(dx=0.0), dict(dy=0.0), dict(dx=-0.1),
                                           dict(dy=float("nan"))]


def test_header_binding_and_exports_agree(lib):
    hdr = (ROOT / "include" / "ldc_fv.h").read_text()
    assert "ldc_fv_sample_nodes" in set(re.findall(r"\b(ldc_[a-z_0-9]+)\s*\(", hdr)) & set(lib.EXPORTS)
    assert hasattr(lib.lib(), "ldc_fv_sample_nodes")
    assert int(re.search(r"#define LDC_FV_SAMPLE_LAUNCH_MAX (\d+)", hdr).group(1)) == lib.SAMPLE_LAUNCH_MAX == 32
    assert C.sizeof(lib.SampleJob) == 112 and lib.SAMPLE_LAUNCH_MAX * C.sizeof(lib.SampleJob) <= 3600
    body = re.search(r"struct ldc_fv_sample_job \{(.*?)\};", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"\*?\s*([A-Za-z_]+)\s*(?:,|$)", decl.strip())]
    assert names == [n for n, _ in lib.SampleJob._fields_]


def test_refused_arguments_need_no_device(lib):
    L = lib.lib()
    assert L.ldc_fv_sample_nodes(None, 1, None) == -1
    assert L.ldc_fv_sample_nodes(C.byref(_job(lib)), 0, None) == -1
    assert L.ldc_fv_sample_nodes(C.byref(_job(lib)), -2, None) == -1
    for over in REFUSED:
        assert L.ldc_fv_sample_nodes(C.byref(_job(lib, **over)), 1, None) == -1, over
        pair = (lib.SampleJob * 2)(_job(lib), _job(lib, **over))          # the second job of a call is checked too
        assert L.ldc_fv_sample_nodes(pair, 2, None) == -1, over
    for ok in (dict(nx=8, ny=1024), dict(Mx=3, My=3)):                    # the ends of the ranges pass validation
        import torch
        if not torch.cuda.is_available():
            assert L.ldc_fv_sample_nodes(C.byref(_job(lib, **ok)), 1, None) == -3          # LDC_E_NODEVICE: past validation


# ------------------------------------------------------------------------------------------------ the keys
OLD_KEYS = {"name", "Re", "lid_velocity", "Lx", "Ly", "nx", "ny", "max_iterations", "tolerance", "method", "basis_type",
            "CFL", "beta_squared", "corner_treatment", "corner_smoothing", "multigrid", "n_levels",
            "coarse_tolerance_factor", "prolongation_method", "restriction_method", "vortex_refine"}
NEW_KEYS = dict(initial_guess="rest", initial_guess_cells=0, initial_guess_tolerance=1e-4, initial_guess_alpha_uv=0.7,
                initial_guess_alpha_p=0.3)


def test_defaults_and_mlflow_keys():
    from solvers.datastructures import SpectralParameters
    p = SpectralParameters(name="spectral", Re=400, nx=64, ny=64, CFL=1.5, basis_type="chebyshev")
    ml = p.to_mlflow()
    assert set(ml) == OLD_KEYS | set(NEW_KEYS)
    assert {k: ml[k] for k in NEW_KEYS} == NEW_KEYS
    assert {k: ml[k] for k in OLD_KEYS} == {k: getattr(p, k) for k in OLD_KEYS}
    ml = SpectralParameters(name="spectral", nx=32, ny=32, initial_guess="fv", initial_guess_cells=48).to_mlflow()
    assert ml["initial_guess"] == "fv" and ml["initial_guess_cells"] == 48


def test_yaml_composes_with_the_override():
    from dataclasses import fields
    from conftest import PKG
    from solvers.datastructures import SpectralParameters
    from utilities.config import compose as Cc
    comp = Cc.Composer(PKG / "conf")
    cfg = Cc.resolve(Cc.compose_job(comp, ["solver=spectral/sg"], []))
    assert not any(k.startswith("initial_guess") for k in cfg["solver"])           # the YAML sets none of them
    cfg = Cc.resolve(Cc.compose_job(comp, ["solver=spectral/sg", "+solver.initial_guess=fv", "N=24", "Re=100"], []))
    kw = {k: v for k, v in cfg["solver"].items() if k != "_target_"}
    assert set(kw) <= {f.name for f in fields(SpectralParameters)}
    p = SpectralParameters(**kw)
    assert p.initial_guess == "fv" and p.nx == 24
    text = (PKG / "conf" / "solver" / "spectral" / "sg.yaml").read_text()
    for k in NEW_KEYS:
        assert re.search(rf"^#\s*{k}:", text, re.M), k                   # documented as comments


def test_key_validation_comes_before_the_device():
    from solvers.spectral.fsg import FSGSolver
    from solvers.spectral.sg import SGSolver
    base = dict(name="spectral", Re=100.0, nx=16, ny=16)
    with pytest.raises(ValueError, match="initial_guess"):
        SGSolver(**base, initial_guess="fvm")
    with pytest.raises(ValueError, match=r"initial_guess.*multigrid|multigrid.*initial_guess"):
        SGSolver(**base, initial_guess="fv", multigrid="fsg")
    with pytest.raises(ValueError, match=r"initial_guess.*multigrid|multigrid.*initial_guess"):
        FSGSolver(**base, initial_guess="fv", multigrid="fsg")
    for bad in (dict(initial_guess_cells=7), dict(initial_guess_cells=1025), dict(initial_guess_tolerance=0.0),
                dict(initial_guess_alpha_uv=0.0), dict(initial_guess_alpha_p=1.5)):
        with pytest.raises(ValueError, match=next(iter(bad))):
            SGSolver(**base, initial_guess="fv", **bad)


def test_the_seed_is_an_fv_trial_of_the_same_cavity():
    from solvers.datastructures import FVParameters, SpectralParameters
    from solvers.spectral import warm_start as W
    p = SpectralParameters(name="spectral", Re=400.0, lid_velocity=1.5, Lx=2.0, Ly=0.5, nx=24, ny=40,
                           corner_treatment="saad", corner_smoothing=0.1, initial_guess="fv", device="cuda:1")
    for mapping in ("chip", "shared"):
        fv = FVParameters(**W.seed_kwargs(p, mapping))
        assert (fv.Re, fv.lid_velocity, fv.Lx, fv.Ly, fv.corner_treatment, fv.corner_smoothing) == \
            (400.0, 1.5, 2.0, 0.5, "saad", 0.1)
        assert (fv.nx, fv.ny) == (24, 40)                                # each axis by its own order
        assert (fv.mapping, fv.pressure_equation, fv.convection_scheme) == (mapping, "consistent", "TVD")
        assert (fv.alpha_uv, fv.alpha_p, fv.tolerance, fv.device) == (0.7, 0.3, 1e-4, "cuda:1")
    assert W.seed_cells(SpectralParameters(nx=12, ny=40)) == (16, 40)
    assert W.seed_cells(SpectralParameters(nx=12, ny=40, initial_guess_cells=64)) == (64, 64)


# ------------------------------------------------------------------------------------------------ plumbing, fake solvers
class FakeSG:
    def __init__(self, guess="fv", **kw):
        from solvers.datastructures import SpectralParameters
        self.params = SpectralParameters(name="spectral", initial_guess=guess, **kw)
        self.initial_guess_info, self.resets, self.metrics = None, 0, None

    def reset_state(self):
        self.resets += 1


class FakeSeeds:
    """What warm_start._SharedSeeds offers: .solvers, .run() -> (latch, nan, iterations) per trial, .close()."""
    made = []

    def __init__(self, trials):
        self.trials = trials
        self.solvers = [SimpleNamespace(nx=t["nx"], ny=t["ny"], kw=t) for t in trials]
        self.closed = False
        FakeSeeds.made.append(self)

    def run(self):
        out = []
        for t in self.trials:                          # Re = 1000 stands for a seed that goes NaN, Re = 2000 for a capped one
            out.append((0, 1, 37) if t["Re"] == 1000.0 else (0, 0, 20000) if t["Re"] == 2000.0 else (1, 0, 400))
        return out

    def close(self):
        self.closed = True


def test_a_batch_runs_one_shared_fv_batch_and_one_transfer_call():
    from solvers.spectral import warm_start as W
    FakeSeeds.made = []
    calls = []
    sgs = [FakeSG(Re=100.0, nx=16, ny=20), FakeSG("rest", Re=100.0, nx=16, ny=20), FakeSG(Re=1000.0, nx=16, ny=20),
           FakeSG(Re=400.0, nx=16, ny=20), FakeSG(Re=2000.0, nx=16, ny=20)]
    W.seed_together(sgs, make_batch=FakeSeeds, transfer=lambda pairs: calls.append(list(pairs)))
    assert len(FakeSeeds.made) == 1 and FakeSeeds.made[0].closed                   # ONE batch of FV trials, closed
    trials = FakeSeeds.made[0].trials
    assert [t["Re"] for t in trials] == [100.0, 1000.0, 400.0, 2000.0]              # the trial from rest has no seed
    assert all(t["mapping"] == "shared" and t["pressure_equation"] == "consistent" and (t["nx"], t["ny"]) == (16, 20)
               for t in trials)
    assert len(calls) == 1                                                         # ONE transfer call ...
    fvs = FakeSeeds.made[0].solvers
    assert calls[0] == [(fvs[0], sgs[0]), (fvs[2], sgs[3])]                        # ... for the seeds that latched
    assert [s.resets for s in sgs] == [0, 0, 1, 0, 1]                              # a failed seed: its own trial from rest
    assert sgs[1].initial_guess_info is None
    assert [sgs[k].initial_guess_info["used"] for k in (0, 2, 3, 4)] == [True, False, True, False]
    info = sgs[0].initial_guess_info
    assert info["cells"] == (16, 20) and info["iterations"] == 400 and info["wall_time_seconds"] >= 0.0
    assert "NaN" in sgs[2].initial_guess_info["reason"] and "20000" in sgs[4].initial_guess_info["reason"]
    # nobody asks: no batch at all
    FakeSeeds.made = []
    assert W.seed_together([FakeSG("rest", nx=16, ny=16)], make_batch=FakeSeeds, transfer=calls.append) == 0.0
    assert not FakeSeeds.made and len(calls) == 1


def test_batched_solve_seeds_before_the_spectral_loop(monkeypatch):
    """``BatchedSGSolver.solve``: seed_together on its solvers, then the unchanged loop."""
    from solvers.spectral import batched as B
    order = []
    monkeypatch.setattr(B.warm_start, "seed_together", lambda solvers: order.append(("seed", list(solvers))))
    monkeypatch.setattr(B, "refine_vortices_together", lambda solvers: None)
    sgs = [FakeSG(Re=100.0, nx=16, ny=16), FakeSG(Re=400.0, nx=16, ny=16)]
    for s in sgs:
        s._store_results = lambda *a, **k: None
    for s in sgs:
        s.M = 17                                       # (from_solvers asks for one size)
    b = B.BatchedSGSolver.from_solvers(sgs)
    monkeypatch.setattr(b, "run_to_tolerance",
                        lambda tols, caps, diag: order.append(("loop",)) or [(1, 100, np.zeros((100, 8)))] * 2)
    b.solve()
    assert [o[0] for o in order] == ["seed", "loop"] and order[0][1] == sgs


def test_a_lone_trial_runs_one_chip_trial_and_closes_it():
    from solvers.spectral import warm_start as W
    made, calls = [], []

    class FakeFV:
        def __init__(self, kw, outcome):
            self.kw, self.nx, self.ny, self.closed, self.outcome = kw, kw["nx"], kw["ny"], False, outcome
            self.params = SimpleNamespace(max_iterations=kw["max_iterations"], tolerance=kw["tolerance"])
            self.rec_cap, self.total = kw["check_every"], 0

        def _begin(self, tol):
            self.begun = tol

        def _advance(self, k):
            self.total += k
            return None, int(self.outcome == "latch" and self.total >= 512), self.total

        def close(self):
            self.closed = True

    for outcome, used in (("latch", True), ("cap", False)):
        sg = FakeSG(Re=100.0, nx=24, ny=24, initial_guess_tolerance=1e-5)
        made.clear(), calls.clear()
        W.seed_alone(sg, make_trial=lambda kw: made.append(FakeFV(kw, outcome)) or made[-1],
                     transfer=lambda pairs: calls.append(list(pairs)))
        fv = made[0]
        assert len(made) == 1 and fv.closed and fv.kw["mapping"] == "chip" and fv.begun == 1e-5
        assert (fv.nx, fv.ny) == (24, 24) and sg.initial_guess_info["used"] is used
        assert calls == ([[(fv, sg)]] if used else []) and sg.resets == (0 if used else 1)
        assert sg.initial_guess_info["iterations"] == (512 if used else W.SEED_MAX_ITERATIONS)
