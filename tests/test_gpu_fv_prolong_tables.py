"""The coarse-to-fine transfer on tensor grids with any spacing per axis on the GPU (ldc_fv_prolong_tables_enqueue through
``solvers.fv.solver.prolong`` with ``transfer="tables"`` on the fine trial) against the NumPy restatement of
tests/fv_prolong_tables_numpy.py applied to the downloaded coarse state, bit for bit: every pair of grids the kernel treats
differently, what it writes and what it leaves alone, calls of several pairs against lone ones, the refusals, and a uniform
pair against the equal-spacing kernel."""
import ctypes as C
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import fv_prolong_tables_numpy as T  # noqa: E402
from fv_stretched_numpy import axis_tables, tanh_vertices  # noqa: E402

pytestmark = pytest.mark.gpu

YAML = dict(name="fv", convection_scheme="TVD", alpha_uv=0.4, alpha_p=0.2, linear_solver_tol=1e-9)      # conf/solver/fv.yaml
# (coarse, fine) as (nx, ny, beta; None: a uniform trial) and the domain: the smallest size; odd sizes on grids that do not
# nest, unequal beta, another domain; a uniform source; a finer source (coarse intervals without a fine centre) into a uniform
# trial served by equal-spacing tables; equal grids; the largest size and the longest bisection (256 is LDC_FV_MAX_N)
CASES = [((8, 8, 1.5), (16, 16, 1.5), {}),
         ((12, 8, 2.5), (25, 17, 1.0), dict(Lx=2.0, Ly=0.5)),
         ((16, 16, None), (37, 37, 1.5), {}),
         ((37, 37, 1.5), (16, 16, None), {}),
         ((32, 32, 1.5), (32, 32, 1.5), {}),
         ((128, 128, 1.5), (256, 256, 1.5), {})]
STATE = ("u", "v", "p", "mdot")


@pytest.fixture(scope="module")
def fv():
    import __graft_entry__ as g
    g.build()
    from solvers.fv import ldc_fv_lib as F
    from solvers.fv.solver import FVSolver, prolong
    return FVSolver, prolong, F


def _trial(FVSolver, spec, geo=None, lid="none", seed=None, transfer="tables", Re=100.0):
    """A trial of ``spec`` at rest, or with a seeded random state (u, v, p and mdot all non-trivial); a uniform source keeps
    the default ``transfer`` unless told otherwise."""
    nx, ny, beta = spec
    grid = dict(grid="uniform") if beta is None else dict(grid="tanh", grid_stretch=beta)
    s = FVSolver(**dict(YAML, nx=nx, ny=ny, Re=Re, corner_treatment=lid, tolerance=1e-30, check_every=8, transfer=transfer,
                        **grid, **(geo or {})))
    if seed is not None:
        rng = np.random.default_rng(seed)
        s.set_state(*(rng.standard_normal(s.t[k].numel()) for k in STATE))
    return s


def _poison(s):
    s.set_state(*(np.full(s.t[k].numel(), np.nan) for k in STATE))


def _tables(s):
    """The restatement's view of a device trial: the tables of its mesh, nothing else."""
    p = s.params
    beta = float(p.grid_stretch) if s.stretched else 0.0
    o = SimpleNamespace(nx=s.nx, ny=s.ny, rho=1.0, Lx=float(p.Lx), Ly=float(p.Ly))
    o.xc, o.hx, o.dxf, o.gxf = axis_tables(tanh_vertices(s.nx, p.Lx, beta))
    o.yc, o.hy, o.dyf, o.gyf = axis_tables(tanh_vertices(s.ny, p.Ly, beta))
    return o


def _restated(coarse, fine):
    """The restatement applied to the coarse trial's downloaded state, in the layout of ``state()``."""
    c, f = _tables(coarse), _tables(fine)
    st = coarse.state()
    c.u, c.v, c.p = (st[k].reshape(coarse.ny, coarse.nx) for k in ("u", "v", "p"))
    c.ulid = coarse.t["ulid"].cpu().numpy()
    T.prolong(c, f)
    return dict(u=f.u.ravel(), v=f.v.ravel(), p=f.p.ravel(), mdot=T.mdot(f))


def _untouched(s):
    return {k: s.t[k].cpu().numpy().copy() for k in ("ctrl", "rec", "work", "ulid")}


@pytest.mark.parametrize("lid", ["none", "smoothing"])
@pytest.mark.parametrize("coarse,fine,geo", CASES)
def test_device_matches_the_restatement_bit_for_bit(fv, coarse, fine, geo, lid):
    FVSolver, prolong, F = fv
    c = _trial(FVSolver, coarse, geo, lid, seed=17, transfer="uniform")
    f = _trial(FVSolver, fine, geo, lid, seed=19)
    _poison(f)
    f.t["ctrl"].fill_(7)                          # (set_state zeroes the words: give the kernel something to spoil)
    f.t["rec"].fill_(0.25)
    before_c, before_f = dict(c.state(), **_untouched(c)), _untouched(f)
    prolong([(c, f)])
    got, want = f.state(), _restated(c, f)
    for k in STATE:
        diff = float(np.max(np.abs(got[k] - want[k]))) if np.all(np.isfinite(got[k])) else float("nan")
        print(coarse, fine, lid, k, "max|field|", float(np.max(np.abs(want[k]))), "max|device - restatement|", diff)
        assert np.all(np.isfinite(got[k])) and np.array_equal(got[k], want[k]), k
    # exact zeros: the pinned cell and the fluxes through the four walls
    assert got["p"][0] == 0.0
    nx, ny = f.nx, f.ny
    fx, fy = got["mdot"][: ny * (nx + 1)].reshape(ny, nx + 1), got["mdot"][ny * (nx + 1):].reshape(ny + 1, nx)
    for wall in (fx[:, 0], fx[:, -1], fy[0, :], fy[-1, :]):
        assert np.all(wall == 0.0) and not np.any(np.signbit(wall))
    assert np.max(np.abs(fx)) > 0 and np.max(np.abs(fy)) > 0
    if coarse == fine:                            # equal grids: the identity on u and v, p minus p[0]
        assert np.array_equal(got["u"], before_c["u"]) and np.array_equal(got["v"], before_c["v"])
        assert np.array_equal(got["p"], before_c["p"] - before_c["p"][0])
    # nothing else written: the coarse trial, and the fine trial's control words, record and work vectors
    after_c, after_f = dict(c.state(), **_untouched(c)), _untouched(f)
    for k in before_c:
        assert np.array_equal(before_c[k], after_c[k], equal_nan=True), ("coarse", k)
    for k in before_f:
        assert np.array_equal(before_f[k], after_f[k], equal_nan=True), ("fine", k)
    # repeating the transfer gives the same bits
    _poison(f)
    prolong([(c, f)])
    again = f.state()
    assert all(np.array_equal(again[k], got[k]) for k in STATE)
    c.close(), f.close()


def test_the_lid_profile_reaches_the_rows_under_the_lid(fv):
    """A coarse trial at rest: the only non-zero input is its lid profile, and it must show in the fine top row."""
    FVSolver, prolong, F = fv
    c, f = _trial(FVSolver, (8, 8, 1.5), lid="saad"), _trial(FVSolver, (16, 16, 1.5), lid="saad")
    _poison(f)
    prolong([(c, f)])
    got, want = f.state(), _restated(c, f)
    u = got["u"].reshape(16, 16)
    assert np.all(u[:-1] == 0.0) and np.all(u[-1, 1:-1] > 0) and np.array_equal(got["u"], want["u"])
    assert np.all(got["v"] == 0.0) and np.all(got["p"] == 0.0) and np.all(got["mdot"][16 * 17:] == 0.0)
    c.close(), f.close()


def test_one_call_of_three_pairs_equals_three_calls(fv):
    FVSolver, prolong, F = fv
    pairs = [(_trial(FVSolver, c, geo, "smoothing", seed=30 + q, transfer="uniform", Re=100.0 * (q + 1)), _trial(FVSolver, f, geo))
             for q, (c, f, geo) in enumerate(CASES[:3])]
    for _, f in pairs:
        _poison(f)
    prolong(pairs)
    together = [f.state() for _, f in pairs]
    for _, f in pairs:
        _poison(f)
    for pair in pairs:
        prolong([pair])
    for q, (c, f) in enumerate(pairs):
        alone, want = f.state(), _restated(c, f)
        for k in STATE:
            assert np.array_equal(alone[k], together[q][k]) and np.array_equal(alone[k], want[k]), (q, k)
    for c, f in pairs:
        c.close(), f.close()


def test_more_pairs_than_a_launch_takes(fv):
    """2 * LAUNCH_MAX + 2 pairs of 8^2 -> 16^2 in ONE call, three launches of the library, from three coarse states in turn:
    every fine trial, the ones at the launch boundaries included, gets the bits of its lone transfer."""
    FVSolver, prolong, F = fv
    m = F.PROLONG_TABLES_LAUNCH_MAX
    n = 2 * m + 2
    assert F.lib().ldc_fv_prolong_tables_launches(n) == 3
    coarse = [_trial(FVSolver, (8, 8, 1.5), seed=40 + q, transfer="uniform") for q in range(3)]
    fines = [_trial(FVSolver, (16, 16, 1.5)) for _ in range(n)]
    for f in fines:
        _poison(f)
    prolong([(coarse[q % 3], f) for q, f in enumerate(fines)])
    together = [f.state() for f in fines]
    want = [_restated(c, fines[0]) for c in coarse]
    for q in range(n):
        assert all(np.array_equal(together[q][k], want[q % 3][k]) for k in STATE), q
    for q in (0, m - 1, m, 2 * m - 1, 2 * m, n - 1):
        _poison(fines[q])
        prolong([(coarse[q % 3], fines[q])])
        alone = fines[q].state()
        assert all(np.array_equal(alone[k], together[q][k]) for k in STATE), q
    for s in coarse + fines:
        s.close()


def test_refusals_come_back_without_a_launch(fv):
    FVSolver, prolong, F = fv
    import torch
    L, J = F.lib(), F.ProlongTablesJob
    call = L.ldc_fv_prolong_tables_enqueue
    a, b, c = (_trial(FVSolver, (8, 8, 1.5), seed=1), _trial(FVSolver, (12, 12, 1.5), seed=2), _trial(FVSolver, (16, 16, None), seed=3))
    before = [s.state() for s in (a, b, c)]
    stream = C.c_void_p(a._stream())
    ab, bc, ac = b._prolong_tables_job(a), c._prolong_tables_job(b), c._prolong_tables_job(a)

    def changed(job, **over):
        out = J.from_buffer_copy(job)
        for k, v in over.items():
            setattr(out, k, v)
        return out
    assert call(None, 1, stream) == -1 and call(C.byref(ab), 0, stream) == -1
    for over in (dict(coarse_u=None), dict(fine_mdot=None), dict(fine_xc=None), dict(coarse_yc=None), dict(fine_x_grid=None),
                 dict(coarse_nx=7), dict(fine_ny=257), dict(fine_nx=0), dict(Lx=0.0), dict(rho=-1.0)):
        assert call(C.byref(changed(ab, **over)), 1, stream) == -1, over
        assert call((J * 2)(ac, changed(ab, **over)), 2, stream) == -1, over
    assert call(C.byref(a._prolong_tables_job(a)), 1, stream) == -1                    # onto itself
    assert call((J * 2)(ab, ab), 2, stream) == -1                                     # one fine trial twice
    assert call((J * 2)(ab, bc), 2, stream) == -1                                     # a chain in one call
    assert call((J * 2)(bc, ab), 2, stream) == -1
    assert call((J * 2)(ac, changed(ab, fine_p=ac.fine_mdot)), 2, stream) == -1       # one array of two jobs' results
    with pytest.raises(ValueError, match="a fine trial is the coarse or the fine trial of another pair"):
        prolong([(a, b), (b, c)])
    with pytest.raises(ValueError, match="cover one domain"):
        wide = _trial(FVSolver, (12, 12, 1.5), dict(Lx=2.0))
        try:
            prolong([(a, wide)])
        finally:
            wide.close()
    torch.cuda.synchronize()
    for s, st in zip((a, b, c), before):
        now = s.state()
        assert all(np.array_equal(now[k], st[k]) for k in STATE)
    assert call((J * 2)(ab, ac), 2, stream) == 0                                      # one coarse trial, two fine: a valid call
    torch.cuda.synchronize()
    for f in (b, c):
        got, want = f.state(), _restated(a, f)
        assert all(np.array_equal(got[k], want[k]) for k in STATE)
    for s in (a, b, c):
        s.close()


@pytest.mark.parametrize("sizes", [((8, 8), (16, 16)), ((12, 8), (25, 17)), ((16, 16), (37, 37))])
def test_a_uniform_pair_agrees_with_the_equal_spacing_kernel(fv, sizes):
    """The same uniform pair through ``transfer="tables"`` and through the default: to rounding, not bit for bit (the centres are
    vertex midpoints here and (k + 1/2) h there).  Both routes in ONE ``prolong`` call."""
    FVSolver, prolong, F = fv
    (cx, cy), (fx, fy) = sizes
    c = _trial(FVSolver, (cx, cy, None), lid="smoothing", seed=50, transfer="uniform")
    f0 = _trial(FVSolver, (fx, fy, None), transfer="uniform")
    f1 = _trial(FVSolver, (fx, fy, None), transfer="tables")
    assert not f0.transfer_tables and f1.transfer_tables
    for f in (f0, f1):
        _poison(f)
    prolong([(c, f0), (c, f1)])
    old, new = f0.state(), f1.state()
    for k in STATE:
        err = float(np.max(np.abs(old[k] - new[k])) / np.max(np.abs(old[k])))
        print(sizes, k, "max relative difference between the two kernels", err)
        assert np.all(np.isfinite(new[k])) and err <= 1e-13, k
    assert all(np.array_equal(new[k], _restated(c, f1)[k]) for k in STATE)
    for s in (c, f0, f1):
        s.close()
