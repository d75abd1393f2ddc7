"""The coarse-to-fine transfer on tensor grids with any spacing per axis over the whole chip on the GPU
(ldc_fv_wide_prolong_tables_enqueue through ``solvers.fv.solver.prolong`` with ``chip_transfer="tables"`` on the fine trial)
against the NumPy restatement of tests/fv_prolong_tables_numpy.py applied to the downloaded coarse state, bit for bit, at
8 ... 1024 cells per axis; against the one-CU table kernel and the equal-spacing chip kernel; calls of several pairs and of
mixed routes; the refusals; and the sequenced and continued solves of stretched chip trials, up to 264 x 264.
``-s`` prints the measured figures; profiles/fv_wide_prolong_tables.md keeps them.  On an MI355X: every bit-for-bit case differs
from the restatement by exactly 0.0; the uniform chip pair differs from the equal-spacing kernel by at most 3.4e-15; 16^2 -> 32^2
takes 441 + 569 iterations (the restatement: 441 + 569) against 864 from rest (864), max |d(u, v)| 1.110e-4, max |dp| 1.068e-3,
first residual 0.105; Re = 400 continued from Re = 100 at 32^2 latches after 509 iterations (715 from rest), first residual
0.029."""
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
# (coarse, fine) as (nx, ny, beta; None: a uniform trial) and the domain: the smallest sizes; grids that do not nest (k = 1 at
# the wall), another domain; a uniform source; a uniform fine trial with the option; equal grids; more than 65 536 fine cells
# (256 work-groups and a second, partial trip of the stride); the longest bisection and the end of the LDS table on either
# axis; a coarse axis longer than the fine one
CASES = [((8, 8, 1.5), (16, 16, 1.5), {}),
         ((12, 8, 2.5), (25, 17, 1.0), dict(Lx=2.0, Ly=0.5)),
         ((16, 16, None), (37, 37, 1.5), {}),
         ((37, 37, 1.5), (16, 16, None), {}),
         ((32, 32, 1.5), (32, 32, 1.5), {}),
         ((132, 125, 1.5), (272, 250, 1.5), {}),
         ((8, 512, 1.5), (8, 1024, 1.5), {}),
         ((512, 8, 1.5), (1024, 8, 1.5), {}),
         ((8, 1024, 1.5), (8, 264, 1.0), {})]
STATE = ("u", "v", "p", "mdot")
SEQ = dict(YAML, mapping="chip", grid="tanh", grid_stretch=1.5, chip_grid="tables", pressure_equation="consistent",
           chip_preconditioner="separable", chip_transfer="tables", Re=100.0, tolerance=1e-6, max_iterations=20000,
           check_every=512)


@pytest.fixture(scope="module")
def fv():
    import __graft_entry__ as g
    g.build()
    from solvers.fv import ldc_fv_lib as F
    from solvers.fv.solver import FVSolver, prolong
    return FVSolver, prolong, F


def _trial(FVSolver, spec, geo=None, lid="none", seed=None, option="tables", Re=100.0, mapping="chip"):
    """A trial of ``spec`` at rest, or with a seeded random state (u, v, p and mdot all non-trivial).  ``mapping="chip"``: a
    chip trial (stretched: with ``chip_grid="tables"``) whose ``chip_transfer`` is ``option``; ``"cu"``: a one-CU trial whose
    ``transfer`` is ``option``."""
    nx, ny, beta = spec
    grid = dict(grid="uniform") if beta is None else dict(grid="tanh", grid_stretch=beta)
    if mapping == "chip":
        grid = dict(grid, mapping="chip", chip_transfer=option, **({} if beta is None else dict(chip_grid="tables")))
    else:
        grid = dict(grid, transfer=option)
    s = FVSolver(**dict(YAML, nx=nx, ny=ny, Re=Re, corner_treatment=lid, tolerance=1e-30, check_every=8, **grid,
                        **(geo or {})))
    if seed is not None:
        rng = np.random.default_rng(seed)
        s.set_state(*(rng.standard_normal(s.t[k].numel()) for k in STATE))
    return s


def _source(FVSolver, spec, geo=None, lid="none", seed=None, Re=100.0):
    """A coarse trial without either option: a one-CU trial where it fits, a chip trial above 256 cells per axis."""
    mapping = "cu" if max(spec[:2]) <= 256 else "chip"
    return _trial(FVSolver, spec, geo, lid, seed, "uniform", Re, mapping)


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


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in STATE)


# ---------------------------------------------------------------------- 1. bit for bit against the restatement
@pytest.mark.parametrize("lid", ["none", "smoothing"])
@pytest.mark.parametrize("coarse,fine,geo", CASES)
def test_device_matches_the_restatement_bit_for_bit(fv, coarse, fine, geo, lid):
    FVSolver, prolong, F = fv
    c = _source(FVSolver, coarse, geo, lid, seed=17)
    f = _trial(FVSolver, fine, geo, lid, seed=19)
    assert f.chip_transfer_tables and not f.transfer_tables and not c.chip_transfer_tables
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
    assert got["p"][0] == 0.0 and not np.signbit(got["p"][0])
    nx, ny = f.nx, f.ny
    fx, fy = got["mdot"][: ny * (nx + 1)].reshape(ny, nx + 1), got["mdot"][ny * (nx + 1):].reshape(ny + 1, nx)
    for wall in (fx[:, 0], fx[:, -1], fy[0, :], fy[-1, :]):
        assert np.all(wall == 0.0) and not np.any(np.signbit(wall))
    assert np.max(np.abs(fx)) > 0 and np.max(np.abs(fy)) > 0
    if coarse == fine:                            # equal grids: the identity on u and v, p minus p[0]
        assert np.array_equal(got["u"], before_c["u"]) and np.array_equal(got["v"], before_c["v"])
        assert np.array_equal(got["p"], before_c["p"] - before_c["p"][0])
    # nothing else written: the coarse trial, and the fine trial's control words, record, work vectors and lid profile
    after_c, after_f = dict(c.state(), **_untouched(c)), _untouched(f)
    for k in before_c:
        assert np.array_equal(before_c[k], after_c[k], equal_nan=True), ("coarse", k)
    for k in before_f:
        assert np.array_equal(before_f[k], after_f[k], equal_nan=True), ("fine", k)
    # repeating the transfer gives the same bits
    _poison(f)
    prolong([(c, f)])
    assert _same(f.state(), got)
    c.close(), f.close()


# ---------------------------------------------------------------------- 2. both table kernels agree
@pytest.mark.parametrize("coarse,fine,geo", [CASES[1], CASES[2], ((128, 128, 1.5), (256, 256, 1.5), {})])
def test_both_table_kernels_give_the_same_bits(fv, coarse, fine, geo):
    """One seeded coarse state into a one-CU trial with ``transfer="tables"`` and into a chip trial with
    ``chip_transfer="tables"``, both routes in ONE call: one statement of the arithmetic, one result."""
    FVSolver, prolong, F = fv
    c = _source(FVSolver, coarse, geo, "smoothing", seed=23)
    f_cu = _trial(FVSolver, fine, geo, "smoothing", option="tables", mapping="cu")
    f_chip = _trial(FVSolver, fine, geo, "smoothing", option="tables", mapping="chip")
    assert f_cu.transfer_tables and f_chip.chip_transfer_tables
    for f in (f_cu, f_chip):
        _poison(f)
    prolong([(c, f_cu), (c, f_chip)])
    a, b = f_cu.state(), f_chip.state()
    for k in STATE:
        assert np.all(np.isfinite(a[k])) and np.array_equal(a[k], b[k]), k
    for s in (c, f_cu, f_chip):
        s.close()


# ---------------------------------------------------------------------- 3. a uniform pair against the equal-spacing kernel
@pytest.mark.parametrize("sizes", [((8, 8), (16, 16)), ((12, 8), (25, 17)), ((16, 16), (37, 37))])
def test_a_uniform_chip_pair_agrees_with_the_equal_spacing_chip_kernel(fv, sizes):
    """The same uniform chip pair through ``chip_transfer="tables"`` and through ``ldc_fv_wide_prolong_enqueue``: to rounding
    (1e-13 relative, the bound of the one-CU counterpart), not bit for bit -- the centres are vertex midpoints here and
    (k + 1/2) h there."""
    FVSolver, prolong, F = fv
    import torch
    (cx, cy), (fx, fy) = sizes
    c = _trial(FVSolver, (cx, cy, None), lid="smoothing", seed=50, option="uniform")
    f0 = _trial(FVSolver, (fx, fy, None), option="uniform")
    f1 = _trial(FVSolver, (fx, fy, None), option="tables")
    for f in (f0, f1):
        _poison(f)
    F.wide_prolong_enqueue(c._wide, f0._wide, c._stream())
    torch.cuda.synchronize()
    prolong([(c, f1)])
    old, new = f0.state(), f1.state()
    for k in STATE:
        err = float(np.max(np.abs(old[k] - new[k])) / np.max(np.abs(old[k])))
        print(sizes, k, "max relative difference between the two chip kernels", err)
        assert np.all(np.isfinite(new[k])) and err <= 1e-13, k
    assert _same(new, _restated(c, f1))
    for s in (c, f0, f1):
        s.close()


# ---------------------------------------------------------------------- 4. calls of several pairs
def test_one_call_of_three_pairs_equals_three_calls(fv):
    FVSolver, prolong, F = fv
    assert F.lib().ldc_fv_wide_prolong_tables_launches(3) == 6
    pairs = [(_source(FVSolver, c, geo, "smoothing", seed=30 + q, Re=100.0 * (q + 1)), _trial(FVSolver, f, geo))
             for q, (c, f, geo) in enumerate((CASES[0], CASES[1], CASES[8]))]
    for _, f in pairs:
        _poison(f)
    prolong(pairs)
    together = [f.state() for _, f in pairs]
    for _, f in pairs:
        _poison(f)
    for pair in pairs:
        prolong([pair])
    for q, (c, f) in enumerate(pairs):
        alone = f.state()
        assert _same(alone, together[q]) and _same(alone, _restated(c, f)), q
    for c, f in pairs:
        c.close(), f.close()


def test_a_call_that_mixes_all_four_routes(fv):
    """``cu`` (a uniform one-CU pair), ``chip`` (a uniform chip pair above 256 cells), ``tables`` (a stretched one-CU pair) and
    the new route (a stretched chip pair) in ONE ``prolong`` call: every fine trial gets the bits of its lone call."""
    FVSolver, prolong, F = fv
    from solvers.fv.solver import prolong_route
    pairs = [(_trial(FVSolver, (8, 8, None), seed=60, option="uniform", mapping="cu"),
              _trial(FVSolver, (16, 16, None), option="uniform", mapping="cu")),
             (_trial(FVSolver, (8, 132, None), seed=61, option="uniform"), _trial(FVSolver, (8, 264, None), option="uniform")),
             (_trial(FVSolver, (12, 8, 2.5), seed=62, option="uniform", mapping="cu"),
              _trial(FVSolver, (25, 17, 1.0), option="tables", mapping="cu")),
             (_trial(FVSolver, (8, 132, 1.5), seed=63, option="uniform"), _trial(FVSolver, (8, 264, 1.5), option="tables"))]
    got = [prolong_route(c._has_cu_handle, f._has_cu_handle, c.chip, f.chip, f.transfer_tables) for c, f in pairs]
    assert got[:3] == ["cu", "chip", "tables"] and pairs[3][1].chip_transfer_tables
    for _, f in pairs:
        _poison(f)
    prolong(pairs)
    together = [f.state() for _, f in pairs]
    for q, (c, f) in enumerate(pairs):
        _poison(f)
        prolong([(c, f)])
        alone = f.state()
        assert all(np.all(np.isfinite(alone[k])) for k in STATE) and _same(alone, together[q]), q
    assert _same(together[3], _restated(*pairs[3])) and _same(together[2], _restated(*pairs[2]))
    for c, f in pairs:
        c.close(), f.close()


# ---------------------------------------------------------------------- 5. refusals at the C ABI
def test_refusals_come_back_without_a_launch(fv):
    FVSolver, prolong, F = fv
    import torch
    L, J = F.lib(), F.ProlongTablesJob
    call = L.ldc_fv_wide_prolong_tables_enqueue
    a, b, c = (_trial(FVSolver, (8, 8, 1.5), seed=1), _trial(FVSolver, (12, 12, 1.5), seed=2), _trial(FVSolver, (16, 16, None), seed=3))
    before = [s.state() for s in (a, b, c)]
    stream = C.c_void_p(a._stream())
    ab, bc, ac = b._prolong_tables_job(a), c._prolong_tables_job(b), c._prolong_tables_job(a)

    def changed(job, **over):
        out = J.from_buffer_copy(job)
        for k, v in over.items():
            setattr(out, k, v)
        return out
    assert call(None, 1, stream) == -1 and call(C.byref(ab), 0, stream) == -1 and call(C.byref(ab), -1, stream) == -1
    nulls = [{k: None} for k, _ in J._fields_[:14]]                # each kind of null pointer
    for over in nulls + [dict(coarse_nx=7), dict(fine_ny=1025), dict(fine_nx=7), dict(coarse_ny=1025), dict(Lx=0.0),
                         dict(rho=-1.0)]:
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
        assert _same(s.state(), st)
    assert call((J * 2)(ab, ac), 2, stream) == 0                                      # one coarse trial, two fine: a valid call
    torch.cuda.synchronize()
    for f in (b, c):
        assert _same(f.state(), _restated(a, f))
    for s in (a, b, c):
        s.close()


# ---------------------------------------------------------------------- 6. - 8. sequenced and continued solves
def test_the_stretched_chip_sequence_ends_where_the_solve_from_rest_ends(fv):
    """16^2 -> 32^2 against the figures of the restatement (SEQ_16_32_*, pinned by tests/test_fv_prolong_tables_cpu.py) with
    the margin tests/test_gpu_fv_fsg_tables.py gives the one-CU route: the chip chain sums in another order."""
    FVSolver, _, _ = fv
    from solvers.fv.fsg import FVFSGSolver
    s = FVFSGSolver(**dict(SEQ, name="fv_fsg", nx=32, ny=32, n_levels=2, coarsest_n=16))
    assert s.level_sizes() == [(16, 16), (32, 32)]
    s.solve()
    lone = FVSolver(**dict(SEQ, nx=32, ny=32))
    lone.solve()
    a, b = s.state(), lone.state()
    duv = max(float(np.max(np.abs(a[k] - b[k]))) for k in ("u", "v"))
    dp = float(np.max(np.abs(a["p"] - b["p"])))
    print("iterations per level", s.level_iterations, "restatement", T.SEQ_16_32_ITERS, "from rest", lone.metrics.iterations,
          "restatement", T.SEQ_16_32_LONE_ITERS, " max |du|, |dv|:", duv, " max |dp|:", dp, " first residuals:",
          s.history[0, 0], lone.history[0, 0])
    assert s.metrics.converged and lone.metrics.converged and s.metrics.final_residual < 1e-6
    assert len(s.level_iterations) == 2 and s.metrics.iterations == s.level_iterations[1] == len(s.history)
    assert all(abs(got - want) <= 1 for got, want in zip(s.level_iterations, T.SEQ_16_32_ITERS))
    assert 0 < duv <= 2 * T.SEQ_16_32_DUV and 0 < dp <= 2 * T.SEQ_16_32_DP
    assert s.history[0, 0] < lone.history[0, 0]
    s.close(), lone.close()


def test_continuation_in_re_on_equal_stretched_chip_grids(fv):
    FVSolver, _, _ = fv
    from solvers.fv.fsg import FVFSGSolver
    common = dict(SEQ, nx=32, ny=32, tolerance=1e-5, check_every=256)
    a = FVSolver(**dict(common, Re=100.0))
    a.solve()
    rest = FVSolver(**dict(common, Re=400.0))
    rest.solve()
    b = FVFSGSolver(**dict(common, name="fv_fsg", Re=400.0))
    b.start_from(a)
    st, src = b.state(), a.state()
    assert np.array_equal(st["u"], src["u"]) and np.array_equal(st["v"], src["v"])      # equal grids: the identity
    assert np.array_equal(st["p"], src["p"] - src["p"][0]) and b.level_sizes() == [(32, 32)]
    b.solve()
    print("Re 100 from rest:", a.metrics.iterations, "; Re 400 from rest:", rest.metrics.iterations, "first residual",
          rest.history[0, 0], "; Re 400 from Re 100:", b.level_iterations, "first residual", b.history[0, 0])
    assert a.metrics.converged and rest.metrics.converged
    assert b.metrics.converged and b.level_iterations == [b.metrics.iterations]
    assert b.history[0, 0] < rest.history[0, 0]
    # ... and a plain FVSolver starts the same way
    d = FVSolver(**dict(common, Re=400.0))
    d.start_from(a)
    assert _same(d.state(), st)
    for s in (a, rest, b, d):
        s.close()


def test_a_sequence_above_256_cells_is_the_same_sequence_done_by_hand(fv):
    """132^2 -> 264^2, 20 iterations per level: no level has a one-CU handle to lean on above 256 cells.  The chip chain
    repeats bit for bit, so any difference from the levels run by hand is the wiring."""
    FVSolver, prolong, _ = fv
    from solvers.fv.fsg import FVFSGSolver, run_level
    kw = dict(SEQ, nx=264, ny=264, max_iterations=20)
    s = FVFSGSolver(**dict(kw, name="fv_fsg", n_levels=2))
    assert s.level_sizes() == [(132, 132), (264, 264)] and s._handle is None
    s.solve()
    assert s.level_iterations == [20, 20] and all(np.all(np.isfinite(v)) for v in s.state().values())
    coarse = FVSolver(**dict(kw, nx=132, ny=132))
    assert run_level(coarse, kw["tolerance"], 20) == (0, 20)
    fine = FVSolver(**kw)
    prolong([(coarse, fine)])
    fine.solve()
    assert fine.metrics.iterations == 20 and not fine.metrics.converged
    assert s.history.shape == fine.history.shape and np.array_equal(s.history, fine.history)
    assert _same(s.state(), fine.state())
    for t in (s, coarse, fine):
        t.close()
