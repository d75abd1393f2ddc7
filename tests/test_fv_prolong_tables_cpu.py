"""The coarse-to-fine transfer on tensor grids with any spacing per axis (transfer="tables", ldc_fv_prolong_tables_enqueue,
csrc/ldc_fv_prolong_tables.hip), CPU side: the parameter surface and the refusals that stay, the C ABI without a device, the
properties of the NumPy restatement (tests/fv_prolong_tables_numpy.py) and the sequenced solve 16^2 -> 32^2 on it."""
import ctypes as C
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
import fv_prolong_numpy as P  # noqa: E402
import fv_prolong_tables_numpy as T  # noqa: E402
from fv_numpy import FVState  # noqa: E402
from fv_stretched_numpy import FVStretchedState  # noqa: E402

from conftest import PKG  # noqa: E402

E_ARG, E_NODEVICE = -1, -3
# (coarse, fine) as (nx, ny, beta or None for a uniform trial), and the domain: the cases of tests/test_gpu_fv_prolong_tables.py
CASES = [((8, 8, 1.5), (16, 16, 1.5), {}),
         ((12, 8, 2.5), (25, 17, 1.0), dict(Lx=2.0, Ly=0.5)),
         ((16, 16, None), (37, 37, 1.5), {}),
         ((37, 37, 1.5), (16, 16, None), {}),
         ((32, 32, 1.5), (32, 32, 1.5), {}),
         ((128, 128, 1.5), (256, 256, 1.5), {})]


def make(spec, geo=None, lid="none"):
    """A state with tables: ``FVStretchedState`` at beta, or a uniform ``FVState`` wrapped with equal-spacing tables."""
    nx, ny, beta = spec
    geo = dict(geo or {})
    if beta is None:
        return T.with_tables(FVState(nx, ny, 100.0, corner_treatment=lid, **geo), **geo)
    return FVStretchedState(nx, ny, 100.0, grid_stretch=beta, corner_treatment=lid, **geo)


def _pair(coarse, fine, geo=None, lid="none", seed=0):
    rng = np.random.default_rng(seed)
    c, f = make(coarse, geo, lid), make(fine, geo, lid)
    c.u, c.v, c.p = (rng.standard_normal((c.ny, c.nx)) for _ in range(3))
    f.u, f.v, f.p = (np.full((f.ny, f.nx), np.nan) for _ in range(3))
    return c, f


# ---------------------------------------------------------------------- the parameter surface
def test_parameter_surface_and_refusals(monkeypatch):
    from solvers.datastructures import FVFSGParameters, FVParameters
    from solvers.fv import solver as S
    from solvers.fv.fsg import _LEVEL_FIELDS, FVFSGSolver
    from solvers.spectral import ldc_lib
    assert FVParameters().transfer == "uniform" and FVFSGParameters().transfer == "uniform"
    assert FVParameters().to_mlflow()["transfer"] == "uniform"
    assert FVParameters(transfer="tables").to_mlflow()["transfer"] == "tables"
    assert S.TRANSFERS == ("uniform", "tables") and "transfer" in _LEVEL_FIELDS
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)        # every ValueError comes before the device
    base = dict(name="fv", Re=100.0, nx=32, ny=32)
    tanh = dict(grid="tanh", pressure_equation="consistent_cu", pressure_preconditioner="separable")
    with pytest.raises(ValueError, match="transfer='nearest': 'uniform' or 'tables'"):
        S.FVSolver(**dict(base, transfer="nearest"))
    for mapping in ("chip", "shared"):
        with pytest.raises(ValueError, match=f"transfer='tables' with mapping='{mapping}'"):
            S.FVSolver(**dict(base, transfer="tables", mapping=mapping))
    # accepted with mapping="cu" on either grid, at both ends of the size range, by the lone and the sequenced solver
    for cls in (S.FVSolver, FVFSGSolver):
        for kw in (dict(), dict(grid="tanh"), tanh, dict(tanh, nx=8, ny=256), dict(nx=256, ny=8), dict(tanh, grid_stretch=0.0)):
            with pytest.raises(ldc_lib.LdcError, match="no CPU fallback"):
                cls(**dict(base, transfer="tables", **kw))
    with pytest.raises(ValueError, match="nx, ny = 257, 32"):
        S.FVSolver(**dict(base, transfer="tables", nx=257))
    # the two pinned refusals: default options, and stand-in objects that have no `transfer_tables`
    with pytest.raises(ValueError, match=r"grid='tanh' with solver=fv/fsg.*transfer='tables'"):
        FVFSGSolver(**dict(base, grid="tanh"))
    with pytest.raises(ValueError, match="grid='tanh' with solver=fv/fsg"):
        FVFSGSolver(**dict(base, **tanh, transfer="uniform"))
    ns = lambda **kw: type("T", (), dict(device=torch.device("cpu"), **kw))()        # noqa: E731
    with pytest.raises(ValueError, match=r"start_from with grid='tanh'.*transfer='tables'"):
        S.prolong([(ns(stretched=False), ns(stretched=True))])
    with pytest.raises(ValueError, match="start_from with grid='tanh'"):
        S.prolong([(ns(stretched=True, stretched_wall=True), ns(stretched=False))])
    # routed by the FINE trial: a stretched coarse trial with the option does not help a fine one without it
    with pytest.raises(ValueError, match="start_from with grid='tanh'"):
        S.prolong([(ns(stretched=True, transfer_tables=True), ns(stretched=True, transfer_tables=False))])
    assert S.prolong_route(True, True, False, False, True) == "tables" and S.prolong_route(True, True, False, False) == "cu"
    assert S.prolong_route(True, True, True, True, True) == "tables" and S.prolong_route(False, False, True, True) == "chip"
    with pytest.raises(ValueError, match="transfer='tables'"):
        S.prolong_route(False, True, True, False, True)          # a coarse trial above 256 cells per axis


def test_the_launcher_composes_the_key():
    sys.path.insert(0, str(PKG))
    from utilities.config import compose as Cmp
    comp = Cmp.Composer(PKG / "conf")
    plain = Cmp.resolve(Cmp.compose_job(comp, ["solver=fv/fsg", "N=32"], []))
    got = Cmp.resolve(Cmp.compose_job(comp, ["solver=fv/fsg", "N=32", "+solver.grid=tanh", "+solver.transfer=tables"], []))
    assert got["solver"] == dict(plain["solver"], grid="tanh", transfer="tables")
    assert "transfer" not in plain["solver"]                      # without the key: the composed config of before
    assert "transfer " in (PKG / "conf" / "solver" / "fv.yaml").read_text()


# ---------------------------------------------------------------------- the C ABI without a device
@pytest.fixture(scope="module")
def fvlib():
    import __graft_entry__ as g
    g.build()
    from solvers.fv import ldc_fv_lib
    return ldc_fv_lib


POINTERS = ("coarse_u", "coarse_v", "coarse_p", "coarse_ulid", "coarse_xc", "coarse_yc", "fine_u", "fine_v", "fine_p",
            "fine_mdot", "fine_x_grid", "fine_y_grid", "fine_xc", "fine_yc")


def _job(F, base=0, **over):
    j = F.ProlongTablesJob()
    for k, n in enumerate(POINTERS):
        setattr(j, n, 4096 * (base + 1) + 8 * k)      # distinct, never dereferenced: validation comes first
    j.Lx, j.Ly, j.rho = 1.0, 1.0, 1.0
    j.coarse_nx, j.coarse_ny, j.fine_nx, j.fine_ny = 16, 12, 32, 25
    for k, v in over.items():
        setattr(j, k, v)
    return j


def test_header_binding_and_exports_agree(fvlib):
    import __graft_entry__ as g
    hdr = (ROOT / "include" / "ldc_fv.h").read_text()
    declared = set(re.findall(r"\b(ldc_[a-z_0-9]+)\s*\(", hdr))
    built = C.CDLL(str(g.LIB))                     # the file build() made, opened anew: its own symbol list
    for name in ("ldc_fv_prolong_tables_enqueue", "ldc_fv_prolong_tables_launches"):
        assert name in declared and name in fvlib.EXPORTS and hasattr(fvlib.lib(), name) and hasattr(built, name)
    assert set(fvlib.EXPORTS) <= declared and all(hasattr(built, name) for name in fvlib.EXPORTS)
    define = lambda n: int(re.search(rf"#define {n} (-?\d+)", hdr).group(1))          # noqa: E731
    m = define("LDC_FV_PROLONG_TABLES_LAUNCH_MAX")
    assert m == fvlib.PROLONG_TABLES_LAUNCH_MAX and define("LDC_FV_PROLONG_LAUNCH_MAX") == 128
    assert define("LDC_FV_VERSION") == 2 == fvlib.VERSION == fvlib.lib().ldc_fv_version()
    # 14 pointers, 3 doubles, 4 int32; the argument block of a launch stays within the 3600 bytes the other units assert,
    # and one job more would not
    size = C.sizeof(fvlib.ProlongTablesJob)
    assert size == 14 * 8 + 3 * 8 + 4 * 4 == 152 and m * size <= 3600 < (m + 1) * size
    body = re.search(r"struct ldc_fv_prolong_tables_job \{(.*?)\};", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"\*?\s*([A-Za-z_]+)\s*(?:,|$)", decl.strip())]
    assert names == [n for n, _ in fvlib.ProlongTablesJob._fields_]
    offsets = [getattr(fvlib.ProlongTablesJob, n).offset for n in names]
    assert offsets == [8 * k for k in range(17)] + [136 + 4 * k for k in range(4)]
    assert g.SRC_FV_PROLONG_TABLES.name == "ldc_fv_prolong_tables.hip" and g.SRC_FV_PROLONG_TABLES.exists()
    assert "csrc/ldc_fv_prolong_tables.hip" in hdr.split(" *\n", 1)[0]          # the unit list at the head
    unit = g.SRC_FV_PROLONG_TABLES.read_text()
    assert "#pragma STDC FP_CONTRACT OFF" in unit and "static_assert(sizeof(FvPtLaunch) <= 3600" in unit


def test_launch_count(fvlib):
    L = fvlib.lib()
    m = fvlib.PROLONG_TABLES_LAUNCH_MAX
    assert [L.ldc_fv_prolong_tables_launches(n) for n in (1, m, m + 1, 2 * m, 2 * m + 2, 256)] == \
        [1, 1, 2, 2, 3, (256 + m - 1) // m]
    assert L.ldc_fv_prolong_tables_launches(0) == E_ARG and L.ldc_fv_prolong_tables_launches(-4) == E_ARG


REFUSED = [{n: None} for n in POINTERS] + [
    dict(coarse_nx=7), dict(coarse_ny=257), dict(fine_nx=0), dict(fine_ny=-3), dict(fine_nx=257), dict(coarse_nx=1024),
    dict(Lx=0.0), dict(Ly=-1.0), dict(rho=0.0), dict(Lx=float("nan"))]


def test_refused_arguments_need_no_device(fvlib):
    L, J = fvlib.lib(), fvlib.ProlongTablesJob
    call = L.ldc_fv_prolong_tables_enqueue
    assert call(None, 1, None) == E_ARG
    assert call(C.byref(_job(fvlib)), 0, None) == E_ARG and call(C.byref(_job(fvlib)), -2, None) == E_ARG
    for over in REFUSED:
        assert call(C.byref(_job(fvlib, **over)), 1, None) == E_ARG, over
        pair = (J * 2)(_job(fvlib), _job(fvlib, 1, **over))                     # the second job of a call is checked too
        assert call(pair, 2, None) == E_ARG, over
    # what a launch writes nobody else in it may touch: a fine field that is a coarse field (of its own job or another's) or a
    # fine field of another job, in any slot and however far apart in the list (beyond one launch too)
    a = _job(fvlib)
    assert call(C.byref(_job(fvlib, fine_u=a.coarse_u)), 1, None) == E_ARG          # onto itself
    assert call(C.byref(_job(fvlib, fine_p=a.fine_v)), 1, None) == E_ARG            # two fields of one job in one array
    for mine in ("fine_u", "fine_v", "fine_p", "fine_mdot"):
        for theirs in ("coarse_u", "coarse_v", "coarse_p", "fine_u", "fine_v", "fine_p", "fine_mdot"):
            pair = (J * 2)(a, _job(fvlib, 1, **{mine: getattr(a, theirs)}))
            assert call(pair, 2, None) == E_ARG, (mine, theirs)
            pair = (J * 2)(_job(fvlib, 1, **{mine: getattr(a, theirs)}), a)
            assert call(pair, 2, None) == E_ARG, (mine, theirs)
    n = 2 * fvlib.PROLONG_TABLES_LAUNCH_MAX + 2
    many = (J * n)(*[_job(fvlib, q) for q in range(n)])
    many[n - 1].fine_mdot = many[0].coarse_p                                          # a chain across launches
    assert call(many, n, None) == E_ARG
    import torch
    if not torch.cuda.is_available():                 # what passes validation: LDC_E_NODEVICE
        shared = (J * 2)(a, _job(fvlib, 1, coarse_u=a.coarse_u, coarse_v=a.coarse_v, coarse_p=a.coarse_p,
                                 fine_x_grid=a.fine_x_grid, fine_xc=a.fine_xc))        # one coarse trial, two fine ones
        assert call(shared, 2, None) == E_NODEVICE
        for ok in (dict(coarse_nx=8, coarse_ny=256, fine_nx=256, fine_ny=8), dict(Lx=2.0, Ly=0.5)):
            assert call(C.byref(_job(fvlib, **ok)), 1, None) == E_NODEVICE, ok
        many[n - 1].fine_mdot = 8
        assert call(many, n, None) == E_NODEVICE


def test_the_solvers_tables_are_the_restatements():
    """``axis_tables`` of the solver on the vertices k L / n: the centres and [h | d | g] a uniform trial is served by."""
    from solvers.fv import solver as S
    for n, L in ((8, 1.0), (37, 2.0), (256, 0.5)):
        xc, h, d, g = S.axis_tables(S.tanh_vertices(n, L, 0.0))
        s = T.with_tables(FVState(n, 8, 100.0, Lx=L), Lx=L)
        assert np.array_equal(xc, s.xc) and np.array_equal(h, s.hx) and np.array_equal(g, s.gxf) and np.array_equal(d, s.dxf)
        assert np.max(np.abs(xc - (np.arange(n) + 0.5) * (L / n))) <= 2e-16 * L and np.max(np.abs(g[1:-1] - 0.5)) <= 1e-13


# ---------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("coarse,fine,geo", CASES)
def test_every_node_and_weight_is_in_range(coarse, fine, geo):
    c, f = make(coarse, geo), make(fine, geo)
    Lx, Ly = T.domain(f)
    assert (Lx, Ly) == (geo.get("Lx", 1.0), geo.get("Ly", 1.0)) == T.domain(c)
    for xc_c, L, xc_f in ((c.xc, Lx, f.xc), (c.yc, Ly, f.yc)):
        k, t = T.locate(xc_c, L, xc_f)
        e = T.nodes(xc_c, L)
        assert np.all(np.diff(e) > 0) and e.size == xc_c.size + 2
        assert k.min() >= 0 and k.max() <= xc_c.size and np.all(np.diff(k) >= 0)
        assert np.all(t >= 0.0) and np.all(t <= 1.0) and np.all(e[k] <= xc_f) and np.all(xc_f <= e[k + 1])
        # bisection as the kernel does it finds the same node
        for x, want in zip(xc_f, k):
            lo, hi = 0, xc_c.size + 1
            while hi - lo > 1:
                mid = (lo + hi) >> 1
                lo, hi = (mid, hi) if e[mid] <= x else (lo, mid)
            assert lo == want
    # both ends of the bisection are met: a first fine centre left of the first coarse centre (k = 0: the wall interval), and,
    # with beta 2.5 under beta 1.0, one to its right (the coarse wall cell is the thinner one: no fine centre in [0, e_1))
    if coarse == (8, 8, 1.5):
        assert T.locate(c.xc, Lx, f.xc)[0][0] == 0 and T.locate(c.yc, Ly, f.yc)[0][-1] == c.ny
    if coarse == (12, 8, 2.5):
        assert T.locate(c.xc, Lx, f.xc)[0][0] == 1 and T.locate(c.yc, Ly, f.yc)[0][0] == 1
    if fine == (16, 16, None):        # a finer source: several coarse intervals hold no fine centre
        assert np.max(np.diff(T.locate(c.xc, Lx, f.xc)[0])) >= 2


BILINEAR = [((16, 16, None), (37, 37, 1.5), {}), ((12, 8, 2.5), (25, 17, 1.0), dict(Lx=2.0, Ly=0.5)),
            ((37, 37, 1.5), (16, 16, None), {}), ((13, 17, 1.5), (29, 31, 0.5), {})]


@pytest.mark.parametrize("coarse,fine,geo", BILINEAR)
def test_a_bilinear_field_with_matching_ring_values_is_reproduced(coarse, fine, geo):
    c, f = make(coarse, geo), make(fine, geo)
    Lx, Ly = T.domain(f)
    bil = lambda X, Y: 0.7 - 1.3 * X + 0.45 * Y + 2.1 * X * Y        # noqa: E731
    ring = bil(*np.meshgrid(T.nodes(c.xc, Lx), T.nodes(c.yc, Ly)))    # the field at every node of the extended axes
    kx, tx = T.locate(c.xc, Lx, f.xc)
    ky, ty = T.locate(c.yc, Ly, f.yc)
    got, want = T.interpolate(ring, kx, tx, ky, ty), bil(*np.meshgrid(f.xc, f.yc))
    err = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
    print(coarse, fine, "bilinear field: max relative error", err)
    assert err <= 1e-13
    # through prolong(): p is the field up to one shift wherever the stencil does not touch the ring
    c.p = bil(*np.meshgrid(c.xc, c.yc))
    T.prolong(c, f)
    inner = ((ky >= 1) & (ky + 1 <= c.ny))[:, None] & ((kx >= 1) & (kx + 1 <= c.nx))[None, :]
    shift = (f.p - want)[inner]
    assert inner.sum() > 0 and np.max(np.abs(shift - shift[0])) <= 1e-13 * np.max(np.abs(want)) and f.p[0, 0] == 0.0


@pytest.mark.parametrize("spec,geo", [((32, 32, 1.5), {}), ((13, 17, 2.5), dict(Lx=2.0, Ly=0.5)), ((9, 13, None), {})])
def test_equal_grids_are_the_identity(spec, geo):
    c, f = _pair(spec, spec, geo, lid="saad", seed=5)
    T.prolong(c, f)
    kx, tx = T.locate(c.xc, T.domain(c)[0], f.xc)
    assert np.array_equal(kx, np.arange(1, c.nx + 1)) and np.all(tx == 0.0)        # every fine centre IS a node
    assert np.array_equal(f.u, c.u) and np.array_equal(f.v, c.v) and np.array_equal(f.p, c.p - c.p[0, 0])


@pytest.mark.parametrize("sizes", [((8, 8), (16, 16)), ((12, 8), (25, 17)), ((16, 16), (37, 37)), ((9, 13), (9, 13))])
@pytest.mark.parametrize("lid", ["none", "saad"])
def test_equal_spacing_agrees_with_the_uniform_restatement(sizes, lid):
    """beta = 0 on both sides against tests/fv_prolong_numpy.py: to rounding, not bit for bit (the centres are
    (xv[k] + xv[k+1]) / 2 there and (k + 1/2) h here)."""
    (cx, cy), (fx, fy) = sizes
    rng = np.random.default_rng(11)
    state = [rng.standard_normal((cy, cx)) for _ in range(3)]
    c0, f0 = FVState(cx, cy, 100.0, corner_treatment=lid), FVState(fx, fy, 100.0, corner_treatment=lid)
    c1, f1 = make((cx, cy, None), lid=lid), make((fx, fy, None), lid=lid)
    for c in (c0, c1):
        c.u, c.v, c.p = (a.copy() for a in state)
    P.prolong(c0, f0)
    T.prolong(c1, f1)
    for name in ("u", "v", "p", "fx", "fy"):
        a, b = getattr(f0, name), getattr(f1, name)
        err = float(np.max(np.abs(a - b)) / np.max(np.abs(a)))
        print(sizes, lid, name, "max relative difference", err)
        assert err <= 1e-13, name
    # ... and the stretched state at beta = 0 is the wrapped uniform one but for the lid (profile at its own centres)
    c2, f2 = make((cx, cy, 0.0), lid=lid), make((fx, fy, 0.0), lid=lid)
    c2.u, c2.v, c2.p, c2.ulid = state[0].copy(), state[1].copy(), state[2].copy(), c1.ulid
    T.prolong(c2, f2)
    assert all(np.array_equal(getattr(f1, k), getattr(f2, k)) for k in ("u", "v", "p", "fx", "fy"))


@pytest.mark.parametrize("coarse,fine,geo", CASES[:5])
@pytest.mark.parametrize("lid", ["none", "saad"])
def test_pinned_cell_and_fluxes(coarse, fine, geo, lid):
    c, f = _pair(coarse, fine, geo, lid, seed=3)
    T.prolong(c, f)
    assert f.p[0, 0] == 0.0 and all(np.all(np.isfinite(a)) for a in (f.u, f.v, f.p, f.fx, f.fy))
    for wall in (f.fx[:, 0], f.fx[:, -1], f.fy[0, :], f.fy[-1, :]):
        assert np.all(wall == 0.0) and not np.any(np.signbit(wall))
    # the inner faces are the state's own face rule times |S|: the fluxes a first SIMPLE iteration forms for itself
    ux, vy = f.faces(f.u, f.v) if hasattr(f, "xv") else T.table_faces(f, f.u, f.v)
    if hasattr(f, "xv"):
        ux, vy = ux[:, 1:-1], vy[1:-1, :]
    assert np.array_equal(f.fx[:, 1:-1], f.rho * (ux * f.hy[:, None]))
    assert np.array_equal(f.fy[1:-1, :], f.rho * (vy * f.hx[None, :]))
    assert T.mdot(f).size == f.ny * (f.nx + 1) + (f.ny + 1) * f.nx
    # the ring: with u = 0 inside, the lid shows in the fine rows above the last coarse centre and nowhere else
    c.u[:] = 0.0
    T.prolong(c, f)
    kx, _ = T.locate(c.xc, T.domain(f)[0], f.xc)
    ky, ty = T.locate(c.yc, T.domain(f)[1], f.yc)
    lid_rows, mid = (ky == c.ny) & (ty > 0), (kx >= 1) & (kx < c.nx)
    assert np.all(f.u[~lid_rows] == 0.0) and np.all(f.u[lid_rows][:, mid] > 0) and mid.sum() >= f.nx // 2
    assert lid_rows.any() == bool(f.yc[-1] > c.yc[-1])


# ---------------------------------------------------------------------- the sequenced solve on the restatement
def test_sequenced_solve_on_the_restatement():
    """16^2 -> 32^2 at beta = 1.5 with the consistent pressure equation and the separable preconditioner: both levels latch,
    and the fine fields are those of the lone run to the bound tests/test_gpu_fv_fsg_tables.py doubles for the device."""
    from fv_separable_numpy import FVSeparableState
    kw = dict(linear_solver_tol=1e-9, convection_scheme="TVD", alpha_uv=0.4, alpha_p=0.2)
    mk = lambda nx, ny: FVSeparableState(nx, ny, 100.0, grid_stretch=1.5, **kw)        # noqa: E731
    sizes = T.hierarchy(32, 32, 2, 16)
    assert sizes == [(16, 16), (32, 32)]
    states, rows = T.sequenced_run(mk, sizes, 1e-6)
    lone = mk(32, 32)
    lone_rows = lone.run(20000, tol=1e-6)
    iters = [len(r) for r in rows]
    f = states[-1]
    duv = max(float(np.max(np.abs(f.u - lone.u))), float(np.max(np.abs(f.v - lone.v))))
    dp = float(np.max(np.abs(f.p - lone.p)))
    print("sequenced", iters, "lone", len(lone_rows), "max|d(u, v)|", duv, "max|dp|", dp)
    assert all(r[-1][0] < 1e-6 for r in rows) and lone_rows[-1][0] < 1e-6
    assert iters == list(T.SEQ_16_32_ITERS) and len(lone_rows) == T.SEQ_16_32_LONE_ITERS
    assert 0.5 * T.SEQ_16_32_DUV <= duv <= T.SEQ_16_32_DUV and 0.5 * T.SEQ_16_32_DP <= dp <= T.SEQ_16_32_DP
    # the prolonged start is a start: the first fine iteration changes the state less than the first one from rest
    assert rows[-1][0][0] < lone_rows[0][0]
