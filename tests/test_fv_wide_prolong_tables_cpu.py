"""The coarse-to-fine transfer on tensor grids with any spacing per axis over the whole chip (chip_transfer="tables",
ldc_fv_wide_prolong_tables_enqueue, csrc/ldc_fv_wide_prolong_tables.hip), CPU side: the parameter surface, the refusals and what
stays as it was, the C ABI without a device, and the NumPy restatement (tests/fv_prolong_tables_numpy.py, imported) at the
sizes only the chip mapping reaches."""
import ctypes as C
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
import fv_prolong_tables_numpy as T  # noqa: E402
from fv_stretched_numpy import axis_tables, tanh_vertices  # noqa: E402

from conftest import PKG  # noqa: E402

E_ARG, E_NODEVICE = -1, -3
# the cases of tests/test_gpu_fv_wide_prolong_tables.py with a side above 256 cells: (coarse, fine) as (nx, ny, beta)
LARGE = [((132, 125, 1.5), (272, 250, 1.5)),
         ((8, 512, 1.5), (8, 1024, 1.5)),
         ((512, 8, 1.5), (1024, 8, 1.5)),
         ((8, 1024, 1.5), (8, 264, 1.0))]
BASE = dict(name="fv", Re=100.0, nx=32, ny=32)
CHIP = dict(mapping="chip", chip_transfer="tables")
TANH = dict(grid="tanh", grid_stretch=1.5, chip_grid="tables")


@pytest.fixture
def no_device(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)        # every ValueError comes before the device


# ---------------------------------------------------------------------- the parameter surface
def test_the_parameter_its_default_and_where_it_goes():
    from solvers.datastructures import FVFSGParameters, FVParameters
    from solvers.fv import solver as S
    from solvers.fv.fsg import _LEVEL_FIELDS
    assert FVParameters().chip_transfer == "uniform" and FVFSGParameters().chip_transfer == "uniform"
    assert "chip_transfer" in _LEVEL_FIELDS and S.CHIP_TRANSFERS == ("uniform", "tables")
    assert S.TRANSFERS == ("uniform", "tables")                           # a parameter of its own, not a value of `transfer`
    # it changes the start of a solve, as `transfer` does: it goes to MLflow (chip_grid names where the same iteration runs)
    ml = FVParameters(**CHIP).to_mlflow()
    assert ml["chip_transfer"] == "tables" and ml["transfer"] == "uniform" and "chip_grid" not in ml


def test_refused_combinations_name_the_option(no_device):
    from solvers.fv import solver as S
    from solvers.fv.batched import BatchedFVFSGSolver, BatchedFVSolver
    from solvers.fv.fsg import FVFSGSolver
    with pytest.raises(ValueError, match="chip_transfer='nearest': 'uniform' or 'tables'"):
        S.FVSolver(**dict(BASE, chip_transfer="nearest"))
    refused = [dict(chip_transfer="tables"),                                        # mapping "cu" (the default)
               dict(chip_transfer="tables", mapping="cu", grid="tanh"),
               dict(chip_transfer="tables", mapping="shared"),
               dict(CHIP, transfer="tables"),                                       # both transfers
               dict(chip_transfer="tables", mapping="cu", transfer="tables"),
               dict(CHIP, grid="tanh")]                                             # a stretched chip trial without its tables
    for cls in (S.FVSolver, FVFSGSolver):
        for kw in refused:
            with pytest.raises(ValueError, match="chip_transfer"):
                cls(**dict(BASE, **kw))
    for cls in (BatchedFVSolver, BatchedFVFSGSolver):
        for kw in (CHIP, dict(CHIP, **TANH), dict(chip_transfer="tables", mapping="shared"), dict(chip_transfer="tables")):
            with pytest.raises(ValueError, match="chip_transfer"):
                cls([dict(BASE), dict(BASE, **kw)])


def test_accepted_combinations_reach_the_device(no_device):
    from solvers.fv import solver as S
    from solvers.fv.fsg import FVFSGSolver
    from solvers.spectral import ldc_lib
    grids = [dict(), dict(TANH), dict(TANH, chip_preconditioner="laplacian"),
             dict(TANH, pressure_equation="consistent"),
             dict(TANH, pressure_equation="consistent", chip_preconditioner="separable"),
             dict(pressure_equation="consistent")]
    for cls in (S.FVSolver, FVFSGSolver):
        for grid in grids:
            for size in (dict(), dict(nx=8, ny=8), dict(nx=13, ny=17), dict(nx=1024, ny=8)):
                with pytest.raises(ldc_lib.LdcError, match="no CPU fallback"):
                    cls(**dict(BASE, **CHIP, **grid, **size))
    # a sequence needs no one-CU handle on any level: it may end above 256 cells, on either grid
    for n in (16, 300, 1024):
        for grid in (dict(), dict(TANH, pressure_equation="consistent", chip_preconditioner="separable")):
            with pytest.raises(ldc_lib.LdcError, match="no CPU fallback"):
                FVFSGSolver(**dict(BASE, **CHIP, **grid, nx=n, ny=n))
    with pytest.raises(ValueError, match="nx, ny = 1025, 32"):
        S.FVSolver(**dict(BASE, **CHIP, nx=1025))


def test_the_defaults_refuse_what_they_refused(no_device):
    import torch
    from solvers.fv import solver as S
    from solvers.fv.batched import BatchedFVSolver
    from solvers.fv.fsg import FVFSGSolver
    chip = dict(BASE, mapping="chip")
    for kw in (dict(chip, **TANH), dict(chip, **TANH, chip_transfer="uniform")):
        with pytest.raises(ValueError, match=r"grid='tanh' with solver=fv/fsg.*transfer='tables'"):
            FVFSGSolver(**kw)
    with pytest.raises(ValueError, match="an FSG level of 300 x 300 cells"):
        FVFSGSolver(**dict(chip, nx=300, ny=300))
    with pytest.raises(ValueError, match="transfer='tables' with mapping='chip'"):
        S.FVSolver(**dict(chip, transfer="tables"))
    with pytest.raises(ValueError, match="mapping='chip' inside a batch"):
        BatchedFVSolver([dict(chip)])
    ns = lambda **kw: type("T", (), dict(device=torch.device("cpu"), **kw))()        # noqa: E731
    with pytest.raises(ValueError, match=r"start_from with grid='tanh'.*transfer='tables'"):
        S.prolong([(ns(stretched=False), ns(stretched=True))])
    # routed by the FINE trial: the option on the coarse one does not help
    with pytest.raises(ValueError, match="start_from with grid='tanh'"):
        S.prolong([(ns(stretched=True, chip_transfer_tables=True), ns(stretched=True, chip_transfer_tables=False))])
    # prolong_route: the signature and the answers of before
    assert S.prolong_route(True, True, False, False, True) == "tables" and S.prolong_route(True, True, False, False) == "cu"
    assert S.prolong_route(False, False, True, True) == "chip" and S.prolong_route(True, True, True, True) == "cu"
    with pytest.raises(ValueError, match="transfer='tables'"):
        S.prolong_route(False, True, True, False, True)
    with pytest.raises(ValueError, match="whole-chip handles"):
        S.prolong_route(False, True, False, True)


def test_the_launcher_composes_the_key():
    sys.path.insert(0, str(PKG))
    from utilities.config import compose as Cmp
    comp = Cmp.Composer(PKG / "conf")
    plain = Cmp.resolve(Cmp.compose_job(comp, ["solver=fv/fsg", "N=512"], []))
    keys = ["+solver.mapping=chip", "+solver.grid=tanh", "+solver.chip_grid=tables", "+solver.chip_transfer=tables"]
    got = Cmp.resolve(Cmp.compose_job(comp, ["solver=fv/fsg", "N=512"] + keys, []))
    assert got["solver"] == dict(plain["solver"], mapping="chip", grid="tanh", chip_grid="tables", chip_transfer="tables")
    assert "chip_transfer" not in plain["solver"]
    assert "chip_transfer " in (PKG / "conf" / "solver" / "fv.yaml").read_text()


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
    j.coarse_nx, j.coarse_ny, j.fine_nx, j.fine_ny = 300, 12, 1024, 25
    for k, v in over.items():
        setattr(j, k, v)
    return j


def test_header_binding_and_exports_agree(fvlib):
    import __graft_entry__ as g
    hdr = (ROOT / "include" / "ldc_fv.h").read_text()
    declared = set(re.findall(r"\b(ldc_[a-z_0-9]+)\s*\(", hdr))
    built = C.CDLL(str(g.LIB))                     # the file build() made, opened anew: its own symbol list
    for name in ("ldc_fv_wide_prolong_tables_enqueue", "ldc_fv_wide_prolong_tables_launches"):
        assert name in declared and name in fvlib.EXPORTS and hasattr(fvlib.lib(), name) and hasattr(built, name)
    assert set(fvlib.EXPORTS) == declared and all(hasattr(built, name) for name in fvlib.EXPORTS)
    define = lambda n: int(re.search(rf"#define {n} (-?\d+)", hdr).group(1))          # noqa: E731
    assert define("LDC_FV_WIDE_PROLONG_TABLES_LAUNCHES") == 2 == fvlib.WIDE_PROLONG_TABLES_LAUNCHES
    assert define("LDC_FV_WIDE_MAX_N") == 1024 == fvlib.WIDE_MAX_N and C.sizeof(fvlib.ProlongTablesJob) == 152
    assert g.SRC_FV_WIDE_PROLONG_TABLES.name == "ldc_fv_wide_prolong_tables.hip" and g.SRC_FV_WIDE_PROLONG_TABLES.exists()
    head = hdr.split(" *\n", 1)[0]                  # the unit list at the head
    assert "csrc/ldc_fv_wide_prolong_tables.hip" in head and "csrc/ldc_fv_prolong_tables_cells.inc" in head
    # one statement of the arithmetic: both units include it behind the pragma, neither states it again
    inc = g.SRC_FV_PROLONG_TABLES.parent / "ldc_fv_prolong_tables_cells.inc"
    for word in ("struct FvPtAxis", "double pt_node(", "double pt_at(", "double pt_xface(", "double pt_yface("):
        assert word in inc.read_text()
    for unit in (g.SRC_FV_PROLONG_TABLES.read_text(), g.SRC_FV_WIDE_PROLONG_TABLES.read_text()):
        assert unit.index("#pragma STDC FP_CONTRACT OFF") < unit.index('#include "ldc_fv_prolong_tables_cells.inc"')
        assert "struct FvPtAxis" not in unit and "pt_node(const" not in unit


def test_launch_count(fvlib):
    L = fvlib.lib()
    assert [L.ldc_fv_wide_prolong_tables_launches(n) for n in (1, 2, 23, 24, 256)] == [2, 4, 46, 48, 512]
    assert L.ldc_fv_wide_prolong_tables_launches(0) == E_ARG and L.ldc_fv_wide_prolong_tables_launches(-4) == E_ARG


REFUSED = [{n: None} for n in POINTERS] + [
    dict(coarse_nx=7), dict(coarse_ny=1025), dict(fine_nx=0), dict(fine_ny=-3), dict(fine_nx=1025), dict(coarse_nx=4096),
    dict(Lx=0.0), dict(Ly=-1.0), dict(rho=0.0), dict(rho=-1.0), dict(Lx=float("nan"))]


def test_refused_arguments_need_no_device(fvlib):
    L, J = fvlib.lib(), fvlib.ProlongTablesJob
    call = L.ldc_fv_wide_prolong_tables_enqueue
    assert call(None, 1, None) == E_ARG
    assert call(C.byref(_job(fvlib)), 0, None) == E_ARG and call(C.byref(_job(fvlib)), -2, None) == E_ARG
    for over in REFUSED:
        assert call(C.byref(_job(fvlib, **over)), 1, None) == E_ARG, over
        pair = (J * 2)(_job(fvlib), _job(fvlib, 1, **over))                     # the second job of a call is checked too
        assert call(pair, 2, None) == E_ARG, over
    a = _job(fvlib)
    assert call(C.byref(_job(fvlib, fine_u=a.coarse_u)), 1, None) == E_ARG          # onto itself
    assert call(C.byref(_job(fvlib, fine_p=a.fine_v)), 1, None) == E_ARG            # two fields of one job in one array
    for mine in ("fine_u", "fine_v", "fine_p", "fine_mdot"):
        for theirs in ("coarse_u", "coarse_v", "coarse_p", "fine_u", "fine_v", "fine_p", "fine_mdot"):
            pair = (J * 2)(a, _job(fvlib, 1, **{mine: getattr(a, theirs)}))
            assert call(pair, 2, None) == E_ARG, (mine, theirs)
            pair = (J * 2)(_job(fvlib, 1, **{mine: getattr(a, theirs)}), a)
            assert call(pair, 2, None) == E_ARG, (mine, theirs)
    import torch
    if not torch.cuda.is_available():                 # what passes validation: LDC_E_NODEVICE
        shared = (J * 2)(a, _job(fvlib, 1, coarse_u=a.coarse_u, coarse_v=a.coarse_v, coarse_p=a.coarse_p,
                                 fine_x_grid=a.fine_x_grid, fine_xc=a.fine_xc))        # one coarse trial, two fine ones
        assert call(shared, 2, None) == E_NODEVICE
        for ok in (dict(coarse_nx=8, coarse_ny=1024, fine_nx=1024, fine_ny=8), dict(Lx=2.0, Ly=0.5),
                   dict(coarse_nx=1024, coarse_ny=1024, fine_nx=1024, fine_ny=1024)):
            assert call(C.byref(_job(fvlib, **ok)), 1, None) == E_NODEVICE, ok
        # the one-CU entry still ends at 256 cells
        assert L.ldc_fv_prolong_tables_enqueue(C.byref(_job(fvlib)), 1, None) == E_ARG


# ---------------------------------------------------------------------- the restatement at the sizes only the chip reaches
def _axes(spec):
    nx, ny, beta = spec
    return axis_tables(tanh_vertices(nx, 1.0, beta))[0], axis_tables(tanh_vertices(ny, 1.0, beta))[0]


@pytest.mark.parametrize("coarse,fine", LARGE)
def test_every_node_and_weight_is_in_range(coarse, fine):
    for xc_c, xc_f in zip(_axes(coarse), _axes(fine)):
        k, t = T.locate(xc_c, 1.0, xc_f)
        e = T.nodes(xc_c, 1.0)
        assert np.all(np.diff(e) > 0) and e.size == xc_c.size + 2
        assert k.min() >= 0 and k.max() <= xc_c.size and np.all(np.diff(k) >= 0)
        assert np.all(t >= 0.0) and np.all(t <= 1.0) and np.all(e[k] <= xc_f) and np.all(xc_f <= e[k + 1])
        # bisection as the kernel does it finds the node np.searchsorted finds
        for x, want in zip(xc_f, k):
            lo, hi = 0, xc_c.size + 1
            while hi - lo > 1:
                mid = (lo + hi) >> 1
                lo, hi = (mid, hi) if e[mid] <= x else (lo, mid)
            assert lo == want
    assert max(fine[:2]) + min(fine[:2]) <= 2048          # the LDS table of `cells`: (k, t) of nx + ny centres


@pytest.mark.parametrize("coarse,fine", LARGE)
def test_a_bilinear_field_with_matching_ring_values_is_reproduced(coarse, fine):
    (cx, cy), (fx, fy) = _axes(coarse), _axes(fine)
    bil = lambda X, Y: 0.7 - 1.3 * X + 0.45 * Y + 2.1 * X * Y        # noqa: E731
    ring = bil(*np.meshgrid(T.nodes(cx, 1.0), T.nodes(cy, 1.0)))      # the field at every node of the extended axes
    kx, tx = T.locate(cx, 1.0, fx)
    ky, ty = T.locate(cy, 1.0, fy)
    got, want = T.interpolate(ring, kx, tx, ky, ty), bil(*np.meshgrid(fx, fy))
    err = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
    print(coarse, fine, "bilinear field: max relative error", err)
    assert err <= 1e-13                                               # the bound of profiles/fv_prolong_tables.md
