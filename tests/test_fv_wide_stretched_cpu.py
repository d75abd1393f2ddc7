"""Wall-clustered grids on the chip mapping (grid="tanh", mapping="chip", chip_grid="tables"; ldc_fv_wide_set_grid,
csrc/ldc_fv_wide_stretched.inc), CPU side: the parameter surface with its refusals, the C ABI against the header, and the
argument validation of ldc_fv_wide_set_grid and of the calls that refuse a handle with tables, on a host-side handle."""
import ctypes as C
import re
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))

from conftest import PKG  # noqa: E402

E_ARG, E_STATE = -1, -2
CHIP = dict(grid="tanh", mapping="chip", chip_grid="tables")


@pytest.fixture(scope="module")
def fvlib():
    import __graft_entry__ as g
    g.build()
    from solvers.fv import ldc_fv_lib
    return ldc_fv_lib


# ------------------------------------------------------------------------------------------- the parameter surface
def test_chip_grid_defaults_and_stays_out_of_mlflow():
    from solvers.datastructures import FVFSGParameters, FVParameters
    from solvers.fv import solver as S
    assert FVParameters().chip_grid == "uniform" and FVFSGParameters().chip_grid == "uniform"
    assert S.CHIP_GRIDS == ("uniform", "tables") and S.GRIDS == ("uniform", "tanh")
    ml = FVParameters(**CHIP).to_mlflow()
    assert "chip_grid" not in ml and "mapping" not in ml and ml["grid"] == "tanh"


def test_accepted_combinations_reach_the_device(monkeypatch):
    import torch
    from solvers.fv import solver as S
    from solvers.spectral import ldc_lib
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)        # every ValueError comes before the device
    base = dict(name="fv", Re=100.0, nx=16, ny=16, **CHIP)
    for mode in ("reference", "consistent"):
        for post in (dict(), dict(streamfunction="reference", vortex_metrics="host"), dict(streamfunction="wall_stretched"),
                     dict(streamfunction="wall_stretched", vortex_refine="quadratic")):
            for size in (dict(nx=8, ny=8), dict(nx=13, ny=17), dict(nx=1024, ny=8), dict(grid_stretch=0.0)):
                kw = dict(base, pressure_equation=mode, **post, **size)
                with pytest.raises(ldc_lib.LdcError, match="no CPU fallback"):
                    S.FVSolver(**kw)


def test_every_refusal_names_its_option(monkeypatch):
    import torch
    from solvers.fv import solver as S
    from solvers.fv.fsg import FVFSGSolver
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    base = dict(name="fv", Re=100.0, nx=16, ny=16)
    # chip_grid itself: a value, and the two options it is accepted with
    for kw in (dict(chip_grid="tanh"), dict(chip_grid="tables"), dict(chip_grid="tables", mapping="chip"),
               dict(chip_grid="tables", grid="tanh"), dict(chip_grid="tables", grid="tanh", mapping="cu"),
               dict(chip_grid="tables", grid="tanh", mapping="shared")):
        with pytest.raises(ValueError, match="chip_grid"):
            S.FVSolver(**dict(base, **kw))
    with pytest.raises(ValueError, match="mapping='shared'"):
        S.FVSolver(**dict(base, **dict(CHIP, mapping="shared")))
    # without the option everything is as it was
    with pytest.raises(ValueError, match="grid='tanh' with mapping='chip': stretched grids run on the one-CU kernel only"):
        S.FVSolver(**dict(base, grid="tanh", mapping="chip"))
    with pytest.raises(ValueError, match="grid='tanh' with mapping='chip'"):
        S.FVSolver(**dict(base, grid="tanh", mapping="chip", chip_grid="uniform"))
    # what such a trial still refuses
    for kw, word in ((dict(acceleration="anderson_chip"), "acceleration"), (dict(acceleration="anderson"), "acceleration"),
                     (dict(pressure_equation="consistent_cu"), "consistent_cu"),
                     (dict(pressure_preconditioner="separable"), "pressure_preconditioner"),
                     (dict(pressure_equation="consistent", pressure_preconditioner="separable"), "pressure_preconditioner"),
                     (dict(transfer="tables"), "transfer"),
                     (dict(vortex_metrics="device"), "vortex_metrics"), (dict(vortex_metrics="chip"), "vortex_metrics"),
                     (dict(nx=300, vortex_metrics="chip"), "vortex_metrics"),
                     (dict(streamfunction="wall"), "streamfunction"),
                     (dict(vortex_refine="quadratic"), "vortex_refine"),
                     (dict(nx=1025), "1024"), (dict(ny=7), "8")):
        with pytest.raises(ValueError, match=word):
            S.FVSolver(**dict(base, **CHIP, **kw))
    with pytest.raises(ValueError, match="solver=fv/fsg"):
        FVFSGSolver(**dict(base, **CHIP))
    # start_from and prolong: the check reads no handle and no device
    ns = lambda **kw: type("T", (), dict(dict(stretched=True, chip=True, chip_tables=True, transfer_tables=False,       # noqa: E731
                                              device=torch.device("cpu")), **kw))()
    with pytest.raises(ValueError, match="start_from with grid='tanh'"):
        S.prolong([(ns(), ns())])
    with pytest.raises(ValueError, match="start_from with grid='tanh'"):
        S.prolong([(ns(stretched=False, chip_tables=False), ns())])
    with pytest.raises(ValueError, match="streamfunction='reference'"):
        S.postprocess([ns(stretched_wall=False)])


def test_the_eigenpairs_of_the_chip_sizes():
    """The generalised eigenpairs of a tanh axis at the sizes only the chip mapping reaches: one zero mode, first; the first mode
    above it near rho (pi / L)^2 whatever n is (lam[1] / lam[-1] falls below 1e-6 there); Q^T H Q = I."""
    import numpy as np
    from solvers.fv import solver as S
    for n, beta, L, rho in ((512, 1.5, 1.0, 1.0), (1024, 1.5, 2.0, 1.0), (1024, 0.0, 1.0, 2.0)):
        _, h, d, _ = S.axis_tables(S.tanh_vertices(n, L, beta))
        lam, Q = S.generalised_eig_host(h, d, rho)
        assert abs(lam[0]) < 1e-9 * lam[-1] and np.all(np.diff(lam) >= 0)       # (the two wall layers' modes come in near pairs)
        assert lam[1] == pytest.approx(rho * (np.pi / L) ** 2, rel=1e-4) and lam[1] < 1e-5 * lam[-1]
        assert np.max(np.abs(Q.T @ (h[:, None] * Q) - np.eye(n))) < 1e-12
        assert np.max(np.abs(Q[:, 0] - Q[0, 0])) < 1e-9 * abs(Q[0, 0])              # the zero mode is a constant


def test_the_launcher_composes_the_keys():
    sys.path.insert(0, str(PKG))
    import main as M
    from utilities.config import compose as Cmp
    comp = Cmp.Composer(PKG / "conf")
    plain = Cmp.resolve(Cmp.compose_job(comp, ["solver=fv", "N=16"], []))
    got = Cmp.resolve(Cmp.compose_job(comp, ["solver=fv", "N=16", "+solver.mapping=chip", "+solver.grid=tanh",
                                             "+solver.chip_grid=tables"], []))
    assert got["solver"] == dict(plain["solver"], mapping="chip", grid="tanh", chip_grid="tables")
    assert "chip_grid" not in plain["solver"]                   # conf/solver/fv.yaml itself is unchanged
    assert M.batch_key(got) == (M.FV, "chip")                   # a chip trial runs on its own


# ------------------------------------------------------------------------------------------- C ABI
def test_wide_set_grid_is_declared_exported_and_bound(fvlib):
    hdr = (ROOT / "include" / "ldc_fv.h").read_text()
    L = fvlib.lib()
    assert "ldc_fv_wide_set_grid" in fvlib.EXPORTS
    assert re.search(r"int ldc_fv_wide_set_grid\(ldc_fv_wide \*h, const struct ldc_fv_grid \*grid\);", hdr)
    assert L.ldc_fv_wide_set_grid.restype is C.c_int and callable(fvlib.wide_set_grid)
    assert L.ldc_fv_wide_set_grid.argtypes[1]._type_ is fvlib.Grid
    val = lambda name: int(re.search(rf"#define {name} \(?(-?\d+)", hdr).group(1))        # noqa: E731
    assert val("LDC_FV_VERSION") == fvlib.VERSION == 2
    assert fvlib.GRID_MODES == dict(uniform=0, tanh=1) and C.sizeof(fvlib.Grid) == 40
    assert "csrc/ldc_fv_wide_stretched.inc" in hdr.split(" *\n", 1)[0]         # the unit list at the head
    assert "Stretched grids of a chip trial" in hdr
    # the arithmetic has one definition: both mappings include the same cells file, and the wide unit has no copy
    csrc = PKG / "csrc"
    cells = (csrc / "ldc_fv_stretched_cells.inc").read_text()
    for name in ("struct SgCtx", "void sg_grad(", "void sg_cell_assemble(", "void sg_cell_faces(", "double sg_wx(", "double sg_wy(",
                 "double sg_row(", "void sg_gauss(", "void sg_cell_correct(", "void sg_cell_fluxvort(", "void sg_cell_sums("):
        assert name in cells, name
        for other in ("ldc_fv_stretched_phases.inc", "ldc_fv_wide_stretched.inc", "ldc_fv_wide.hip"):
            assert name not in (csrc / other).read_text(), (name, other)
    assert '#include "ldc_fv_stretched_cells.inc"' in (csrc / "ldc_fv_stretched_phases.inc").read_text()
    assert '#include "ldc_fv_stretched_cells.inc"' in (csrc / "ldc_fv_wide.hip").read_text()


class HostWide(C.Structure):
    """Room for the library's host-side ``struct ldc_fv_wide`` (csrc/ldc_fv_wide.hip), all zero but the sizes: an empty list
    of graphs, no mixing, the reference pressure equation, the uniform grid.  Only the head is named: the trial's descriptor
    (validation reads nx, ny and max_lin_iters) and, at the end of the first 216 bytes, the graph switch, the grid mode (in
    what was the high byte of the graph switch: the other tests' mirrors, which end before the tables, stay good) and the
    mixing flag."""
    _fields_ = ([(n, C.c_int) for n in ("nx", "ny", "scheme", "rec_cap", "warmup", "maxit")] + [("desc", C.c_char * 184)]
                + [("device", C.c_int), ("graph", C.c_byte), ("grid_mode", C.c_byte), ("mixing", C.c_short),
                   ("tail", C.c_char * 296)])


def _host(**kw):
    h = HostWide(**dict(dict(nx=13, ny=17, scheme=1, rec_cap=4, warmup=10, maxit=1000, device=63), **kw))
    return h, C.c_void_p(C.addressof(h))


def test_wide_set_grid_validation_on_a_host_side_handle(fvlib):
    L, G = fvlib.lib(), fvlib.Grid
    call = L.ldc_fv_wide_set_grid
    assert (HostWide.grid_mode.offset, HostWide.mixing.offset, HostWide.tail.offset) == (213, 214, 216)
    fake = 8                                                     # never dereferenced: the pointers travel by value
    good = dict(mode=1, pad=0, x_tables=fake, y_tables=fake, x_len=3 * 13 + 2, y_len=3 * 17 + 2)
    assert call(None, C.byref(G(**good))) == E_ARG and call(None, None) == E_ARG
    for start in (None, good):                                   # a refused call leaves the handle as it was
        h, hp = _host()
        if start:
            assert call(hp, C.byref(G(**start))) == 0
        before = bytes(h)
        for bad in (dict(mode=2), dict(mode=-1), dict(x_tables=None), dict(y_tables=None), dict(x_len=3 * 13 + 1),
                    dict(y_len=3 * 17 + 1), dict(x_len=0), dict(y_len=-1)):
            assert call(hp, C.byref(G(**dict(good, **bad)))) == E_ARG, bad
            assert bytes(h) == before, bad
    # tables go on and come off, by mode and by NULL: of the head (all that ldc_fv_wide_launches reads) only the grid mode
    # moves, the two pointers stand at the end of the handle, and no device is asked
    h, hp = _host()
    plain = bytes(h)
    launches = [L.ldc_fv_wide_launches(hp, b) for b in (1, 12, 4000)]
    assert launches == [16, 71, 5011]
    assert call(hp, C.byref(G(**good))) == 0
    attached = bytes(h)
    assert h.grid_mode == 1 and (h.graph, h.mixing) == (0, 0)
    assert attached[:213] == plain[:213] and attached[214:296] == plain[214:296] and attached[296:] != plain[296:]
    assert [L.ldc_fv_wide_launches(hp, b) for b in (1, 12, 4000)] == launches          # launch for launch the uniform chain
    assert call(hp, C.byref(G(**good))) == 0 and bytes(h) == attached
    assert call(hp, C.byref(G(mode=0))) == 0 and bytes(h) == plain
    assert call(hp, C.byref(G(**good))) == 0 and call(hp, None) == 0 and bytes(h) == plain
    # a uniform request needs no tables
    assert call(hp, C.byref(G(mode=0, x_tables=None, y_tables=None, x_len=0, y_len=0))) == 0 and bytes(h) == plain
    # ... and a handle without tables is not read behind its head: a mirror that ends there will do
    short = (C.c_char * 216).from_buffer_copy(plain[:216])
    assert call(C.c_void_p(C.addressof(short)), None) == 0 and bytes(short) == plain[:216]
    assert L.ldc_fv_wide_set_graph(hp, 1) == 0 and (h.graph, h.grid_mode) == (1, 0)
    assert call(hp, C.byref(G(**good))) == 0 and L.ldc_fv_wide_set_graph(hp, 0) == 0 and (h.graph, h.grid_mode) == (0, 1)


def _mixing(fvlib, nx, ny, depth=2):
    fake = 8
    acc = fvlib.Anderson(depth=depth, start=1, hist=fake, hist_len=fvlib.anderson_hist_len(nx, ny, depth), astate=fake)
    return acc, fake, fvlib.wide_anderson_scratch_len(nx, ny, depth)


def test_mixing_and_tables_refuse_each_other_in_either_order(fvlib):
    L, G = fvlib.lib(), fvlib.Grid
    good = G(mode=1, pad=0, x_tables=8, y_tables=8, x_len=3 * 13 + 2, y_len=3 * 17 + 2)
    acc, scratch, scratch_len = _mixing(fvlib, 13, 17)
    # mixing first
    h, hp = _host()
    assert L.ldc_fv_wide_set_anderson(hp, C.byref(acc), scratch, scratch_len) == 0 and h.mixing == 1
    before = bytes(h)
    assert L.ldc_fv_wide_set_grid(hp, C.byref(good)) == E_ARG and bytes(h) == before
    assert L.ldc_fv_wide_set_grid(hp, None) == 0 and bytes(h) == before                # (uniform: nothing to refuse)
    # tables first
    h, hp = _host()
    assert L.ldc_fv_wide_set_grid(hp, C.byref(good)) == 0
    before = bytes(h)
    assert L.ldc_fv_wide_set_anderson(hp, C.byref(acc), scratch, scratch_len) == E_ARG and bytes(h) == before
    assert L.ldc_fv_wide_set_anderson(hp, None, None, 0) == 0 and bytes(h) == before   # (detaching what is not there)
    assert L.ldc_fv_wide_set_grid(hp, None) == 0
    assert L.ldc_fv_wide_set_anderson(hp, C.byref(acc), scratch, scratch_len) == 0 and h.mixing == 1


def test_a_handle_with_tables_is_refused_where_equal_spacing_is_assumed(fvlib):
    """ldc_fv_wide_batch_create, ldc_fv_wide_post_enqueue and ldc_fv_wide_prolong_enqueue return LDC_E_ARG for a handle with
    tables before they ask for a device, whichever place of the list or of the pair it stands in."""
    L, G = fvlib.lib(), fvlib.Grid
    good = G(mode=1, pad=0, x_tables=8, y_tables=8, x_len=3 * 13 + 2, y_len=3 * 17 + 2)
    h, hp = _host()
    other, op = _host()
    fake = 8
    post = fvlib.Post(Sx=fake, lamx=fake, Sy=fake, lamy=fake, ix_lt=0, ix_gt=0, jy_lt=0, jy_gt=0, psi=fake, omega=fake,
                      result=fake)
    hs = (C.c_void_p * 2)(hp, op)
    table_len = fvlib.wide_batch_table_len([(13, 17), (13, 17)])
    b = C.c_void_p()

    def calls():
        return (L.ldc_fv_wide_batch_create(hs, 2, fake, table_len, C.byref(b)),
                L.ldc_fv_wide_batch_create(hs, 1, fake, table_len, C.byref(b)),
                L.ldc_fv_wide_post_enqueue(hp, C.byref(post), None, 0, None),
                L.ldc_fv_wide_prolong_enqueue(hp, op, None), L.ldc_fv_wide_prolong_enqueue(op, hp, None))

    # (no call here may pass validation: the pointers are fakes, and with a device the next step would use them)
    assert L.ldc_fv_wide_set_grid(hp, C.byref(good)) == 0
    assert calls() == (E_ARG,) * 5 and not b.value
    # the table entry is full: the tables cannot ride in a batch, so a second trial with tables is refused as the first
    assert L.ldc_fv_wide_set_grid(op, C.byref(good)) == 0 and L.ldc_fv_wide_set_grid(hp, None) == 0
    assert L.ldc_fv_wide_batch_create(hs, 2, fake, table_len, C.byref(b)) == E_ARG and not b.value
