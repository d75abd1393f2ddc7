"""The separable scaled preconditioner on the chip mapping (chip_preconditioner="separable"; ldc_fv_wide_set_preconditioner,
csrc/ldc_fv_wide_separable.inc), CPU side: the parameter surface with its refusals, the tables at the sizes only the chip
mapping reaches, the C ABI against the header with its validation on a host-side handle, and the one definition of the
scaling factor."""
import ctypes as C
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))

from conftest import PKG  # noqa: E402

E_ARG = -1
CHIP = dict(grid="tanh", mapping="chip", chip_grid="tables", pressure_equation="consistent")
SEP = dict(CHIP, chip_preconditioner="separable")


@pytest.fixture(scope="module")
def fvlib():
    import __graft_entry__ as g
    g.build()
    from solvers.fv import ldc_fv_lib
    return ldc_fv_lib


# ------------------------------------------------------------------------------------------- the parameter surface
def test_chip_preconditioner_defaults_and_goes_to_mlflow():
    from solvers.datastructures import FVFSGParameters, FVParameters
    from solvers.fv import solver as S
    assert FVParameters().chip_preconditioner == "laplacian" and FVFSGParameters().chip_preconditioner == "laplacian"
    assert S.CHIP_PRECONDITIONERS == ("laplacian", "separable") and S.PRESSURE_PRECONDITIONERS == ("laplacian", "separable")
    assert FVParameters().to_mlflow()["chip_preconditioner"] == "laplacian"
    ml = FVParameters(**SEP).to_mlflow()
    assert ml["chip_preconditioner"] == "separable" and ml["pressure_preconditioner"] == "laplacian" and "chip_grid" not in ml


def test_the_accepted_combination_reaches_the_device(monkeypatch):
    import torch
    from solvers.fv import solver as S
    from solvers.spectral import ldc_lib
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)        # every ValueError comes before the device
    for size in (dict(nx=16, ny=16), dict(nx=13, ny=17), dict(nx=1024, ny=8)):
        for pre in ("separable", "laplacian"):
            with pytest.raises(ldc_lib.LdcError, match="no CPU fallback"):
                S.FVSolver(name="fv", Re=100.0, **size, **dict(SEP, chip_preconditioner=pre))


def test_every_refusal_names_chip_preconditioner(monkeypatch):
    import torch
    from solvers.fv import solver as S
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    base = dict(name="fv", Re=100.0, nx=16, ny=16, chip_preconditioner="separable")
    for kw in (dict(),                                                                      # a plain one-CU trial
               dict(mapping="chip"), dict(mapping="chip", pressure_equation="consistent"),          # without chip_grid="tables"
               dict(grid="tanh"), dict(grid="tanh", pressure_equation="consistent_cu"),             # mapping "cu"
               dict(grid="tanh", pressure_equation="consistent_cu", pressure_preconditioner="separable"),
               dict(mapping="shared", pressure_equation="consistent"),
               dict(grid="tanh", mapping="chip", chip_grid="tables"),                               # the reference equation
               dict(grid="tanh", mapping="chip", chip_grid="tables", pressure_equation="reference")):
        with pytest.raises(ValueError, match="chip_preconditioner") as e:
            S.FVSolver(**dict(base, **kw))
        assert "chip_grid='tables'" in str(e.value) and "pressure_equation='consistent'" in str(e.value)   # what to give instead
    for bad in ("Separable", "jacobi", "", None):
        with pytest.raises(ValueError, match="chip_preconditioner=.*'laplacian' or 'separable'"):
            S.FVSolver(**dict(base, **dict(SEP, chip_preconditioner=bad)))
    # the one-CU key keeps its meaning and its refusal for such a trial, with either value of the new key
    for pre in ("laplacian", "separable"):
        with pytest.raises(ValueError, match="pressure_preconditioner"):
            S.FVSolver(**dict(base, **dict(SEP, chip_preconditioner=pre, pressure_preconditioner="separable")))
    with pytest.raises(ValueError, match="'laplacian' or 'separable'"):
        S.FVSolver(**dict(base, **dict(SEP, pressure_preconditioner="jacobi")))
    # what a chip-tables trial refuses, it refuses with the new key too
    for kw, word in ((dict(acceleration="anderson_chip"), "acceleration"), (dict(transfer="tables"), "transfer"),
                     (dict(mapping="shared"), "mapping='shared'"), (dict(vortex_metrics="chip"), "vortex_metrics")):
        with pytest.raises(ValueError, match=word):
            S.FVSolver(**dict(base, **dict(SEP, **kw)))


def test_the_launcher_composes_the_key():
    sys.path.insert(0, str(PKG))
    from utilities.config import compose as Cmp
    comp = Cmp.Composer(PKG / "conf")
    plain = Cmp.resolve(Cmp.compose_job(comp, ["solver=fv", "N=16"], []))
    got = Cmp.resolve(Cmp.compose_job(comp, ["solver=fv", "N=16", "+solver.mapping=chip", "+solver.grid=tanh",
                                             "+solver.chip_grid=tables", "+solver.pressure_equation=consistent",
                                             "+solver.chip_preconditioner=separable"], []))
    assert got["solver"] == dict(plain["solver"], mapping="chip", grid="tanh", chip_grid="tables",
                                 pressure_equation="consistent", chip_preconditioner="separable")
    assert "chip_preconditioner" not in plain["solver"]
    assert "chip_preconditioner" in (PKG / "conf" / "solver" / "fv.yaml").read_text()       # (the comment block names it)


# ------------------------------------------------------------------------------------------- the tables
TABLE_CASES = [(1024, 8, 1.0, 1.0, 1.5, 1.0), (8, 1024, 1.0, 1.0, 1.5, 1.0), (600, 600, 1.0, 1.0, 1.5, 1.0),
               (256, 256, 1.0, 1.0, 2.5, 1.0), (64, 48, 2.0, 2.0, 1.5, 2.0), (64, 48, 2.0, 1.0, 1.5, 1.0),
               (1024, 8, 2.0, 2.0, 1.5, 2.0)]


@pytest.mark.parametrize("nx,ny,Lx,Ly,beta,rho", TABLE_CASES, ids=lambda v: str(v))
def test_the_tables_of_the_chip_sizes(nx, ny, Lx, Ly, beta, rho):
    """The generalised eigenpairs of the fitted operator where lam[1] / lam[-1] falls below 1e-6 (5.1e-7 at 1024 cells, 1.0e-6
    at 600, 3.4e-7 at 256 with beta 2.5), and with L = 2, rho = 2 and unequal axes: lam ascending, one zero mode, first, lam[1]
    above rho (pi / L)^2 / 2 (it lies at 1.0 ... 2.3 times rho (pi / L)^2: 3.32 ... 22.1 in these cases), Q^T diag(h a) Q = I.
    The largest case, 1024 cells, gives max|Q^T M Q - I| = 2.4e-15 on the CPU (2.1e-15 ... 2.4e-15 over its three meshes; the
    smaller cases 4e-16 ... 3.4e-15); ten times that figure, 2.4e-14, is allowed."""
    from solvers.fv import solver as S
    tx, ty = S.separable_tables_host(nx, ny, Lx, Ly, beta, rho)
    for n, L, t in ((nx, Lx, tx), (ny, Ly, ty)):
        assert t.size == n * (n + 2)
        a, lam, Q = t[:n], t[n:2 * n], t[2 * n:].reshape(n, n)
        _, h, _, _ = S.axis_tables(S.tanh_vertices(n, L, beta))
        assert np.all(a > 0) and np.all(np.diff(lam) >= 0)
        assert abs(lam[0]) < 1e-9 * lam[-1]
        assert lam[1] > 0.5 * rho * (np.pi / L) ** 2
        err = float(np.max(np.abs(Q.T @ ((h * a)[:, None] * Q) - np.eye(n))))
        print(f"{nx} x {ny}, n {n}: lam[1] {lam[1]:.3f}, lam[1] / lam[-1] {lam[1] / lam[-1]:.1e}, orthogonality {err:.2e}")
        assert err <= 2.4e-14


# ------------------------------------------------------------------------------------------- C ABI
def test_wide_set_preconditioner_is_declared_exported_and_bound(fvlib):
    hdr = (ROOT / "include" / "ldc_fv.h").read_text()
    L = fvlib.lib()
    assert "ldc_fv_wide_set_preconditioner" in fvlib.EXPORTS
    assert re.search(r"int ldc_fv_wide_set_preconditioner\(ldc_fv_wide \*h, const struct ldc_fv_precond \*cfg\);", hdr)
    assert L.ldc_fv_wide_set_preconditioner.restype is C.c_int and callable(fvlib.wide_set_preconditioner)
    assert L.ldc_fv_wide_set_preconditioner.argtypes[1]._type_ is fvlib.Precond
    assert fvlib.PRECOND_MODES == dict(laplacian=0, separable=1) and C.sizeof(fvlib.Precond) == 40
    assert "csrc/ldc_fv_wide_separable.inc" in hdr.split(" *\n", 1)[0]         # the unit list at the head
    assert "The separable scaled preconditioner of a chip trial" in hdr


def test_the_scaling_factor_has_one_definition():
    """Both mappings include the same cells file, and neither unit has a copy of the expression."""
    csrc = PKG / "csrc"
    name = "double sg_sep_scale("
    assert (csrc / "ldc_fv_stretched_cells.inc").read_text().count(name) == 1
    for other in ("ldc_fv_stretched_sep.hip", "ldc_fv_stretched_phases.inc", "ldc_fv_wide_separable.inc",
                  "ldc_fv_wide_stretched.inc", "ldc_fv_wide.hip"):
        assert name not in (csrc / other).read_text(), other
    for unit in ("ldc_fv_stretched_sep.hip", "ldc_fv_wide_separable.inc"):          # (comments aside, neither takes a root)
        code = "\n".join(line.split("//", 1)[0] for line in (csrc / unit).read_text().splitlines())
        assert "sqrt" not in code, unit
    assert "sg_sep_scale(s, t.ax, t.ay, c, i, j)" in (csrc / "ldc_fv_stretched_sep.hip").read_text()
    assert "sg_sep_scale(sg, pb.px, pb.py, c, c % nx, c / nx)" in (csrc / "ldc_fv_wide_separable.inc").read_text()
    assert '#include "ldc_fv_stretched_cells.inc"' in (csrc / "ldc_fv_stretched_phases.inc").read_text()
    assert '#include "ldc_fv_stretched_phases.inc"' in (csrc / "ldc_fv_stretched_sep.hip").read_text()
    wide = (csrc / "ldc_fv_wide.hip").read_text()
    assert wide.index('#include "ldc_fv_stretched_cells.inc"') < wide.index('#include "ldc_fv_wide_stretched.inc"') \
        < wide.index('#include "ldc_fv_wide_separable.inc"')


class HostWide(C.Structure):
    """Room for the library's host-side ``struct ldc_fv_wide`` (csrc/ldc_fv_wide.hip), 512 bytes, all zero but the sizes: the
    mirror of tests/test_fv_wide_stretched_cpu.py with the pressure cap (the last word of the trial's arguments) named too."""
    _fields_ = ([(n, C.c_int) for n in ("nx", "ny", "scheme", "rec_cap", "warmup", "maxit")] + [("desc", C.c_char * 180)]
                + [("pmax", C.c_int), ("device", C.c_int), ("graph", C.c_byte), ("grid_mode", C.c_byte), ("mixing", C.c_short),
                   ("tail", C.c_char * 296)])


def _host(**kw):
    h = HostWide(**dict(dict(nx=13, ny=17, scheme=1, rec_cap=4, warmup=10, maxit=1000, device=63), **kw))
    return h, C.c_void_p(C.addressof(h))


NX, NY = 13, 17
GRID = dict(mode=1, pad=0, x_tables=8, y_tables=8, x_len=3 * NX + 2, y_len=3 * NY + 2)     # (fakes: never dereferenced)
GOOD = dict(mode=1, pad=0, x_table=16, y_table=24, x_len=NX * (NX + 2), y_len=NY * (NY + 2))


def test_wide_set_preconditioner_validation_on_a_host_side_handle(fvlib):
    L, G, P = fvlib.lib(), fvlib.Grid, fvlib.Precond
    call, set_grid = L.ldc_fv_wide_set_preconditioner, L.ldc_fv_wide_set_grid
    assert C.sizeof(HostWide) == 512 and (HostWide.pmax.offset, HostWide.grid_mode.offset, HostWide.tail.offset) == (204, 213, 216)
    assert call(None, C.byref(P(**GOOD))) == E_ARG and call(None, None) == E_ARG
    # a handle without geometry tables: refused, and a detach finds nothing to do -- on a mirror that ends at the head too
    h, hp = _host()
    plain = bytes(h)
    assert call(hp, C.byref(P(**GOOD))) == E_ARG and bytes(h) == plain
    assert call(hp, None) == 0 and call(hp, C.byref(P(mode=0))) == 0 and bytes(h) == plain
    short = (C.c_char * 216).from_buffer_copy(plain[:216])
    sp = C.c_void_p(C.addressof(short))
    assert call(sp, C.byref(P(**GOOD))) == E_ARG and call(sp, None) == 0 and set_grid(sp, None) == 0
    assert bytes(short) == plain[:216]
    # a refused call leaves every byte as it was, with and without a block attached, in both pressure modes
    for pmax in (0, 200):
        for start in (None, GOOD):
            h, hp = _host(pmax=pmax)
            assert set_grid(hp, C.byref(G(**GRID))) == 0
            if start:
                assert call(hp, C.byref(P(**start))) == 0
            before = bytes(h)
            for bad in (dict(mode=2), dict(mode=-1), dict(x_table=None), dict(y_table=None), dict(x_len=NX * (NX + 2) - 1),
                        dict(y_len=NY * (NY + 2) - 1), dict(x_len=0), dict(y_len=-1)):
                assert call(hp, C.byref(P(**dict(GOOD, **bad)))) == E_ARG, bad
                assert bytes(h) == before, bad


@pytest.mark.parametrize("pmax", [0, 200], ids=["reference", "consistent"])
def test_the_block_goes_on_and_comes_off_behind_the_grid(fvlib, pmax):
    """Attaching changes no byte of the first 304 (the head and everything up to `grid`) nor the grid block (304 .. 319);
    detaching by NULL and by mode 0 restores the bytes; ldc_fv_wide_set_grid resets the block when it attaches again and when
    it detaches; ldc_fv_wide_launches returns the same numbers throughout; no device is asked."""
    L, G, P = fvlib.lib(), fvlib.Grid, fvlib.Precond
    call, set_grid = L.ldc_fv_wide_set_preconditioner, L.ldc_fv_wide_set_grid
    h, hp = _host(pmax=pmax)
    plain = bytes(h)
    launches = lambda: [L.ldc_fv_wide_launches(hp, b) for b in (1, 12, 4000)]       # noqa: E731
    want = launches()
    # (the mirror's pressure budget is 0: init and pfinish come, the exact solve's four GEMMs go)
    assert want == ([16, 71, 5011] if pmax == 0 else [14, 69, 5009])
    assert set_grid(hp, C.byref(G(**GRID))) == 0
    tables = bytes(h)
    assert launches() == want
    assert call(hp, C.byref(P(**GOOD))) == 0
    attached = bytes(h)
    assert attached[:320] == tables[:320] and attached[320:] != tables[320:]
    assert attached[320:344] == bytes((C.c_int64 * 3)(16, 24, 1)) and not any(attached[344:])     # px, py, the mode
    assert launches() == want
    assert call(hp, C.byref(P(**GOOD))) == 0 and bytes(h) == attached
    assert call(hp, None) == 0 and bytes(h) == tables
    assert call(hp, C.byref(P(**GOOD))) == 0 and call(hp, C.byref(P(mode=0))) == 0 and bytes(h) == tables
    # a laplacian request needs no tables
    assert call(hp, C.byref(P(mode=0, x_table=None, y_table=None, x_len=0, y_len=0))) == 0 and bytes(h) == tables
    # the geometry tables attached again, and taken off: the block is reset either way
    assert call(hp, C.byref(P(**GOOD))) == 0 and set_grid(hp, C.byref(G(**GRID))) == 0 and bytes(h) == tables
    assert call(hp, C.byref(P(**GOOD))) == 0 and set_grid(hp, None) == 0 and bytes(h) == plain
    assert call(hp, C.byref(P(**GOOD))) == E_ARG and bytes(h) == plain and launches() == want


def test_a_handle_with_the_block_is_still_refused_where_tables_are(fvlib):
    L, G, P = fvlib.lib(), fvlib.Grid, fvlib.Precond
    h, hp = _host(pmax=200)
    other, op = _host()
    assert L.ldc_fv_wide_set_grid(hp, C.byref(G(**GRID))) == 0 and L.ldc_fv_wide_set_preconditioner(hp, C.byref(P(**GOOD))) == 0
    before = bytes(h)
    fake = 8
    post = fvlib.Post(Sx=fake, lamx=fake, Sy=fake, lamy=fake, ix_lt=0, ix_gt=0, jy_lt=0, jy_gt=0, psi=fake, omega=fake,
                      result=fake)
    hs = (C.c_void_p * 2)(hp, op)
    b = C.c_void_p()
    acc = fvlib.Anderson(depth=2, start=1, hist=fake, hist_len=fvlib.anderson_hist_len(NX, NY, 2), astate=fake)
    assert L.ldc_fv_wide_batch_create(hs, 2, fake, fvlib.wide_batch_table_len([(NX, NY)] * 2), C.byref(b)) == E_ARG and not b.value
    assert L.ldc_fv_wide_post_enqueue(hp, C.byref(post), None, 0, None) == E_ARG
    assert L.ldc_fv_wide_prolong_enqueue(hp, op, None) == E_ARG and L.ldc_fv_wide_prolong_enqueue(op, hp, None) == E_ARG
    assert L.ldc_fv_wide_set_anderson(hp, C.byref(acc), fake, fvlib.wide_anderson_scratch_len(NX, NY, 2)) == E_ARG
    assert bytes(h) == before
