"""The separable scaled preconditioner of the stretched-grid pressure CG (pressure_preconditioner="separable",
ldc_fv_set_preconditioner, csrc/ldc_fv_stretched_sep.hip), CPU side: the tables and the operator of the NumPy restatement
(tests/fv_separable_numpy.py) against dense matrices, positive definiteness on the range of A, the CG loop against dense
solves, its iteration counts beside the constant-coefficient preconditioner's, the solver's host builder, the parameter
surface, the launcher's key and the C ABI without a device."""
import ctypes as C
import re
import sys
from pathlib import Path

import numpy as np
import pytest

from conftest import PKG  # noqa: E402
from fv_separable_numpy import FVSeparableState, axis_table, separable_eig, separable_fit
from fv_stretched_numpy import FVStretchedState

ROOT = Path(__file__).resolve().parent.parent
E_ARG, E_STATE = -1, -2
MESHES = [(8, 8, 1.0, {}), (13, 17, 1.5, dict(Lx=2.0, Ly=0.5)), (16, 16, 0.0, {})]
KW = dict(linear_solver_tol=1e-9, convection_scheme="TVD")


def _state(nx, ny, beta, geo, cls=FVSeparableState, **kw):
    return cls(nx, ny, 100.0, grid_stretch=beta, **dict(KW, **geo, **kw))


# ---------------------------------------------------------------------- the tables
@pytest.mark.parametrize("nx,ny,beta,geo", MESHES)
def test_tables_are_generalised_eigenpairs_and_invert_the_separable_operator(nx, ny, beta, geo):
    o = _state(nx, ny, beta, geo)
    assert np.all(o.sa > 0) and np.all(o.sb > 0) and o.G.shape == (ny, nx)
    # the fit is the least-squares one of log G by a sum: the residual has zero row and column means
    res = np.log(o.G) - np.log(o.sb[:, None] * o.sa[None, :])
    assert np.max(np.abs(res.mean(axis=0))) <= 1e-13 and np.max(np.abs(res.mean(axis=1))) <= 1e-13
    for lam, Q, K, M in ((o.slamx, o.sQx, o.sKx, o.sMx), (o.slamy, o.sQy, o.sKy, o.sMy)):
        n = lam.size
        assert np.max(np.abs(Q.T @ (M[:, None] * Q) - np.eye(n))) <= 1e-11
        assert np.max(np.abs(K @ Q - (M[:, None] * Q) * lam[None, :])) <= 1e-11 * np.max(np.abs(K))
        assert abs(lam[0]) <= 1e-11 * lam[-1] and lam[1] > 1e-6 * lam[-1] and np.all(np.diff(lam) >= 0)
        assert np.allclose(K, K.T, rtol=0, atol=0) and np.max(np.abs(K.sum(axis=1))) <= 1e-12 * np.max(np.abs(K))
    Ls = o.separable_dense()
    rng = np.random.default_rng(7)
    for _ in range(3):
        r = rng.standard_normal((ny, nx))
        r -= r.mean()
        back = (Ls @ o.separable_pinv(r).ravel()).reshape(ny, nx)
        assert np.linalg.norm(back - r) <= 1e-10 * np.linalg.norm(r)
    tx, ty = o.tables()
    assert tx.size == nx * (nx + 2) and ty.size == ny * (ny + 2)
    assert np.array_equal(tx[:nx], o.sa) and np.array_equal(tx[nx: 2 * nx], o.slamx)
    assert np.array_equal(tx[2 * nx:].reshape(nx, nx)[:, 3], o.sQx[:, 3])          # row-major, column k the k-th vector


@pytest.mark.parametrize("nx,ny,beta,geo", MESHES)
def test_the_preconditioner_is_positive_on_the_range_of_a(nx, ny, beta, geo):
    """D from a state after 5 iterations; the dense M^-1 = S L_s+ S restricted to the vectors of zero sum (an orthonormal basis
    Z of them: Z^T M^-1 Z) has only positive eigenvalues."""
    o = _state(nx, ny, beta, geo)
    o.run(5)
    n = nx * ny
    s = o.scale.ravel()
    assert s.shape == (n,) and np.all(s > 0)
    Lp = np.stack([o.separable_pinv(e.reshape(ny, nx)).ravel() for e in np.eye(n)], axis=1)
    assert np.max(np.abs(Lp - Lp.T)) <= 1e-12 * np.max(np.abs(Lp))
    Minv = s[:, None] * Lp * s[None, :]
    Zf, _ = np.linalg.qr(np.concatenate([np.ones((n, 1)), np.eye(n)[:, 1:]], axis=1))
    Z = Zf[:, 1:]                                            # orthogonal to the constants
    assert np.max(np.abs(Z.sum(axis=0))) <= 1e-12
    ev = np.linalg.eigvalsh(Z.T @ (0.5 * (Minv + Minv.T)) @ Z)
    print(f"{nx}x{ny} beta {beta}: eigenvalues of Z^T M^-1 Z in [{ev[0]:.3e}, {ev[-1]:.3e}]")
    assert ev[0] > 0.0 and ev[0] > 1e-12 * ev[-1]
    # and it is what precondition() applies
    r = np.random.default_rng(3).standard_normal((ny, nx))
    assert np.allclose(o.precondition(r).ravel(), Minv @ r.ravel(), rtol=0, atol=1e-12 * np.max(np.abs(Minv)) * n)


# ---------------------------------------------------------------------- the loop
@pytest.mark.parametrize("nx,ny,beta,geo", MESHES)
def test_cg_meets_the_residual_and_follows_the_direct_solve(nx, ny, beta, geo):
    """As tests/test_fv_pressure_cpu.py judges the existing loop: CG at 1e-13 and the dense solve of the pinned system give the
    same 20 iterations to 1e-12, and |div mdot| <= 2 pressure_tol |b| after each; besides, the iterate of every solve meets
    |A x - b| <= tol |b| against the dense A (plus the rounding of the product)."""
    tol = 1e-13
    cg = _state(nx, ny, beta, geo, pressure_solver="cg", pressure_tol=tol)
    direct = _state(nx, ny, beta, geo, cls=FVStretchedState, pressure_solver="direct", pressure_equation="consistent")
    eps = np.finfo(float).eps
    for k in range(20):
        row = cg.step()
        direct.step()
        A = cg.dense(cg.last["wx"], cg.last["wy"])
        b, x = cg.last["b"].ravel(), cg.last["x"].ravel()
        res = np.linalg.norm(A @ x - b)
        slack = 64 * eps * np.linalg.norm(np.abs(A) @ np.abs(x))
        du, dv, dp = (np.max(np.abs(getattr(cg, f) - getattr(direct, f))) for f in "uvp")
        print(f"{nx}x{ny} iteration {k}: CG {cg.cg_iters[-1]}, |Ax-b| {res:.1e} (tol |b| {tol * cg.last['bnorm']:.1e}), "
              f"|du| {du:.1e} |dp| {dp:.1e}, |div| {row[3]:.1e}")
        assert res <= tol * cg.last["bnorm"] + slack
        assert du <= 1e-12 and dv <= 1e-12 and dp <= 1e-12
        assert row[3] <= 2 * tol * cg.last["bnorm"]
    assert max(cg.cg_iters) <= 40 and cg.cg_caps == 0 and len(cg.cg_iters) == 20


# (nx, ny, Re, beta, SIMPLE iterations, other settings): TVD with 0.7 / 0.3 unless it says otherwise; from rest,
# pressure_tol 1e-8, linear_solver_tol 1e-9
COUNT_ROWS = [(16, 16, 100.0, 1.5, 30, {}),
              (13, 17, 100.0, 1.5, 30, dict(Lx=2.0, Ly=0.5)),
              (8, 8, 100.0, 1.0, 20, {}),
              (24, 40, 400.0, 2.0, 30, dict(alpha_uv=0.4, alpha_p=0.2)),
              (32, 32, 1000.0, 1.5, 40, dict(convection_scheme="Upwind", alpha_uv=0.4, alpha_p=0.2))]


@pytest.mark.parametrize("nx,ny,Re,beta,K,kw", COUNT_ROWS)
def test_cg_counts_beside_the_constant_coefficient_preconditioner(nx, ny, Re, beta, K, kw):
    """Measured (mean / max CG iterations per solve, laplacian then separable): 40.4 / 44 and 11.9 / 12; 36.7 / 38 and 8.9 / 9;
    17.3 / 18 and 9.5 / 10; 132.4 / 136 and 15.0 / 16; 61.3 / 63 and 15.1 / 16.  Asked: no caps, the separable max at most the
    laplacian max, and at beta >= 1.5 the separable mean at most half the laplacian mean (the largest ratio measured is 0.39);
    below that only at most the laplacian mean."""
    args = dict(dict(convection_scheme="TVD", alpha_uv=0.7, alpha_p=0.3), **kw)
    runs = {}
    for name, cls in (("laplacian", FVStretchedState), ("separable", FVSeparableState)):
        o = cls(nx, ny, Re, grid_stretch=beta, linear_solver_tol=1e-9, pressure_equation="consistent", pressure_solver="cg",
                pressure_tol=1e-8, pressure_max_iters=300, **args)
        o.run(K)
        assert o.cg_caps == 0 and len(o.cg_iters) == K
        runs[name] = o
    lap, sep = runs["laplacian"].cg_iters, runs["separable"].cg_iters
    diff = max(np.max(np.abs(getattr(runs["laplacian"], f) - getattr(runs["separable"], f))) for f in "uvp")
    print(f"{nx}x{ny} Re {Re} beta {beta}: laplacian {np.mean(lap):.1f} / {max(lap)}, separable {np.mean(sep):.1f} / {max(sep)}, "
          f"max field difference {diff:.1e}")
    assert max(sep) <= max(lap)
    assert np.mean(sep) <= (0.5 if beta >= 1.5 else 1.0) * np.mean(lap)


# ---------------------------------------------------------------------- the solver's host builder
def test_the_solvers_tables_are_the_restatements():
    sys.path.insert(0, str(PKG / "src"))
    from solvers.fv import solver as S
    for nx, ny, beta, geo in MESHES:
        o = _state(nx, ny, beta, geo)
        a, b = S.separable_fit(o.hx, o.dxf, o.hy, o.dyf)
        a2, b2, _ = separable_fit(o.hx, o.dxf, o.hy, o.dyf)
        assert np.array_equal(a, a2) and np.array_equal(b, b2)
        lam, Q = S.separable_axis_host(o.hx, o.dxf, o.gxf, a)
        lam2, Q2, _, _ = separable_eig(o.hx, o.dxf, o.gxf, a2)
        assert np.array_equal(lam, lam2) and np.array_equal(Q, Q2)
        tx, ty = S.separable_tables_host(nx, ny, geo.get("Lx", 1.0), geo.get("Ly", 1.0), beta)
        wx, wy = o.tables()
        assert np.array_equal(tx, wx) and np.array_equal(ty, wy)
        assert np.array_equal(tx, axis_table(o.sa, o.slamx, o.sQx))
    assert S.PRESSURE_PRECONDITIONERS == ("laplacian", "separable")


# ---------------------------------------------------------------------- the parameter surface
def test_parameter_surface_and_rejections(monkeypatch):
    from solvers.datastructures import FVParameters
    from solvers.fv import solver as S
    from solvers.spectral import ldc_lib
    assert FVParameters().pressure_preconditioner == "laplacian"
    assert FVParameters().to_mlflow()["pressure_preconditioner"] == "laplacian"
    assert FVParameters(pressure_preconditioner="separable").to_mlflow()["pressure_preconditioner"] == "separable"
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)        # every ValueError comes before the device
    base = dict(name="fv", Re=100.0, nx=16, ny=16)
    good = dict(grid="tanh", pressure_equation="consistent_cu", pressure_preconditioner="separable")
    for ok in (dict(), dict(grid_stretch=0.0), dict(nx=13, ny=17, Lx=2.0, Ly=0.5), dict(grid_stretch=2.0, Re=1000.0)):
        with pytest.raises(ldc_lib.LdcError, match="no CPU fallback"):
            S.FVSolver(**dict(base, **good, **ok))
    for ok in (dict(), dict(grid="tanh"), dict(grid="tanh", pressure_equation="consistent_cu")):      # the default anywhere
        with pytest.raises(ldc_lib.LdcError, match="no CPU fallback"):
            S.FVSolver(**dict(base, pressure_preconditioner="laplacian", **ok))
    with pytest.raises(ValueError, match="pressure_preconditioner='jacobi': 'laplacian' or 'separable'"):
        S.FVSolver(**dict(base, **dict(good, pressure_preconditioner="jacobi")))
    rejected = [dict(), dict(pressure_equation="consistent_cu"), dict(grid="tanh"),
                dict(grid="tanh", pressure_equation="reference"), dict(mapping="chip", pressure_equation="consistent"),
                dict(mapping="shared", pressure_equation="consistent")]
    for kw in rejected:
        with pytest.raises(ValueError, match="pressure_preconditioner='separable' with"):
            S.FVSolver(**dict(base, pressure_preconditioner="separable", **kw))
    # what grid="tanh" refuses stays refused, by the grid's own message
    for kw, word in ((dict(acceleration="anderson"), "acceleration"), (dict(vortex_metrics="device"), "vortex_metrics"),
                     (dict(streamfunction="wall"), "streamfunction")):
        with pytest.raises(ValueError, match=f"grid='tanh' with {word}"):
            S.FVSolver(**dict(base, **good, **kw))


def test_the_launcher_composes_the_key():
    sys.path.insert(0, str(PKG))
    from utilities.config import compose as Cmp
    comp = Cmp.Composer(PKG / "conf")
    plain = Cmp.resolve(Cmp.compose_job(comp, ["solver=fv", "N=16"], []))
    got = Cmp.resolve(Cmp.compose_job(comp, ["solver=fv", "N=16", "+solver.grid=tanh", "+solver.pressure_equation=consistent_cu",
                                             "+solver.pressure_preconditioner=separable"], []))
    assert got["solver"] == dict(plain["solver"], grid="tanh", pressure_equation="consistent_cu",
                                 pressure_preconditioner="separable")
    assert "pressure_preconditioner" not in plain["solver"]     # without the key: the composed config of before


# ---------------------------------------------------------------------- the C ABI without a device
@pytest.fixture(scope="module")
def fvlib():
    import __graft_entry__ as g
    g.build()
    from solvers.fv import ldc_fv_lib
    return ldc_fv_lib


class HostFv(C.Structure):
    """The library's host-side ``struct ldc_fv`` (csrc/ldc_fv_common.inc), the preconditioner mode at its end."""
    _fields_ = [("dev", C.c_void_p), ("ctrl", C.c_void_p), ("rec_cap", C.c_int), ("device", C.c_int), ("nx", C.c_int),
                ("ny", C.c_int), ("dx", C.c_double), ("dy", C.c_double), ("pressure_mode", C.c_int), ("grid_mode", C.c_int),
                ("precond_mode", C.c_int)]


def test_set_preconditioner_is_declared_exported_and_bound(fvlib):
    hdr = (ROOT / "include" / "ldc_fv.h").read_text()
    L = fvlib.lib()
    assert "ldc_fv_set_preconditioner" in fvlib.EXPORTS and re.search(r"int ldc_fv_set_preconditioner\(", hdr)
    assert L.ldc_fv_set_preconditioner.restype is C.c_int and callable(fvlib.set_preconditioner)
    val = lambda name: int(re.search(rf"#define {name} \(?(-?\d+)", hdr).group(1))        # noqa: E731
    assert (val("LDC_FV_PRECOND_LAPLACIAN"), val("LDC_FV_PRECOND_SEPARABLE")) == (0, 1)
    assert fvlib.PRECOND_MODES == dict(laplacian=0, separable=1)
    assert val("LDC_FV_VERSION") == fvlib.VERSION == L.ldc_fv_version() == 2 and val("LDC_FV_NWORK") == 32
    assert "#define LDC_FV_PRECOND_TABLE_LEN(n) ((int64_t)(n) * ((int64_t)(n) + 2))" in hdr
    assert fvlib.precond_table_len(13) == 13 * 15 and fvlib.precond_table_len(256) == 256 * 258
    assert "csrc/ldc_fv_stretched_sep.hip" in hdr.split(" *\n", 1)[0]          # the unit list at the head
    assert "The separable scaled preconditioner" in hdr and "ldc_fv_stretched_sep_launch" not in hdr
    import __graft_entry__ as g
    assert g.SRC_FV_STRETCHED_SEP.name == "ldc_fv_stretched_sep.hip" and g.SRC_FV_STRETCHED_SEP.exists()
    # struct sizes: the new one, and the others as pinned
    assert C.sizeof(fvlib.Precond) == 40 and C.sizeof(fvlib.Grid) == 40 and C.sizeof(fvlib.Pressure) == 16
    assert C.sizeof(fvlib.Problem) == 24 + 72 + 96
    m = re.search(r"struct ldc_fv_precond \{(.*?)\};", hdr, re.S)
    names = re.findall(r"\b(mode|pad|x_table|y_table|x_len|y_len)\b\s*[;,]", m.group(1))
    assert names == ["mode", "pad", "x_table", "y_table", "x_len", "y_len"] == [f for f, _ in fvlib.Precond._fields_]
    # the blocks of the descriptor slot: the new one behind the grid block, clear of the pressure block; FvDesc as it was
    inc = (PKG / "csrc" / "ldc_fv_common.inc").read_text()
    assert "constexpr int kFvPrecondOffset = 344;" in inc and "constexpr int kFvGridOffset = 328;" in inc
    assert "constexpr int kFvCuPcgOffset = 384;" in inc and "static_assert(kFvPrecondOffset >=" in inc
    # the shared phases moved into an include of both units
    for unit in ("ldc_fv_stretched.hip", "ldc_fv_stretched_sep.hip"):
        assert '#include "ldc_fv_stretched_phases.inc"' in (PKG / "csrc" / unit).read_text()
    # the CG loop, the four-GEMM solve and the kernel frame: one include of the three units with a pressure CG of their own
    for unit in ("ldc_fv_cu_pressure.hip", "ldc_fv_stretched.hip", "ldc_fv_stretched_sep.hip"):
        assert '#include "ldc_fv_cu_solve.inc"' in (PKG / "csrc" / unit).read_text()


def test_set_preconditioner_validation_needs_no_device(fvlib):
    L = fvlib.lib()
    P = fvlib.Precond
    fake = 8                                                     # never dereferenced by a refused call
    call = L.ldc_fv_set_preconditioner
    assert HostFv.grid_mode.offset == 52 and HostFv.precond_mode.offset == 56      # the new field: at the end
    good = dict(mode=1, pad=0, x_table=fake, y_table=fake, x_len=13 * 15, y_len=17 * 19)
    assert call(None, C.byref(P(**good))) == E_STATE
    for start in (0, 1):                                         # a refused call leaves the modes alone
        h = HostFv(dev=None, ctrl=None, rec_cap=4, device=63, nx=13, ny=17, dx=1 / 13, dy=1 / 17, pressure_mode=1,
                   grid_mode=1, precond_mode=start)
        hp = C.c_void_p(C.addressof(h))
        for bad in (dict(mode=2), dict(mode=-1), dict(x_table=None), dict(y_table=None), dict(x_len=13 * 15 - 1),
                    dict(y_len=17 * 19 - 1), dict(x_len=0), dict(x_len=3 * 13 + 2)):
            assert call(hp, C.byref(P(**dict(good, **bad)))) == E_ARG, bad
            assert (h.precond_mode, h.grid_mode, h.pressure_mode) == (start, 1, 1), bad
    # a handle without geometry tables is refused, whatever else is right
    h = HostFv(device=63, nx=13, ny=17, rec_cap=4, pressure_mode=1, grid_mode=0, precond_mode=0)
    hp = C.c_void_p(C.addressof(h))
    assert call(hp, C.byref(P(**good))) == E_ARG and (h.precond_mode, h.grid_mode) == (0, 0)
    # back to the constant-coefficient preconditioner: by mode and by NULL, neither touches the device nor the other modes
    h = HostFv(device=63, nx=13, ny=17, rec_cap=4, pressure_mode=1, grid_mode=1, precond_mode=1)
    hp = C.c_void_p(C.addressof(h))
    assert call(hp, C.byref(P(mode=0))) == 0 and (h.precond_mode, h.grid_mode, h.pressure_mode) == (0, 1, 1)
    h.precond_mode = 1
    assert call(hp, None) == 0 and (h.precond_mode, h.grid_mode, h.pressure_mode) == (0, 1, 1)
    # ... and on a uniform handle too
    h.grid_mode, h.precond_mode = 0, 1
    assert call(hp, None) == 0 and h.precond_mode == 0

