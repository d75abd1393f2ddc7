"""The wall-anchored finite-volume post-processing without a device (include/ldc_fv.h, ldc_fv_wall_post_enqueue): the
NumPy statement of tests/fv_wall_post_numpy.py against exact fields and the stored 128 x 128 solution, the refinement with
its floors and statuses on its own, and the plumbing (parameters, configuration, routes, the binding, argument checks)."""
import ctypes as C
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
import fv_wall_post_numpy as W  # noqa: E402

from conftest import PKG  # noqa: E402

BOTELLA_RE400 = dict(psi_min=-0.11396, x=0.5547, y=0.6055)      # data/validation/botella/botella_Re400_vortex.csv


# ------------------------------------------------------------------------------------------------ 1. tables
@pytest.mark.parametrize("n", [8, 13, 257])
def test_tables_diagonalise_the_wall_matrix(n):
    lam, Cm = W.tables(n)
    T = W.wall_matrix(n)
    e1 = float(np.max(np.abs(Cm.T @ T @ Cm - np.diag(lam))))
    e2 = float(np.max(np.abs(Cm.T @ Cm - np.eye(n))))
    print(f"n={n}: |C^T T C - Lam| {e1:.2e}, |C^T C - I| {e2:.2e}")
    assert e1 <= 1e-12 and e2 <= 1e-12
    assert np.all(np.diff(lam) > 0) and lam[-1] == pytest.approx(4.0, abs=1e-14)
    assert float(np.max(np.abs(Cm - Cm.T))) > 1e-3                    # not symmetric
    from solvers.fv.solver import wall_eig_host
    lam2, C2 = wall_eig_host(n)                                       # what the solver uploads is the statement's table
    assert np.array_equal(lam2, lam) and np.array_equal(C2, Cm)


# ------------------------------------------------------------------------------------------------ 2. manufactured field
def _wall_solution(nx, ny):
    """omega and psi of the manufactured field, psi with the tables the solver uploads (``solver.wall_eig_host``)."""
    from solvers.fv.solver import wall_eig_host
    u, v, ulid, exact = W.manufactured(nx, ny)
    dx, dy = 1.0 / nx, 1.0 / ny
    om = W.omega(u, v, ulid, dx, dy)
    return om, W.psi_solve(om, dx, dy, basis=wall_eig_host), exact, dx, dy


def test_manufactured_psi_is_second_order_and_beats_the_ring_rule():
    err = {}
    for n in (16, 32):
        om, psi, exact, dx, dy = _wall_solution(n, n)
        err[n] = float(np.max(np.abs(psi - exact)))
    om, psi, exact, dx, dy = _wall_solution(16, 16)
    ring = float(np.max(np.abs(W.psi_ring_rule(om, dx, dy) - exact)))
    print(f"max|psi - exact|: 16^2 {err[16]:.3e}, 32^2 {err[32]:.3e} (ratio {err[16] / err[32]:.2f}); ring rule at 16^2 "
          f"{ring:.3e} ({ring / err[16]:.1f} times the wall rule's)")
    assert err[32] <= err[16] / 3
    assert err[16] <= ring / 5


@pytest.mark.parametrize("shape", [(8, 8), (16, 16), (32, 32), (13, 17), (24, 16), (33, 20)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_manufactured_centre_refined_against_snapped(shape):
    nx, ny = shape
    om, psi, exact, dx, dy = _wall_solution(nx, ny)
    xs, ys = W.cell_centres(nx, ny)
    snapped = W.block_groups(W.result_block(psi, om, W.mask_bounds(xs, ys), dx, dy, refine=0))["min"]
    refined = W.block_groups(W.result_block(psi, om, W.mask_bounds(xs, ys), dx, dy, refine=1))["min"]
    assert snapped[W.G_STATUS] == -1 and refined[W.G_STATUS] == 0
    dist = lambda g: float(np.hypot(g[W.G_X] - W.EXACT_CENTRE[0], g[W.G_Y] - W.EXACT_CENTRE[1]))      # noqa: E731
    print(f"{nx}x{ny}: snapped {dist(snapped):.3e}, refined {dist(refined):.3e}, ratio 1/{dist(snapped) / dist(refined):.1f}")
    assert dist(refined) <= dist(snapped) / 4


# ------------------------------------------------------------------------------------------------ 3. the stored field
def test_stored_re400_field():
    g = np.load(PKG / "data" / "validation" / "fv" / "Re400" / "solution.npz")
    x, y = g["x"], g["y"]
    xs, ys = np.unique(x), np.unique(y)
    nx, ny = xs.size, ys.size
    order = np.lexsort((x, y))
    U, V = g["u"][order].reshape(ny, nx), g["v"][order].reshape(ny, nx)
    dx, dy = 1.0 / nx, 1.0 / ny
    from solvers.fv.solver import lid_profile, wall_eig_host
    om = W.omega(U, V, lid_profile(nx), dx, dy)                     # (the solver's lid profile and tables)
    psi = W.psi_solve(om, dx, dy, basis=wall_eig_host)
    m = W.metrics(W.result_block(psi, om, W.mask_bounds(xs, ys), dx, dy, refine=1), nx, dx, dy)
    ring = float(np.min(W.psi_ring_rule(om, dx, dy)))
    rel = lambda a: abs(a - BOTELLA_RE400["psi_min"]) / abs(BOTELLA_RE400["psi_min"])          # noqa: E731
    print(f"Re 400, {nx}x{ny}: wall + quadratic psi_min {m['psi_min']:.6f} ({100 * rel(m['psi_min']):.2f} %), centre "
          f"({m['psi_min_x']:.5f}, {m['psi_min_y']:.5f}); ring rule psi_min {ring:.6f} ({100 * rel(ring):.2f} %)")
    assert rel(m["psi_min"]) <= 0.01
    assert abs(m["psi_min_x"] - BOTELLA_RE400["x"]) <= 1e-3 and abs(m["psi_min_y"] - BOTELLA_RE400["y"]) <= 1e-3
    assert rel(ring) > 0.015
    assert m["psi_BR"] > 0 and m["omega_BR"] != 0.0 and m["psi_BL"] > 0 and m["omega_BL"] != 0.0


# ------------------------------------------------------------------------------------------------ 4. refine alone
def _codes():
    """The binding's names of the group slots and status codes: the statement uses the same numbers."""
    from solvers.fv import ldc_fv_lib as F
    assert (F.WALL_X, F.WALL_Y, F.WALL_PSI, F.WALL_OMEGA, F.WALL_STATUS, F.WALL_SX, F.WALL_SY) == \
        (W.G_X, W.G_Y, W.G_PSI, W.G_OMEGA, W.G_STATUS, W.G_SX, W.G_SY)
    return F


def _quadratic(nx, ny, i0, j0, a, b, h, c):
    I, J = np.meshgrid(np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64))
    return c + 0.5 * a * (I - i0) ** 2 + 0.5 * b * (J - j0) ** 2 + h * (I - i0) * (J - j0)


@pytest.mark.parametrize("case", [(5.3, 6.2, 2.0, 1.0, 0.5, -3.0, True), (4.6, 7.45, 1.0, 3.0, -0.7, -0.25, True),
                                  (6.0, 5.0, 1.5, 1.5, 0.0, -1.0, True), (5.3, 6.2, -2.0, -1.0, 0.5, 3.0, False),
                                  (7.5, 4.5, -1.0, -2.5, -0.9, 0.125, False)])
def test_refine_is_exact_on_definite_quadratics(case):
    i0, j0, a, b, h, c, want_min = case
    F = _codes()
    nx, ny, dx, dy = 13, 12, 0.1, 0.25
    psi = _quadratic(nx, ny, i0, j0, a, b, h, c)
    om = _quadratic(nx, ny, 3.0, 2.0, 0.3, -0.2, 0.1, 5.0)
    om_at = 5.0 + 0.15 * (i0 - 3.0) ** 2 - 0.1 * (j0 - 2.0) ** 2 + 0.1 * (i0 - 3.0) * (j0 - 2.0)
    for di, dj in ((0, 0), (1, 0), (0, 1)):                      # from every cell within one cell of the stationary point
        i, j = int(np.floor(i0)) + di, int(np.floor(j0)) + dj
        if abs(i - i0) > 1 or abs(j - j0) > 1:
            continue
        for dtype in (np.float64, W.LD):
            r = W.group(psi, om, j * nx + i, dx, dy, want_min, dtype=dtype)
            assert r[F.WALL_STATUS] == F.WALL_REFINED
            assert abs(r[W.G_X] - (i0 + 0.5) * dx) <= 1e-12 and abs(r[W.G_Y] - (j0 + 0.5) * dy) <= 1e-12
            assert abs(r[W.G_PSI] - c) <= 1e-12 and abs(r[W.G_OMEGA] - om_at) <= 1e-12
            assert abs(r[W.G_SX] - (i0 - i)) <= 1e-12 and abs(r[W.G_SY] - (j0 - j)) <= 1e-12 and r[7] == 0.0


def test_every_status_code():
    nx, ny, dx, dy = 12, 10, 1.0 / 12, 1.0 / 10
    xs, ys = W.cell_centres(nx, ny)
    bounds = W.mask_bounds(xs, ys)
    om = np.zeros((ny, nx))
    F = _codes()
    assert (F.WALL_NOT_ASKED, F.WALL_REFINED, F.WALL_NO_CANDIDATE, F.WALL_INDEFINITE, F.WALL_REJECTED) == (-1, 0, 1, 2, 3)
    status = lambda r: [int(g[F.WALL_STATUS]) for g in W.block_groups(r).values()]          # noqa: E731
    # all zero: the minimum is cell 0 and flat; no corner has a positive value
    r = W.result_block(np.zeros((ny, nx)), om, bounds, dx, dy)
    assert status(r) == [2, 1, 1, 1] and r[W.PSI_MIN_CELL] == 0
    assert status(W.result_block(np.zeros((ny, nx)), om, bounds, dx, dy, refine=0)) == [-1, -1, -1, -1]
    # a linear ramp at an interior cell: both second differences are below their floors
    I, J = np.meshgrid(np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64))
    ramp = 0.1 * I + 0.3 * J - 7.0
    g = W.group(ramp, om, 4 * nx + 5, dx, dy, True)
    assert g[W.G_STATUS] == 2 and g[W.G_X] == xs[5] and g[W.G_Y] == ys[4] and g[W.G_PSI] == ramp[4, 5] and g[W.G_SX] == 0
    # a saddle: det < 0
    assert W.group(_quadratic(nx, ny, 5.2, 4.1, 1.0, -1.0, 0.0, 0.0), om, 4 * nx + 5, dx, dy, True)[W.G_STATUS] == 2
    # a maximum where a minimum is asked for, and the other way round
    bowl = _quadratic(nx, ny, 5.2, 4.1, 1.0, 2.0, 0.1, -1.0)
    assert W.group(bowl, om, 4 * nx + 5, dx, dy, False)[W.G_STATUS] == 2
    assert W.group(-bowl, om, 4 * nx + 5, dx, dy, True)[W.G_STATUS] == 2
    # a long step: definite, the stationary point 2.4 cells away
    g = W.group(_quadratic(nx, ny, 7.4, 4.1, 1.0, 2.0, 0.1, -1.0), om, 4 * nx + 5, dx, dy, True)
    assert g[W.G_STATUS] == 3 and g[W.G_X] == xs[5] and g[W.G_SX] == 0 and g[W.G_SY] == 0
    # an extremum on the ring: the stencil needs the odd reflection (W = -C), the fit is definite and stays inside
    X, Y = np.meshgrid(xs, ys)
    wall = -(X / dx) * np.exp(-2 * X / dx) * np.exp(-((Y - 0.45) ** 2) / 0.05)
    r = W.result_block(wall, om + 1.5, bounds, dx, dy)
    g = W.block_groups(r)["min"]
    assert int(r[W.PSI_MIN_CELL]) % nx == 0 and g[W.G_STATUS] == 0 and 0 < g[W.G_SX] < 1 and 0 < g[W.G_X] < 2 * dx
    assert g[W.G_OMEGA] == 1.5 and g[W.G_PSI] < wall.min()          # on the ring omega is the cell's own
    assert W.reflected(wall, -1, 3) == -wall[3, 0] and W.reflected(wall, nx, ny) == wall[ny - 1, nx - 1]
    assert status(r)[1:] == [1, 1, 1]                                # psi <= 0 everywhere: no corner candidate
    # a corner vortex in BR only
    field = wall + 0.3 * np.exp(-((X - 0.8) ** 2 + (Y - 0.2) ** 2) / 0.01)
    assert status(W.result_block(field, om, bounds, dx, dy)) == [0, 0, 1, 1]
    # a NaN anywhere: the not-finite flag, no candidate at all
    bad = field.copy()
    bad[7, 7] = np.nan
    r = W.result_block(bad, om, bounds, dx, dy)
    assert r[W.NONFINITE] == 1 and status(r) == [1, 1, 1, 1]
    r = W.result_block(np.full((ny, nx), np.nan), om, bounds, dx, dy)
    assert r[W.NONFINITE] == 1 and r[W.PSI_MIN_CELL] == -1 and status(r) == [1, 1, 1, 1] and np.all(r[W.POST_LEN:][[0, 1, 2, 3]] == 0)


def test_status_fields_through_the_whole_statement():
    """The fields the GPU test drives through the chain, here through the statement (state -> omega -> psi with the solver's
    tables -> block): each reaches the status it was built for, the saddle by det < 0 and the ramp by the wrong sign."""
    from solvers.fv.solver import wall_eig_host
    F = _codes()
    nx, ny, dx, dy = 12, 10, 1.0 / 12, 1.0 / 10
    bounds = W.mask_bounds(*W.cell_centres(nx, ny))
    seen = set()
    for name, (target, want) in W.status_fields(nx, ny).items():
        om = W.omega(*W.state_for_psi(target, dx, dy), dx, dy)
        psi = W.psi_solve(om, dx, dy, basis=wall_eig_host)
        assert float(np.max(np.abs(psi - target))) <= 1e-12, name
        r = W.result_block(psi, om, bounds, dx, dy)
        got = [int(g[F.WALL_STATUS]) for g in W.block_groups(r).values()]
        assert all(w is None or g == w for g, w in zip(got, want)), (name, got, want)
        seen.update(got)
        if name in ("saddle", "ramp"):
            c = int(r[W.PSI_MIN_CELL])
            at = lambda a, b: W.reflected(psi, c % nx + a, c // nx + b)        # noqa: E731
            Hxx, Hyy = at(1, 0) - 2 * at(0, 0) + at(-1, 0), at(0, 1) - 2 * at(0, 0) + at(0, -1)
            Hxy = (at(1, 1) - at(-1, 1) - at(1, -1) + at(-1, -1)) / 4
            det = Hxx * Hyy - Hxy * Hxy
            assert (det < -1e-3 and Hxx > 0) if name == "saddle" else (det > 1 and Hxx < -1 and c == 0), (name, det, Hxx)
    assert {0, 1, 2, 3} <= seen


# ------------------------------------------------------------------------------------------------ 5. plumbing
def test_defaults_and_mlflow():
    from solvers.datastructures import FVFSGParameters, FVParameters
    p = FVParameters()
    assert p.streamfunction == "reference" and p.vortex_refine == "none"
    ml = p.to_mlflow()
    assert ml["streamfunction"] == "reference" and ml["vortex_refine"] == "none"
    ml = FVFSGParameters(streamfunction="wall", vortex_refine="quadratic").to_mlflow()
    assert ml["streamfunction"] == "wall" and ml["vortex_refine"] == "quadratic"


def test_unknown_values_raise_before_the_device():
    from solvers.fv.fsg import FVFSGSolver
    from solvers.fv.solver import FVSolver
    base = dict(name="fv", Re=100.0, nx=16, ny=16, device="cuda:7")
    for cls in (FVSolver, FVFSGSolver):
        with pytest.raises(ValueError, match="streamfunction"):
            cls(**base, streamfunction="face")
        with pytest.raises(ValueError, match="vortex_refine"):
            cls(**base, streamfunction="wall", vortex_refine="newton")
        with pytest.raises(ValueError, match=r"vortex_refine='quadratic'.*streamfunction='reference'"):
            cls(**base, vortex_refine="quadratic")


@pytest.mark.parametrize("solver", ["fv", "fv/fsg"])
def test_configuration_takes_the_two_options(solver):
    from dataclasses import fields
    from solvers.datastructures import FVFSGParameters, FVParameters
    from utilities.config import compose as Cc
    comp = Cc.Composer(PKG / "conf")
    cfg = Cc.resolve(Cc.compose_job(comp, [f"solver={solver}"], []))
    assert "streamfunction" not in cfg["solver"] and "vortex_refine" not in cfg["solver"]      # the YAML sets neither
    cfg = Cc.resolve(Cc.compose_job(comp, [f"solver={solver}", "+solver.streamfunction=wall",
                                           "+solver.vortex_refine=quadratic", "N=16", "Re=100"], []))
    kw = {k: v for k, v in cfg["solver"].items() if k != "_target_"}
    cls = FVFSGParameters if solver.endswith("fsg") else FVParameters
    assert set(kw) <= {f.name for f in fields(cls)}
    p = cls(**kw)
    assert p.streamfunction == "wall" and p.vortex_refine == "quadratic" and p.nx == 16
    for name in ("fv.yaml", "fv/fsg.yaml"):
        text = (PKG / "conf" / "solver" / name).read_text()
        assert "streamfunction" not in text and "vortex_refine" not in text


def test_post_route():
    from solvers.fv.solver import post_route
    assert post_route("host", True) == "cu" and post_route("device", True) == "cu"
    assert post_route("chip", True) == "chip" and post_route("device", False) == "chip"
    assert post_route("device", True, "reference") == "cu" and post_route("chip", False, "reference") == "chip"
    for vm in ("host", "device", "chip"):
        for has in (True, False):
            assert post_route(vm, has, "wall") == "wall"
            assert post_route(vm, has, streamfunction="wall") == "wall"


def test_level_and_seed_solvers_get_the_parameters():
    from solvers.datastructures import FVFSGParameters
    from solvers.fv import fsg
    assert "streamfunction" in fsg._LEVEL_FIELDS and "vortex_refine" in fsg._LEVEL_FIELDS
    p = FVFSGParameters(streamfunction="wall", vortex_refine="quadratic")
    kw = {k: getattr(p, k) for k in fsg._LEVEL_FIELDS}
    assert kw["streamfunction"] == "wall" and kw["vortex_refine"] == "quadratic"


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from solvers.fv import ldc_fv_lib
    return ldc_fv_lib


POINTERS = ("u", "v", "ulid", "Cx", "lamx", "Cy", "lamy", "psi", "omega", "scratch", "result")


def _job(F, **over):
    j = F.WallJob()
    for n in POINTERS:
        setattr(j, n, 8)                              # never dereferenced: validation comes first
    j.nx, j.ny, j.dx, j.dy = 32, 20, 1.0 / 32, 1.0 / 20
    j.ix_lt, j.ix_gt, j.jy_lt, j.jy_gt, j.refine = 16, 16, 10, 10, 1
    for k, v in over.items():
        setattr(j, k, v)
    return j


def test_header_binding_and_exports_agree(lib):
    hdr = (ROOT / "include" / "ldc_fv.h").read_text()
    declared = set(re.findall(r"\b(ldc_[a-z_0-9]+)\s*\(", hdr))
    for name in ("ldc_fv_wall_post_enqueue", "ldc_fv_wall_post_launches"):
        assert name in declared and name in lib.EXPORTS and hasattr(lib.lib(), name)
    assert set(lib.EXPORTS) <= declared
    define = lambda n: int(re.search(rf"#define {n} (-?\d+)", hdr).group(1))          # noqa: E731
    assert define("LDC_FV_WALL_LAUNCH_MAX") == lib.WALL_LAUNCH_MAX
    assert define("LDC_FV_WALL_RESULT_LEN") == lib.WALL_RESULT_LEN == lib.POST_RESULT_LEN + 4 * lib.WALL_GROUP_LEN
    assert define("LDC_FV_WALL_GROUP_LEN") == lib.WALL_GROUP_LEN == W.GROUP_LEN and lib.WALL_RESULT_LEN == W.RESULT_LEN
    for q, n in enumerate(("X", "Y", "PSI", "OMEGA", "STATUS", "SX", "SY")):
        assert define(f"LDC_FV_WALL_{n}") == getattr(lib, f"WALL_{n}") == q
    assert define("LDC_FV_VERSION") == 2 and lib.lib().ldc_fv_version() == 2 == lib.VERSION
    # the layout of the header: 11 pointers, 2 doubles, 8 int32
    assert C.sizeof(lib.WallJob) == 11 * 8 + 2 * 8 + 8 * 4 == 136 and lib.WALL_LAUNCH_MAX * 136 < 4096
    body = re.search(r"struct ldc_fv_wall_job \{(.*?)\};", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"\*?\s*([A-Za-z_]+)\s*(?:,|$)", decl.strip())]
    assert names == [n for n, _ in lib.WallJob._fields_]
    for nx, ny in ((8, 8), (260, 9), (1024, 1024)):
        assert lib.wall_scratch_len(nx, ny) == 2 * nx * ny + 12 * lib.wide_groups(nx, ny)
    assert re.search(r"#define LDC_FV_WALL_SCRATCH_LEN\(nx, ny\) \(2 \* \(int64_t\)\(nx\) \* \(ny\) \+ 12 \* LDC_FV_WIDE_GROUPS", hdr)


def test_launch_count(lib):
    L = lib.lib()
    m = lib.WALL_LAUNCH_MAX
    assert [L.ldc_fv_wall_post_launches(n) for n in (1, m, m + 1, 26, 256)] == [7, 7, 14, 14, 7 * ((256 + m - 1) // m)]
    assert L.ldc_fv_wall_post_launches(0) == -1 and L.ldc_fv_wall_post_launches(-4) == -1
    assert m <= 25                                    # 26 jobs are at least two launch groups


REFUSED = [{n: None} for n in POINTERS] + [
    dict(nx=7), dict(ny=7), dict(nx=1025), dict(ny=1025), dict(nx=0), dict(ny=-3), dict(dx=0.0), dict(dy=0.0),
    dict(dx=-0.1), dict(dy=float("nan")), dict(ix_lt=-1), dict(ix_lt=33), dict(ix_gt=-1), dict(ix_gt=33), dict(jy_lt=-1),
    dict(jy_lt=21), dict(jy_gt=-1), dict(jy_gt=21), dict(refine=2), dict(refine=-1)]


def test_refused_arguments_need_no_device(lib):
    L = lib.lib()
    assert L.ldc_fv_wall_post_enqueue(None, 1, None) == -1
    assert L.ldc_fv_wall_post_enqueue(C.byref(_job(lib)), 0, None) == -1
    assert L.ldc_fv_wall_post_enqueue(C.byref(_job(lib)), -2, None) == -1
    for over in REFUSED:
        assert L.ldc_fv_wall_post_enqueue(C.byref(_job(lib, **over)), 1, None) == -1, over
        pair = (lib.WallJob * 2)(_job(lib), _job(lib, **over))          # the second job of a call is checked too
        assert L.ldc_fv_wall_post_enqueue(pair, 2, None) == -1, over
    import torch
    if not torch.cuda.is_available():                 # the ends of the ranges pass validation: LDC_E_NODEVICE
        for ok in (dict(nx=8, ny=1024, ix_lt=0, ix_gt=8, jy_lt=1024, jy_gt=0), dict(refine=0), dict(nx=1024, ny=8, jy_lt=8, jy_gt=8)):
            assert L.ldc_fv_wall_post_enqueue(C.byref(_job(lib, **ok)), 1, None) == -3, ok
