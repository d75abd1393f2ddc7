"""The wall-anchored finite-volume post-processing on stretched grids without a device (include/ldc_fv.h,
ldc_fv_wall_stretched_post_enqueue): the NumPy statement of tests/fv_wall_stretched_numpy.py against a long-double direct
solve of the same operator, against the uniform statement at beta = 0 and against smooth and exactly quadratic fields; the
refinement's statuses; and the plumbing (parameters, routes, the binding, argument checks)."""
import ctypes as C
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
import fv_wall_post_numpy as W  # noqa: E402
import fv_wall_stretched_numpy as S  # noqa: E402
from fv_wall_stretched_numpy import EPS, LD  # noqa: E402

SHAPES = [(8, 8), (13, 17), (37, 50)]


# ------------------------------------------------------------------------------------------------ 1. tables
@pytest.mark.parametrize("beta", S.BETAS)
@pytest.mark.parametrize("n", [8, 13, 50])
def test_tables_are_dirichlet_generalised_eigenpairs(n, beta):
    ax = S.axis(n, 1.0, beta)
    lam, Q = S.dirichlet_eig(ax)
    K, H = S.dirichlet_stiffness(ax[2]), np.diag(ax[1])
    scale = float(np.max(np.abs(K)))
    # no zero mode; ascending (the modes at the two clustered walls pair up to rounding: any basis of a pair serves the solve)
    assert np.all(lam > 0) and np.all(np.diff(lam) >= 0)
    assert float(np.max(np.abs(Q.T @ H @ Q - np.eye(n)))) <= 1e-12
    assert float(np.max(np.abs(Q.T @ K @ Q - np.diag(lam)))) <= 1e-12 * scale * float(np.max(ax[1])) * n
    assert K[0, 0] == 1 / ax[2][0] + 1 / ax[2][1] and ax[2][0] == 0.5 * ax[1][0]      # the wall face carries 1 / (h / 2)
    from solvers.fv.solver import axis_tables, dirichlet_eig_host, tanh_vertices
    xc, h, d, g = axis_tables(tanh_vertices(n, 1.0, beta))                     # what the solver uploads is the statement's table
    lam2, Q2 = dirichlet_eig_host(h, d)
    assert all(np.array_equal(a, b) for a, b in zip((xc, h, d, g), ax))
    assert np.array_equal(lam2, lam) and np.array_equal(Q2, Q)
    lam3, Q3 = S.dirichlet_eig(ax, tridiagonal=True)                          # the O(n^2) route of the GPU tests' long axes
    assert float(np.max(np.abs(lam3 - lam))) <= 1e-12 * lam[-1] and float(np.max(np.abs(Q3.T @ H @ Q3 - np.eye(n)))) <= 1e-12
    assert float(np.max(np.abs(Q3.T @ K @ Q3 - np.diag(lam3)))) <= 1e-12 * scale * float(np.max(ax[1])) * n
    if beta == 0:                                                             # equal widths: h T_n / h^2 of the uniform rule
        assert float(np.max(np.abs(K * ax[1][0] - W.wall_matrix(n)))) <= 1e-12
        assert float(np.max(np.abs(lam * ax[1][0] ** 2 - W.tables(n)[0]))) <= 1e-12 * 4


# ------------------------------------------------------------------------------------------------ 2. psi
@pytest.mark.parametrize("beta", S.BETAS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_psi_against_a_long_double_solve_of_the_same_operator(shape, beta):
    """|psi - long double| <= 4 eps kappa max|psi|, kappa the condition number of the stretched generalised problem.
    Measured share of eps kappa max|psi| (bound 4): 1.3 (8 x 8, beta 0), 0.7 (13 x 17, beta 2.5), at most 0.3 elsewhere."""
    nx, ny = shape
    ax, ay = S.axis(nx, 1.0, beta), S.axis(ny, 1.0, beta)
    u, v, ulid, _ = S.manufactured(ax, ay)
    om = S.omega(u, v, ulid, ax, ay)
    psi_ld = S.psi_solve_ld(om, ax, ay)
    residual = float(np.max(np.abs(S.apply_operator(psi_ld, ax, ay, LD) - S.volume_rhs(om, ax, ay).astype(LD))))
    # the yardstick is a direct solve: its residual is a banded factorisation's backward error, 16 b eps_LD max|A| max|psi|
    amax = float(np.max(ay[1]) * np.max(np.diag(S.dirichlet_stiffness(ax[2]))) + np.max(np.diag(S.dirichlet_stiffness(ay[2]))) * np.max(ax[1]))
    assert residual <= 16 * min(nx, ny) * float(np.finfo(LD).eps) * amax * float(np.max(np.abs(psi_ld)))
    err = float(np.max(np.abs(S.psi_solve(om, ax, ay).astype(LD) - psi_ld)))
    k, top = S.kappa(ax, ay), float(np.max(np.abs(psi_ld)))
    print(f"FVWS {nx}x{ny} beta {beta}: psi err {err:.2e}, kappa {k:.2e}, share of eps kappa max|psi| {err / (EPS * k * top):.3f} "
          f"(bound 4); long-double residual {residual:.1e}")
    assert err <= S.psi_bound(psi_ld, ax, ay)


@pytest.mark.parametrize("shape", SHAPES + [(12, 10)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_beta_zero_is_the_uniform_statement(shape):
    """omega (constant lid), psi, the slots, the groups and the statuses equal tests/fv_wall_post_numpy.py to rounding."""
    nx, ny = shape
    dx, dy = 1.0 / nx, 1.0 / ny
    ax, ay = S.axis(nx, 1.0, 0.0), S.axis(ny, 1.0, 0.0)
    u, v, _ = W.smooth_state(nx, ny)
    ulid = np.full(nx, 1.0)
    om_u, om_s = W.omega(u, v, ulid, dx, dy), S.omega(u, v, ulid, ax, ay)
    assert float(np.max(np.abs(om_u - om_s))) <= W.omega_bound(u, v, ulid, dx, dy) + S.omega_bound(u, v, ulid, ax, ay)
    psi_u, psi_s = W.psi_solve(om_u, dx, dy), S.psi_solve(om_s, ax, ay)
    assert float(np.max(np.abs(psi_u - psi_s))) <= 2 * W.psi_bound(psi_u, nx, ny, dx, dy)
    assert S.kappa(ax, ay) == pytest.approx(W.kappa(nx, ny, dx, dy), rel=1e-10)
    fields = [(psi_u, om_u)]
    if shape == (12, 10):                             # every status code of the uniform statement
        fields += [(f, om_u) for f, _ in W.status_fields(nx, ny).values()]
    seen = set()
    for psi, om in fields:
        for refine in (0, 1):
            b_u = W.result_block(psi, om, S.mask_bounds(ax, ay), dx, dy, refine=refine)
            b_s = S.result_block(psi, om, S.mask_bounds(ax, ay), ax, ay, refine=refine)
            assert np.array_equal(b_u[:S.POST_LEN], b_s[:S.POST_LEN])
            assert S.statuses(b_u) == S.statuses(b_s)
            seen.update(S.statuses(b_s))
            # (omega* sums terms of the size of the second differences of omega: rounding in units of its stencil's spread)
            scale = np.maximum(1.0, np.abs(b_u))
            scale[S.POST_LEN + S.G_OMEGA:: S.GROUP_LEN] = max(1.0, float(np.max(np.abs(om))))
            assert np.all(np.abs(b_u - b_s) <= 1e-12 * scale), (b_u - b_s)
    if shape == (12, 10):
        assert {-1, 0, 1, 2, 3} <= seen


@pytest.mark.parametrize("beta", [1.5, 2.5])
def test_psi_is_second_order_on_a_smooth_field(beta):
    """max|psi - exact| falls by at least 3 per doubling, 16^2 -> 32^2 -> 64^2.  Measured ratios: 3.87, 3.98 at beta 1.5;
    3.64, 3.92 at beta 2.5 (3.99, 4.00 at beta 0)."""
    err = []
    for n in (16, 32, 64):
        ax = S.axis(n, 1.0, beta)
        exact, om = S.smooth_field(ax, ax)
        err.append(float(np.max(np.abs(S.psi_solve(om, ax, ax) - exact))))
    print(f"beta {beta}: max|psi - exact| {err[0]:.3e}, {err[1]:.3e}, {err[2]:.3e}; ratios {err[0] / err[1]:.2f}, {err[1] / err[2]:.2f}")
    assert err[0] / err[1] >= 3 and err[1] / err[2] >= 3


def test_omega_is_the_solvers_gauss_rule():
    """``FVSolver._vorticity`` of a stretched trial, on a bare namespace with the host branch's attributes."""
    from types import SimpleNamespace
    from solvers.fv.solver import FVSolver
    nx, ny = 13, 17
    ax, ay = S.axis(nx, 1.0, 1.5), S.axis(ny, 1.0, 1.5)
    u, v, ulid, _ = S.manufactured(ax, ay)
    ns = SimpleNamespace(stretched=True, shape_full=(ny, nx), _gxf=ax[3], _gyf=ay[3], _hx=ax[1], _hy=ay[1], _ulid_host=ulid,
                         fields=SimpleNamespace(u=u.ravel(), v=v.ravel()))
    ns._gauss_gradient = lambda f, lid: FVSolver._gauss_gradient(ns, f, lid)
    assert np.array_equal(FVSolver._vorticity(ns), S.omega(u, v, ulid, ax, ay))


# ------------------------------------------------------------------------------------------------ 3. refinement
@pytest.mark.parametrize("centre", [(0.53, 0.57), (0.031, 0.4), (0.9, 0.97)])
def test_the_fit_is_exact_for_a_six_term_quadratic(centre):
    """On a beta = 1.5 mesh the fit returns the stationary point and value of a sampled quadratic to rounding, in the interior
    and from a cell whose stencil has unequal sides."""
    ax, ay = S.axis(24, 1.0, 1.5), S.axis(20, 1.0, 1.5)
    x0, y0 = centre
    psi = S.quadratic_field(ax, ay, x0, y0)
    om = S.quadratic_field(ax, ay, x0 + 0.01, y0 - 0.02, a=-3.0, b=2.0, c=0.7, level=5.0)
    i, j = int(np.argmin(np.abs(ax[0] - x0))), int(np.argmin(np.abs(ay[0] - y0)))
    assert 0 < i < 23 and 0 < j < 19                  # (the reflected stencil of a ring cell does not sample the quadratic)
    g = S.group(psi, om, j * 24 + i, ax, ay, True)
    want_om = 5.0 - 3.0 * 0.01**2 + 2.0 * 0.02**2 - 0.7 * 0.01 * 0.02
    print(centre, g)
    assert g[S.G_STATUS] == 0
    assert abs(g[S.G_X] - x0) <= 1e-13 and abs(g[S.G_Y] - y0) <= 1e-13 and abs(g[S.G_PSI] + 1.0) <= 1e-13
    assert abs(g[S.G_OMEGA] - want_om) <= 1e-12
    dw, de = S.stencil_distances(ax[2], i)
    sx = x0 - ax[0][i]
    assert g[S.G_SX] == pytest.approx(sx / dw if sx < 0 else sx / de, abs=1e-11)


def test_the_refined_centre_beats_the_cell_centre():
    """64^2, beta 1.5, the smooth field: the fitted minimum is at least 100 times nearer the true one than the cell centre."""
    from scipy.optimize import minimize
    ax = S.axis(64, 1.0, 1.5)
    exact, om = S.smooth_field(ax, ax)
    f = lambda p: -np.sin(np.pi * p[0]) * np.sin(np.pi * p[1]) * np.exp(-((p[0] - 0.53) ** 2 + (p[1] - 0.57) ** 2))  # noqa: E731
    true = minimize(f, (0.5, 0.5), tol=1e-14, method="Nelder-Mead", options=dict(xatol=1e-12, fatol=1e-16)).x
    r = S.result_block(exact, om, S.mask_bounds(ax, ax), ax, ax)
    g, cell = S.block_groups(r)["min"], int(r[W.PSI_MIN_CELL])
    snapped = np.hypot(ax[0][cell % 64] - true[0], ax[0][cell // 64] - true[1])
    refined = np.hypot(g[S.G_X] - true[0], g[S.G_Y] - true[1])
    print(f"snapped {snapped:.2e}, refined {refined:.2e}")
    assert g[S.G_STATUS] == 0 and refined <= snapped / 100


@pytest.mark.parametrize("beta", [1.5, 2.5])
def test_constructed_fields_reach_every_status(beta):
    ax, ay = S.axis(12, 1.0, beta), S.axis(10, 1.0, beta)
    seen = set()
    for name, (psi, want) in S.status_fields(ax, ay).items():
        om = np.zeros_like(psi)
        for refine in (1, 0):
            r = S.result_block(psi, om, S.mask_bounds(ax, ay), ax, ay, refine=refine)
            got = S.statuses(r)
            if refine == 0:
                assert got == (-1, -1, -1, -1)
                continue
            print(beta, name, got)
            assert all(w is None or g == w for g, w in zip(got, want)), (name, got, want)
            seen.update(got)
            for g in S.block_groups(r).values():      # every status other than 0 reports the cell's own values
                if g[S.G_STATUS] != 0:
                    assert g[S.G_SX] == 0 and g[S.G_SY] == 0
        if name == "short_side":                      # within the long side's distance, beyond the short side's
            c = int(r[W.PSI_MIN_CELL])
            i, j = c % 12, c // 12
            assert (i, j) == (3, 4)
            dw, de = S.stencil_distances(ax[2], i)
            ds, dn = S.stencil_distances(ay[2], j)
            at = lambda a, b: S.reflected(psi, i + a, j + b)        # noqa: E731
            gx, gy, Hxx, Hyy, Hxy = S.fit(at(0, 0), at(-1, 0), at(1, 0), at(0, -1), at(0, 1), at(-1, -1), at(1, -1), at(-1, 1),
                                          at(1, 1), dw, de, ds, dn)
            det = Hxx * Hyy - Hxy * Hxy
            sx, sy = -(Hyy * gx - Hxy * gy) / det, -(Hxx * gy - Hxy * gx) / det
            assert det > 0 and Hxx > 0 and -de < sx < -dw and -ds < sy < dn, (sx, dw, de, sy, ds, dn)
            assert ax[0][i] + sx > 0
    assert {0, 1, 2, 3} <= seen
    # a result that is not finite: status 3
    psi = S.quadratic_field(ax, ay, ax[0][5] + 0.01, ay[0][4] - 0.01)
    om = np.zeros_like(psi)
    om[4, 6] = 1e308
    om[4, 4] = -1e308
    with np.errstate(all="ignore"):
        g = S.group(psi, om, 4 * 12 + 5, ax, ay, True)
    assert g[S.G_STATUS] == 3 and g[S.G_X] == ax[0][5] and g[S.G_PSI] == psi[4, 5] and g[S.G_SX] == 0


# ------------------------------------------------------------------------------------------------ 4. plumbing
def test_post_route_keeps_its_values_and_knows_the_new_route():
    from solvers.fv.solver import post_route
    for vm in ("host", "device", "chip"):
        for has in (True, False):
            assert post_route(vm, has, "wall") == "wall" and post_route(vm, has, "wall_stretched") == "wall_stretched"
            assert post_route(vm, has, streamfunction="wall_stretched") == "wall_stretched"
            assert post_route(vm, has, "reference") == post_route(vm, has) in ("cu", "chip")


def test_refusals_that_stay_and_the_new_value_is_accepted(monkeypatch):
    from solvers.fv import solver as Sv
    from solvers.fv.fsg import FVFSGSolver
    from solvers.spectral import ldc_lib
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)        # every ValueError comes before the device
    base = dict(name="fv", Re=100.0, nx=16, ny=16, grid="tanh")
    for ok in (dict(streamfunction="wall_stretched"), dict(streamfunction="wall_stretched", vortex_refine="quadratic"),
               dict(streamfunction="wall_stretched", vortex_refine="none", vortex_metrics="device"),       # (not consulted with the wall rule)
               dict(streamfunction="wall_stretched", vortex_refine="quadratic", pressure_equation="consistent_cu",
                    pressure_preconditioner="separable", nx=13, ny=17)):
        with pytest.raises(ldc_lib.LdcError, match="no CPU fallback"):      # past every check, up to the device
            Sv.FVSolver(**dict(base, **ok))
    wall = dict(streamfunction="wall_stretched", vortex_refine="quadratic")
    rejected = [(dict(mapping="chip"), "grid='tanh' with mapping"), (dict(mapping="shared"), "grid='tanh' with mapping"),
                (dict(acceleration="anderson"), "grid='tanh' with acceleration"),
                (dict(mapping="chip", acceleration="anderson_chip"), "grid='tanh' with (mapping|acceleration)")]
    for kw, msg in rejected:
        for extra in (dict(), wall):
            with pytest.raises(ValueError, match=msg):
                Sv.FVSolver(**dict(base, **kw, **extra))
    for vm in ("device",):
        with pytest.raises(ValueError, match="grid='tanh' with vortex_metrics"):
            Sv.FVSolver(**dict(base, vortex_metrics=vm, streamfunction="reference"))
    with pytest.raises(ValueError, match="grid='tanh' with (mapping|vortex_metrics)"):
        Sv.FVSolver(**dict(base, mapping="chip", vortex_metrics="chip"))
    with pytest.raises(ValueError, match=r"vortex_refine='quadratic'.*streamfunction='reference'"):
        Sv.FVSolver(**dict(base, vortex_refine="quadratic"))
    # the uniform kernel's spelling stays refused on a stretched mesh, and the new one on a uniform mesh
    for extra in (dict(), dict(vortex_refine="quadratic")):
        with pytest.raises(ValueError, match="grid='tanh' with streamfunction='wall'.*'wall_stretched'"):
            Sv.FVSolver(**dict(base, streamfunction="wall", **extra))
        with pytest.raises(ValueError, match="streamfunction='wall_stretched' with grid='uniform'"):
            Sv.FVSolver(**dict(base, grid="uniform", streamfunction="wall_stretched", **extra))
    with pytest.raises(ValueError, match="streamfunction='face'"):
        Sv.FVSolver(**dict(base, streamfunction="face"))
    for extra in (dict(), wall):
        with pytest.raises(ValueError, match="grid='tanh' with solver=fv/fsg"):
            FVFSGSolver(**dict(base, **extra))
    ns = lambda **kw: type("T", (), dict(device=torch.device("cpu"), **kw))()        # noqa: E731
    with pytest.raises(ValueError, match="start_from with grid='tanh'"):
        Sv.prolong([(ns(stretched=False), ns(stretched=True, stretched_wall=True))])
    with pytest.raises(ValueError, match="grid='tanh' trials with streamfunction='reference'"):
        Sv.postprocess([ns(stretched=True, stretched_wall=False)])


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from solvers.fv import ldc_fv_lib
    return ldc_fv_lib


POINTERS = ("u", "v", "ulid", "x_grid", "y_grid", "x_post", "y_post", "psi", "omega", "scratch", "result")


def _job(F, **over):
    j = F.WallStretchedJob()
    for n in POINTERS:
        setattr(j, n, 8)                              # never dereferenced: validation comes first
    j.nx, j.ny = 32, 20
    j.ix_lt, j.ix_gt, j.jy_lt, j.jy_gt, j.refine = 16, 16, 10, 10, 1
    for k, v in over.items():
        setattr(j, k, v)
    return j


def test_header_binding_and_exports_agree(lib):
    hdr = (ROOT / "include" / "ldc_fv.h").read_text()
    declared = set(re.findall(r"\b(ldc_[a-z_0-9]+)\s*\(", hdr))
    for name in ("ldc_fv_wall_stretched_post_enqueue", "ldc_fv_wall_stretched_post_launches"):
        assert name in declared and name in lib.EXPORTS and hasattr(lib.lib(), name)
    assert set(lib.EXPORTS) <= declared
    define = lambda n: int(re.search(rf"#define {n} (-?\d+)", hdr).group(1))          # noqa: E731
    assert define("LDC_FV_WALL_STRETCHED_LAUNCH_MAX") == lib.WALL_STRETCHED_LAUNCH_MAX == S.LAUNCH_MAX
    assert define("LDC_FV_VERSION") == 2 and lib.lib().ldc_fv_version() == 2 == lib.VERSION
    assert C.sizeof(lib.WallJob) == 136 and define("LDC_FV_WALL_LAUNCH_MAX") == 24       # the uniform entry is as it was
    # the layout of the header: 11 pointers, 8 int32; the argument block of a launch stays under 4096 bytes
    assert C.sizeof(lib.WallStretchedJob) == 11 * 8 + 8 * 4 == 120 and lib.WALL_STRETCHED_LAUNCH_MAX * 120 < 4096
    body = re.search(r"struct ldc_fv_wall_stretched_job \{(.*?)\};", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"\*?\s*([A-Za-z_]+)\s*(?:,|$)", decl.strip())]
    assert names == [n for n, _ in lib.WallStretchedJob._fields_]
    offsets = [getattr(lib.WallStretchedJob, n).offset for n in names]
    assert offsets == [8 * k for k in range(11)] + [88 + 4 * k for k in range(8)]
    for n in (8, 13):
        assert lib.wall_stretched_table_len(n) == n * (n + 2) == S.post_table(S.axis(n)).size
        assert lib.grid_table_len(n) == 3 * n + 2 == S.grid_table(S.axis(n)).size
    assert re.search(r"#define LDC_FV_WALL_STRETCHED_TABLE_LEN\(n\) \(\(int64_t\)\(n\) \* \(\(int64_t\)\(n\) \+ 2\)\)", hdr)


def test_launch_count(lib):
    L = lib.lib()
    m = lib.WALL_STRETCHED_LAUNCH_MAX
    assert [L.ldc_fv_wall_stretched_post_launches(n) for n in (1, m, m + 1, 2 * m, 2 * m + 1, 256)] == \
        [7, 7, 14, 14, 21, 7 * ((256 + m - 1) // m)]
    assert L.ldc_fv_wall_stretched_post_launches(0) == -1 and L.ldc_fv_wall_stretched_post_launches(-4) == -1


REFUSED = [{n: None} for n in POINTERS] + [
    dict(nx=7), dict(ny=7), dict(nx=1025), dict(ny=1025), dict(nx=0), dict(ny=-3), dict(ix_lt=-1), dict(ix_lt=33),
    dict(ix_gt=-1), dict(ix_gt=33), dict(jy_lt=-1), dict(jy_lt=21), dict(jy_gt=-1), dict(jy_gt=21), dict(refine=2),
    dict(refine=-1)]


def test_refused_arguments_need_no_device(lib):
    L = lib.lib()
    assert L.ldc_fv_wall_stretched_post_enqueue(None, 1, None) == -1
    assert L.ldc_fv_wall_stretched_post_enqueue(C.byref(_job(lib)), 0, None) == -1
    assert L.ldc_fv_wall_stretched_post_enqueue(C.byref(_job(lib)), -2, None) == -1
    for over in REFUSED:
        assert L.ldc_fv_wall_stretched_post_enqueue(C.byref(_job(lib, **over)), 1, None) == -1, over
        pair = (lib.WallStretchedJob * 2)(_job(lib), _job(lib, **over))          # the second job of a call is checked too
        assert L.ldc_fv_wall_stretched_post_enqueue(pair, 2, None) == -1, over
    import torch
    if not torch.cuda.is_available():                 # the ends of the ranges pass validation: LDC_E_NODEVICE
        for ok in (dict(nx=8, ny=1024, ix_lt=0, ix_gt=8, jy_lt=1024, jy_gt=0), dict(refine=0), dict(nx=1024, ny=8, jy_lt=8, jy_gt=8)):
            assert L.ldc_fv_wall_stretched_post_enqueue(C.byref(_job(lib, **ok)), 1, None) == -3, ok
