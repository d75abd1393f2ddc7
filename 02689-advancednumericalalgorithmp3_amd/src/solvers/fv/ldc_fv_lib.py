"""ctypes binding of the finite-volume entry points of ``libldc_hip.so`` (C ABI: ``include/ldc_fv.h``).

The same library and loader as the spectral solver (solvers.spectral.ldc_lib): Python owns the device memory as torch
tensors and hands raw pointers to the HIP kernel.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

from solvers.spectral import ldc_lib as _L

VERSION = 2
MIN_N, MAX_N = 8, 256
REC_LEN, CTRL_LEN = 8, 8
NWORK, DESC_DOUBLES = 32, 64
LAUNCH_MAX = 256
PROLONG_LAUNCH_MAX = 128
SAMPLE_LAUNCH_MAX = 32         # LDC_FV_SAMPLE_LAUNCH_MAX: jobs per launch of ldc_fv_sample_nodes
ANDERSON_LAUNCH_MAX, ANDERSON_MAX_DEPTH, ANDERSON_STATE_LEN = 96, 16, 4
ASTATE_COLUMNS, ASTATE_POSITION, ASTATE_SEEN, ASTATE_FALLBACKS = range(4)
E_NAN = -5
WIDE_MAX_N = 1024
WIDE_BATCH_MAX, WIDE_BATCH_ENTRY_BYTES = 256, 256        # LDC_FV_WIDE_BATCH_MAX, LDC_FV_WIDE_BATCH_ENTRY_BYTES
WIDE_ANDERSON_LAUNCHES = 3     # LDC_FV_WIDE_ANDERSON_LAUNCHES: push | mix | close behind every iteration
E_BUDGET = -6                  # ldc_fv_wide_status: the last enqueue ran out of BiCGSTAB launches (LDC_FV_WIDE_E_BUDGET)
# the consistent pressure equation of a chip or shared trial (ldc_fv_wide_set_pressure): modes, launches of one CG iteration,
# the default budget, the statistics words, and the values of the overflow word (which budget was too small)
PRESSURE_MODES = {"reference": 0, "consistent": 1}
WIDE_PRESSURE_LAUNCHES, WIDE_PRESSURE_BUDGET_DEFAULT, WIDE_PRESSURE_SCRATCH_LEN = 7, 12, 4
PSTAT_ITERS, PSTAT_SOLVES, PSTAT_CAPS, PSTAT_LAST = range(4)
PRESSURE_STATS_LEN = 4         # LDC_FV_PRESSURE_STATS_LEN: the same four words for a one-CU trial (ldc_fv_set_pressure)
OVERFLOW_LINEAR, OVERFLOW_PRESSURE = 1, 2
GRID_MODES = {"uniform": 0, "tanh": 1}      # LDC_FV_GRID_UNIFORM, LDC_FV_GRID_TABLES (ldc_fv_set_grid)
PRECOND_MODES = {"laplacian": 0, "separable": 1}    # LDC_FV_PRECOND_LAPLACIAN, LDC_FV_PRECOND_SEPARABLE (ldc_fv_set_preconditioner)
CTRL_DONE, CTRL_ITER, CTRL_NAN, CTRL_GIVEUP, CTRL_LIN_ITERS, CTRL_SOLVES = range(6)
# slots of a result block of ldc_fv_post_enqueue (LDC_FV_POST_*)
(POST_PSI_MIN, POST_OMEGA_CENTER, POST_OMEGA_MAX, POST_PSI_BR, POST_PSI_BL, POST_PSI_TL, POST_PSI_MIN_CELL,
 POST_OMEGA_MAX_CELL, POST_PSI_BR_CELL, POST_PSI_BL_CELL, POST_PSI_TL_CELL, POST_NONFINITE) = range(12)
POST_RESULT_LEN = 16
# ldc_fv_wall_post_enqueue: jobs per launch, the result block (the POST_* slots, then four groups of WALL_GROUP_LEN doubles:
# the primary minimum, BR, BL, TL), the slots of a group and its status codes (LDC_FV_WALL_*)
WALL_LAUNCH_MAX = 24
WALL_GROUP_LEN, WALL_RESULT_LEN = 8, 48
WALL_X, WALL_Y, WALL_PSI, WALL_OMEGA, WALL_STATUS, WALL_SX, WALL_SY = range(7)
WALL_NOT_ASKED, WALL_REFINED, WALL_NO_CANDIDATE, WALL_INDEFINITE, WALL_REJECTED = -1, 0, 1, 2, 3
WALL_POST_LAUNCHES = 7         # omega | gemm x 4 | extrema | result, per group of WALL_LAUNCH_MAX jobs
WALL_STRETCHED_LAUNCH_MAX = 32     # LDC_FV_WALL_STRETCHED_LAUNCH_MAX: jobs per launch of ldc_fv_wall_stretched_post_enqueue
PROLONG_TABLES_LAUNCH_MAX = 23     # LDC_FV_PROLONG_TABLES_LAUNCH_MAX: jobs per launch of ldc_fv_prolong_tables_enqueue
WIDE_PROLONG_TABLES_LAUNCHES = 2   # LDC_FV_WIDE_PROLONG_TABLES_LAUNCHES: cells | faces, per job of ldc_fv_wide_prolong_tables_enqueue
DBG = ("grad_p", "diag", "b", "u_star", "v_star", "mdot_star", "rhs_p", "p_prime", "u_prime", "v_prime", "mdot")

_dp = C.c_void_p


class Problem(C.Structure):
    """Mirror of ``struct ldc_fv_problem`` -- keep field order in sync with the header."""
    _fields_ = (
        [(n, C.c_int32) for n in ("nx", "ny", "scheme", "rec_cap", "warmup", "max_lin_iters")]
        + [(n, C.c_double) for n in ("dx", "dy", "rho", "mu", "alpha_uv", "alpha_p", "lin_tol", "tol", "lid_velocity")]
        + [(n, _dp) for n in ("ulid", "Qx", "lamx", "Qy", "lamy", "u", "v", "p", "mdot", "work", "rec", "ctrl")]
    )


class Post(C.Structure):
    """Mirror of ``struct ldc_fv_post`` -- keep field order in sync with the header."""
    _fields_ = (
        [(n, _dp) for n in ("Sx", "lamx", "Sy", "lamy")]
        + [(n, C.c_int32) for n in ("ix_lt", "ix_gt", "jy_lt", "jy_gt")]
        + [(n, _dp) for n in ("psi", "omega", "result")]
    )


class Anderson(C.Structure):
    """Mirror of ``struct ldc_fv_anderson`` -- keep field order in sync with the header."""
    _fields_ = [("depth", C.c_int32), ("start", C.c_int32), ("hist", _dp), ("hist_len", C.c_int64), ("astate", _dp)]


class Pressure(C.Structure):
    """Mirror of ``struct ldc_fv_pressure`` -- keep field order in sync with the header."""
    _fields_ = [("mode", C.c_int32), ("max_iters", C.c_int32), ("tol", C.c_double)]


class Grid(C.Structure):
    """Mirror of ``struct ldc_fv_grid`` -- keep field order in sync with the header."""
    _fields_ = [("mode", C.c_int32), ("pad", C.c_int32), ("x_tables", _dp), ("y_tables", _dp), ("x_len", C.c_int64),
                ("y_len", C.c_int64)]


class Precond(C.Structure):
    """Mirror of ``struct ldc_fv_precond`` -- keep field order in sync with the header."""
    _fields_ = [("mode", C.c_int32), ("pad", C.c_int32), ("x_table", _dp), ("y_table", _dp), ("x_len", C.c_int64),
                ("y_len", C.c_int64)]


class SampleJob(C.Structure):
    """Mirror of ``struct ldc_fv_sample_job`` -- keep field order in sync with the header."""
    _fields_ = (
        [(n, _dp) for n in ("u", "v", "p", "ulid")]
        + [("nx", C.c_int32), ("ny", C.c_int32), ("dx", C.c_double), ("dy", C.c_double)]
        + [(n, _dp) for n in ("x", "y", "ulid_nodes")]
        + [("Mx", C.c_int32), ("My", C.c_int32)]
        + [(n, _dp) for n in ("U", "V", "P")]
    )


class WallJob(C.Structure):
    """Mirror of ``struct ldc_fv_wall_job`` -- keep field order in sync with the header."""
    _fields_ = (
        [(n, _dp) for n in ("u", "v", "ulid", "Cx", "lamx", "Cy", "lamy", "psi", "omega", "scratch", "result")]
        + [("dx", C.c_double), ("dy", C.c_double)]
        + [(n, C.c_int32) for n in ("nx", "ny", "ix_lt", "ix_gt", "jy_lt", "jy_gt", "refine", "pad")]
    )


class WallStretchedJob(C.Structure):
    """Mirror of ``struct ldc_fv_wall_stretched_job`` -- keep field order in sync with the header."""
    _fields_ = (
        [(n, _dp) for n in ("u", "v", "ulid", "x_grid", "y_grid", "x_post", "y_post", "psi", "omega", "scratch", "result")]
        + [(n, C.c_int32) for n in ("nx", "ny", "ix_lt", "ix_gt", "jy_lt", "jy_gt", "refine", "pad")]
    )


class ProlongTablesJob(C.Structure):
    """Mirror of ``struct ldc_fv_prolong_tables_job`` -- keep field order in sync with the header."""
    _fields_ = (
        [(n, _dp) for n in ("coarse_u", "coarse_v", "coarse_p", "coarse_ulid", "coarse_xc", "coarse_yc", "fine_u", "fine_v",
                            "fine_p", "fine_mdot", "fine_x_grid", "fine_y_grid", "fine_xc", "fine_yc")]
        + [(n, C.c_double) for n in ("Lx", "Ly", "rho")]
        + [(n, C.c_int32) for n in ("coarse_nx", "coarse_ny", "fine_nx", "fine_ny")]
    )


# every symbol include/ldc_fv.h declares (tests check the .so exports all of them)
EXPORTS = ("ldc_fv_version", "ldc_fv_create", "ldc_fv_destroy", "ldc_fv_enqueue", "ldc_fv_batch_enqueue",
           "ldc_fv_status", "ldc_fv_step_debug", "ldc_fv_set_pressure", "ldc_fv_set_grid", "ldc_fv_set_preconditioner", "ldc_fv_post_enqueue", "ldc_fv_prolong_enqueue",
           "ldc_fv_anderson_enqueue", "ldc_fv_wide_create", "ldc_fv_wide_destroy", "ldc_fv_wide_enqueue",
           "ldc_fv_wide_launches", "ldc_fv_wide_status", "ldc_fv_wide_set_graph", "ldc_fv_wide_batch_create",
           "ldc_fv_wide_batch_destroy", "ldc_fv_wide_batch_enqueue", "ldc_fv_wide_batch_set_graph",
           "ldc_fv_wide_batch_launches", "ldc_fv_wide_post_enqueue", "ldc_fv_wide_post_launches",
           "ldc_fv_wide_prolong_enqueue", "ldc_fv_wide_set_anderson", "ldc_fv_wide_set_pressure",
           "ldc_fv_wide_set_pressure_budget", "ldc_fv_wide_batch_set_pressure_budget", "ldc_fv_wide_set_grid",
           "ldc_fv_wide_set_preconditioner",
           "ldc_fv_sample_nodes",
           "ldc_fv_wall_post_enqueue", "ldc_fv_wall_post_launches", "ldc_fv_wall_stretched_post_enqueue",
           "ldc_fv_wall_stretched_post_launches", "ldc_fv_prolong_tables_enqueue", "ldc_fv_prolong_tables_launches",
           "ldc_fv_wide_prolong_tables_enqueue", "ldc_fv_wide_prolong_tables_launches")

_bound = None


def work_len(nx: int, ny: int) -> int:
    return NWORK * nx * ny + DESC_DOUBLES


def faces(nx: int, ny: int) -> int:
    return ny * (nx + 1) + (ny + 1) * nx


def anderson_hist_len(nx: int, ny: int, depth: int) -> int:
    """x, g_prev, f_prev and ``depth`` columns each of dG and dF, every one [u | v | p | mdot]."""
    return (2 * depth + 3) * (3 * nx * ny + faces(nx, ny))


def wide_groups(nx: int, ny: int) -> int:
    """Work-groups of a cell sweep of the chip mapping (LDC_FV_WIDE_GROUPS)."""
    return min(256, (nx * ny + 255) // 256)


def wide_scratch_len(nx: int, ny: int) -> int:
    """LDC_FV_WIDE_SCRATCH_LEN: control words, two copies of the BiCGSTAB scalars, three sets of slot sums."""
    return 80 + 30 * wide_groups(nx, ny)


def wide_post_scratch_len(nx: int, ny: int) -> int:
    """LDC_FV_WIDE_POST_SCRATCH_LEN: one slot of 12 doubles per work-group of a cell sweep (five keys, five cells, two
    not-finite flags)."""
    return 12 * wide_groups(nx, ny)


def wall_scratch_len(nx: int, ny: int) -> int:
    """LDC_FV_WALL_SCRATCH_LEN: two fields of n doubles, then one slot of 12 doubles per work-group of a cell sweep."""
    return 2 * nx * ny + 12 * wide_groups(nx, ny)


def wide_anderson_scratch_len(nx: int, ny: int, depth: int) -> int:
    """LDC_FV_WIDE_ANDERSON_SCRATCH_LEN: 8 words, then per work-group of a sweep b[depth] and the lower triangle of A."""
    return 8 + wide_groups(nx, ny) * (depth * (depth + 3) // 2)


def wide_gemm_groups(nx: int, ny: int) -> int:
    """Work-groups of one GEMM launch of a chip or shared trial (LDC_FV_WIDE_GEMM_GROUPS): four 16 x 16 tiles each."""
    return (((ny + 15) // 16) * ((nx + 15) // 16) + 3) // 4


def wide_batch_table_len(sizes) -> int:
    """LDC_FV_WIDE_BATCH_TABLE_LEN for trials of ``sizes`` [(nx, ny)]: the BYTES of the batch's table."""
    sizes = list(sizes)
    return (WIDE_BATCH_ENTRY_BYTES * len(sizes)
            + 4 * sum(wide_groups(nx, ny) + wide_gemm_groups(nx, ny) for nx, ny in sizes))


def lib() -> C.CDLL:
    """The shared library with the FV entry points' signatures set (raises if it has not been built)."""
    global _bound
    L = _L.lib()
    if _bound is None:
        missing = [name for name in EXPORTS if not hasattr(L, name)]
        if missing:               # (the entry points after ldc_fv_post_enqueue came without a new version number)
            raise _L.LdcError(f"libldc_hip.so is out of date: it does not export {', '.join(missing)}; rebuild it")
        L.ldc_fv_version.restype = C.c_int
        L.ldc_fv_create.argtypes = [C.POINTER(Problem), C.POINTER(_dp)]
        L.ldc_fv_destroy.argtypes = [_dp]
        L.ldc_fv_enqueue.argtypes = [_dp, C.c_int, _dp]
        L.ldc_fv_batch_enqueue.argtypes = [C.POINTER(_dp), C.c_int, C.c_int, _dp]
        L.ldc_fv_status.argtypes = [_dp]
        L.ldc_fv_step_debug.argtypes = [_dp, C.c_int, C.POINTER(_dp), _dp]
        L.ldc_fv_set_pressure.argtypes = [_dp, C.POINTER(Pressure), _dp, C.c_int64]
        L.ldc_fv_set_grid.argtypes = [_dp, C.POINTER(Grid)]
        L.ldc_fv_set_preconditioner.argtypes = [_dp, C.POINTER(Precond)]
        L.ldc_fv_post_enqueue.argtypes = [C.POINTER(_dp), C.POINTER(Post), C.c_int, _dp]
        L.ldc_fv_prolong_enqueue.argtypes = [C.POINTER(_dp), C.POINTER(_dp), C.c_int, _dp]
        L.ldc_fv_anderson_enqueue.argtypes = [C.POINTER(_dp), C.POINTER(Anderson), C.c_int, C.c_int, _dp]
        L.ldc_fv_wide_create.argtypes = [C.POINTER(Problem), _dp, C.c_int64, C.POINTER(_dp)]
        L.ldc_fv_wide_destroy.argtypes = [_dp]
        L.ldc_fv_wide_enqueue.argtypes = [_dp, C.c_int, C.c_int, _dp]
        L.ldc_fv_wide_launches.argtypes = [_dp, C.c_int]
        L.ldc_fv_wide_status.argtypes = [_dp]
        L.ldc_fv_wide_set_graph.argtypes = [_dp, C.c_int]
        L.ldc_fv_wide_batch_create.argtypes = [C.POINTER(_dp), C.c_int, _dp, C.c_int64, C.POINTER(_dp)]
        L.ldc_fv_wide_batch_destroy.argtypes = [_dp]
        L.ldc_fv_wide_batch_enqueue.argtypes = [_dp, C.POINTER(C.c_int32), C.c_int, _dp]
        L.ldc_fv_wide_batch_set_graph.argtypes = [_dp, C.c_int]
        L.ldc_fv_wide_batch_launches.argtypes = [_dp, C.c_int]
        L.ldc_fv_wide_post_enqueue.argtypes = [_dp, C.POINTER(Post), _dp, C.c_int64, _dp]
        L.ldc_fv_wide_post_launches.argtypes = [_dp]
        L.ldc_fv_wide_prolong_enqueue.argtypes = [_dp, _dp, _dp]
        L.ldc_fv_wide_set_anderson.argtypes = [_dp, C.POINTER(Anderson), _dp, C.c_int64]
        L.ldc_fv_wide_set_pressure.argtypes = [_dp, C.POINTER(Pressure), _dp, C.c_int64]
        L.ldc_fv_wide_set_pressure_budget.argtypes = [_dp, C.c_int]
        L.ldc_fv_wide_set_grid.argtypes = [_dp, C.POINTER(Grid)]
        L.ldc_fv_wide_set_preconditioner.argtypes = [_dp, C.POINTER(Precond)]
        L.ldc_fv_wide_batch_set_pressure_budget.argtypes = [_dp, C.c_int]
        L.ldc_fv_sample_nodes.argtypes = [C.POINTER(SampleJob), C.c_int, _dp]
        L.ldc_fv_wall_post_enqueue.argtypes = [C.POINTER(WallJob), C.c_int, _dp]
        L.ldc_fv_wall_post_launches.argtypes = [C.c_int]
        L.ldc_fv_wall_stretched_post_enqueue.argtypes = [C.POINTER(WallStretchedJob), C.c_int, _dp]
        L.ldc_fv_wall_stretched_post_launches.argtypes = [C.c_int]
        L.ldc_fv_prolong_tables_enqueue.argtypes = [C.POINTER(ProlongTablesJob), C.c_int, _dp]
        L.ldc_fv_prolong_tables_launches.argtypes = [C.c_int]
        L.ldc_fv_wide_prolong_tables_enqueue.argtypes = [C.POINTER(ProlongTablesJob), C.c_int, _dp]
        L.ldc_fv_wide_prolong_tables_launches.argtypes = [C.c_int]
        for name in EXPORTS:
            getattr(L, name).restype = C.c_int
        _bound = L
    return L


def check(code: int, what: str = "ldc_fv call"):
    if code == E_NAN:
        raise _L.LdcError(f"{what}: the finite-volume trial produced a NaN and stopped (code {code})")
    _L.check(code, what)


def batch_enqueue(handles, n_iters: int, stream) -> None:
    """One launch (per LAUNCH_MAX trials) advancing every handle by up to n_iters iterations."""
    arr = (_dp * len(handles))(*[h.value if isinstance(h, _dp) else h for h in handles])
    check(lib().ldc_fv_batch_enqueue(arr, len(handles), int(n_iters), _dp(stream)), "ldc_fv_batch_enqueue")


def set_pressure(handle, mode: str, tol: float, max_iters: int, stats_ptr: int = None,
                 stats_len: int = PRESSURE_STATS_LEN) -> None:
    """The pressure equation of an ``ldc_fv`` handle (a one-CU trial): ``"reference"`` or ``"consistent"`` (CG inside the
    trial's work-group to ``tol``, at most ``max_iters`` iterations, statistics in the caller's ``stats_len`` int64
    words).  One synchronous copy into the tail of the trial's work buffer: nothing of the handle may be in flight."""
    cfg = Pressure(mode=PRESSURE_MODES[mode], max_iters=int(max_iters), tol=float(tol))
    check(lib().ldc_fv_set_pressure(handle, C.byref(cfg), _dp(stats_ptr), int(stats_len)), "ldc_fv_set_pressure")


def grid_table_len(n: int) -> int:
    """LDC_FV_GRID_TABLE_LEN: one axis' table [h (n) | d (n + 1) | g (n + 1)]."""
    return 3 * n + 2


def set_grid(handle, x_tables_ptr: int, x_len: int, y_tables_ptr: int, y_len: int) -> None:
    """Attach the per-axis geometry tables to an ``ldc_fv`` handle (a one-CU trial on a stretched grid; include/ldc_fv.h).
    One synchronous copy into the tail of the trial's work buffer: nothing of the handle may be in flight."""
    cfg = Grid(mode=GRID_MODES["tanh"], pad=0, x_tables=x_tables_ptr, y_tables=y_tables_ptr, x_len=int(x_len),
               y_len=int(y_len))
    check(lib().ldc_fv_set_grid(handle, C.byref(cfg)), "ldc_fv_set_grid")


def precond_table_len(n: int) -> int:
    """LDC_FV_PRECOND_TABLE_LEN: one axis' table [a (n) | lam (n) | Q (n x n)]."""
    return n * (n + 2)


def set_preconditioner(handle, x_table_ptr: int, x_len: int, y_table_ptr: int, y_len: int) -> None:
    """Attach the per-axis tables of the separable scaled preconditioner to an ``ldc_fv`` handle with geometry tables
    (include/ldc_fv.h).  One synchronous copy into the tail of the trial's work buffer: nothing of the handle may be in flight."""
    cfg = Precond(mode=PRECOND_MODES["separable"], pad=0, x_table=x_table_ptr, y_table=y_table_ptr, x_len=int(x_len),
                  y_len=int(y_len))
    check(lib().ldc_fv_set_preconditioner(handle, C.byref(cfg)), "ldc_fv_set_preconditioner")


def post_enqueue(handles, posts, stream) -> None:
    """omega, psi and the result block of every handle (``posts``: one ``Post`` each), one launch per LAUNCH_MAX."""
    arr = (_dp * len(handles))(*[h.value if isinstance(h, _dp) else h for h in handles])
    blocks = (Post * len(posts))(*posts)
    check(lib().ldc_fv_post_enqueue(arr, blocks, len(handles), _dp(stream)), "ldc_fv_post_enqueue")


def prolong_enqueue(coarse_handles, fine_handles, stream) -> None:
    """fine_handles[q] <- the prolongation of coarse_handles[q] (u, v, p, mdot; include/ldc_fv.h), one work-group per
    pair, any number of pairs: the library launches PROLONG_LAUNCH_MAX at a time and checks all of them first."""
    if len(coarse_handles) != len(fine_handles):
        raise ValueError(f"{len(coarse_handles)} coarse handles for {len(fine_handles)} fine ones")
    raw = lambda hs: (_dp * len(hs))(*[h.value if isinstance(h, _dp) else h for h in hs])        # noqa: E731
    check(lib().ldc_fv_prolong_enqueue(raw(coarse_handles), raw(fine_handles), len(fine_handles), _dp(stream)),
          "ldc_fv_prolong_enqueue")


def anderson_enqueue(handles, blocks, n_iters: int, stream) -> None:
    """``n_iters`` times: one SIMPLE iteration of every handle, then the mixing kernel (``blocks``: one ``Anderson``
    each, depth 0 for a plain trial); all enqueued, nothing synchronises."""
    if len(handles) != len(blocks):
        raise ValueError(f"{len(blocks)} Anderson blocks for {len(handles)} handles")
    arr = (_dp * len(handles))(*[h.value if isinstance(h, _dp) else h for h in handles])
    acc = (Anderson * len(blocks))(*blocks)
    check(lib().ldc_fv_anderson_enqueue(arr, acc, len(handles), int(n_iters), _dp(stream)), "ldc_fv_anderson_enqueue")


def wide_batch_create(handles, table_ptr: int, table_len: int) -> _dp:
    """The batch object of ``handles`` (ldc_fv_wide handles of one device) with its table in the caller's device buffer."""
    arr = (_dp * len(handles))(*[h.value if isinstance(h, _dp) else h for h in handles])
    out = _dp()
    check(lib().ldc_fv_wide_batch_create(arr, len(handles), _dp(table_ptr), int(table_len), C.byref(out)),
          "ldc_fv_wide_batch_create")
    return out


def wide_batch_enqueue(batch, quotas, lin_budget: int, stream) -> None:
    """``quotas[q]`` iterations of trial q (0: the trial is left alone), all in the same launches; nothing synchronises."""
    arr = (C.c_int32 * len(quotas))(*[int(k) for k in quotas])
    check(lib().ldc_fv_wide_batch_enqueue(batch, arr, int(lin_budget), _dp(stream)), "ldc_fv_wide_batch_enqueue")


def wide_post_enqueue(wide, post: Post, scratch_ptr: int, scratch_len: int, stream) -> None:
    """omega, psi and the result block of ONE chip or shared trial (its ``ldc_fv_wide`` handle) by the whole chip: the
    launches of ``ldc_fv_wide_post_launches``, all enqueued; nothing synchronises."""
    check(lib().ldc_fv_wide_post_enqueue(wide, C.byref(post), _dp(scratch_ptr), int(scratch_len), _dp(stream)),
          "ldc_fv_wide_post_enqueue")


def wide_prolong_enqueue(coarse, fine, stream) -> None:
    """fine <- the prolongation of coarse, both ``ldc_fv_wide`` handles of one device: two launches over the chip."""
    check(lib().ldc_fv_wide_prolong_enqueue(coarse, fine, _dp(stream)), "ldc_fv_wide_prolong_enqueue")


def wide_set_anderson(wide, block, scratch_ptr: int = None, scratch_len: int = 0) -> None:
    """Attach the mixing chain to an ``ldc_fv_wide`` handle (``block``: an ``Anderson`` of depth >= 1, with the mixing
    scratch) or detach it (``None`` or depth 0).  A batch copies the block when it is created: attach first."""
    check(lib().ldc_fv_wide_set_anderson(wide, C.byref(block) if block is not None else None, _dp(scratch_ptr),
                                         int(scratch_len)), "ldc_fv_wide_set_anderson")


def wide_set_pressure(wide, mode: str, tol: float, max_iters: int, stats_ptr: int = None,
                      stats_len: int = WIDE_PRESSURE_SCRATCH_LEN) -> None:
    """The pressure equation of an ``ldc_fv_wide`` handle: ``"reference"`` or ``"consistent"`` (CG to ``tol``, at most
    ``max_iters`` iterations, statistics in the caller's ``stats_len`` int64 words).  A batch copies the block when it is
    created: set it first."""
    cfg = Pressure(mode=PRESSURE_MODES[mode], max_iters=int(max_iters), tol=float(tol))
    check(lib().ldc_fv_wide_set_pressure(wide, C.byref(cfg), _dp(stats_ptr), int(stats_len)), "ldc_fv_wide_set_pressure")


def wide_set_grid(wide, x_tables_ptr: int, x_len: int, y_tables_ptr: int, y_len: int) -> None:
    """Attach the per-axis geometry tables of ``set_grid`` to an ``ldc_fv_wide`` handle (a lone chip trial on a stretched grid;
    include/ldc_fv.h).  The pointers travel in the kernel arguments: nothing is copied; the handle's graphs are freed."""
    cfg = Grid(mode=GRID_MODES["tanh"], pad=0, x_tables=x_tables_ptr, y_tables=y_tables_ptr, x_len=int(x_len),
               y_len=int(y_len))
    check(lib().ldc_fv_wide_set_grid(wide, C.byref(cfg)), "ldc_fv_wide_set_grid")


def wide_set_preconditioner(wide, x_table_ptr: int, x_len: int, y_table_ptr: int, y_len: int) -> None:
    """Attach the per-axis tables of ``set_preconditioner`` to an ``ldc_fv_wide`` handle with geometry tables (the separable
    scaled preconditioner of a lone chip trial; include/ldc_fv.h).  The pointers travel in the kernel arguments: nothing is
    copied; the handle's graphs are freed."""
    cfg = Precond(mode=PRECOND_MODES["separable"], pad=0, x_table=x_table_ptr, y_table=y_table_ptr, x_len=int(x_len),
                  y_len=int(y_len))
    check(lib().ldc_fv_wide_set_preconditioner(wide, C.byref(cfg)), "ldc_fv_wide_set_preconditioner")


def sample_nodes(jobs, stream) -> None:
    """U, V, P of every ``SampleJob`` from its FV state (include/ldc_fv.h): ONE call for all jobs, which the library
    checks first and launches SAMPLE_LAUNCH_MAX at a time; nothing synchronises."""
    arr = (SampleJob * len(jobs))(*jobs)
    check(lib().ldc_fv_sample_nodes(arr, len(jobs), _dp(stream)), "ldc_fv_sample_nodes")


def wall_post_enqueue(jobs, stream) -> None:
    """omega, the wall-anchored psi and the result block of every ``WallJob`` (include/ldc_fv.h): ONE call for all jobs,
    which the library checks first and launches WALL_LAUNCH_MAX at a time, seven launches each; nothing synchronises."""
    arr = (WallJob * len(jobs))(*jobs)
    check(lib().ldc_fv_wall_post_enqueue(arr, len(jobs), _dp(stream)), "ldc_fv_wall_post_enqueue")


def wall_stretched_table_len(n: int) -> int:
    """LDC_FV_WALL_STRETCHED_TABLE_LEN: one axis' post table [xc (n) | lam (n) | Q (n x n)]."""
    return n * (n + 2)


def wall_stretched_post_enqueue(jobs, stream) -> None:
    """The same for every ``WallStretchedJob`` (a trial on a stretched tensor grid; include/ldc_fv.h): ONE call for all jobs,
    which the library checks first and launches WALL_STRETCHED_LAUNCH_MAX at a time, seven launches each; nothing synchronises."""
    arr = (WallStretchedJob * len(jobs))(*jobs)
    check(lib().ldc_fv_wall_stretched_post_enqueue(arr, len(jobs), _dp(stream)), "ldc_fv_wall_stretched_post_enqueue")


def prolong_tables_enqueue(jobs, stream) -> None:
    """The fine u, v, p and mdot of every ``ProlongTablesJob`` from its coarse state, the geometry of both read from tables
    (tensor grids with any spacing per axis; include/ldc_fv.h): ONE call for all jobs, which the library checks first and
    launches PROLONG_TABLES_LAUNCH_MAX at a time, one work-group each; nothing synchronises."""
    arr = (ProlongTablesJob * len(jobs))(*jobs)
    check(lib().ldc_fv_prolong_tables_enqueue(arr, len(jobs), _dp(stream)), "ldc_fv_prolong_tables_enqueue")


def wide_prolong_tables_enqueue(jobs, stream) -> None:
    """The same for jobs of 8 ... 1024 cells per axis on either side, by the chip mapping's rules (include/ldc_fv.h): ONE call
    for all jobs, which the library checks first and launches one after another, two launches over the whole chip each;
    nothing synchronises."""
    arr = (ProlongTablesJob * len(jobs))(*jobs)
    check(lib().ldc_fv_wide_prolong_tables_enqueue(arr, len(jobs), _dp(stream)), "ldc_fv_wide_prolong_tables_enqueue")
