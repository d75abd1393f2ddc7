"""The stretched chip chain (grid="tanh", mapping="chip", chip_grid="tables"; csrc/ldc_fv_wide_stretched.inc,
csrc/ldc_fv_wide_separable.inc) phase by phase and at low Krylov caps: the cases and references of
tests/test_fv_wide_stretched_edges_cpu.py and tests/test_gpu_fv_wide_stretched_edges.py (test helper, no test in it).

Nothing here is new arithmetic.  The phase cases, their references and the work-vector table are those of
tests/fv_stretched_probe.py (the one-CU stretched kernels share the cell bodies and the ``FvVec`` indices with the chip chain);
the seed formula, the lost-share mutants, the distances and the bounds are those of tests/fv_krylov_probe.py (the uniform chip
chain).  What is new: the three chains' solver settings under their one-CU names, the two work vectors that differ on the chip
(``WSEP_S``, ``WSEP_SR``), the seed evaluated at the stretched cell centres, and the capped, threshold and edge-shape runs of
the stretched restatement (tests/fv_stretched_numpy.py, tests/fv_separable_numpy.py).

Every reference is made once per case (``functools.lru_cache``) and never changed by a caller; the mutants are test doubles of
the RESTATEMENT, never of a kernel.
"""
from __future__ import annotations

import functools

import numpy as np

import fv_krylov_probe as K
import fv_stretched_probe as S
from fv_krylov_probe import MUTANT_BOUND, SENSITIVITY_BOUND, TOL, lost_share, rel, rows_rel  # noqa: F401
from fv_separable_numpy import FVSeparableState
from fv_stretched_numpy import FVStretchedState
from fv_stretched_probe import PHASE_MORE, PHASE_TAGS, PHASE_TOL, phase_case, phase_reference  # noqa: F401

# ---------------------------------------------------------------------------------------------- the three chains
CHAINS = S.KERNELS                      # "reference", "laplacian", "separable": the one-CU names, so the case ids read alike
CHIP = dict(grid="tanh", mapping="chip", chip_grid="tables")
CHIP_MODE = dict(reference=dict(CHIP, pressure_equation="reference"),
                 laplacian=dict(CHIP, pressure_equation="consistent"),
                 separable=dict(CHIP, pressure_equation="consistent", chip_preconditioner="separable"))
CONSISTENT = ("laplacian", "separable")

# The work vectors of the chip chain: the one-CU table with the scaling vectors moved.  The chip CG keeps two copies of p
# (PCG_P and the vector behind it, 14 and 15, alternating by the CG iteration) and q in PCG_Q (16), so the one-CU kernel's
# SEP_S = 15 is taken; s lives in WSEP_S = FV_PHV (18) and s . r in WSEP_SR = FV_SHU (19).
INDEX = dict({k: v for k, v in S.INDEX.items() if k != "SEP_S"}, PCG_P=14, PCG_Q=16, WSEP_S=18, WSEP_SR=19)
PCG_P_COPIES = 2
VEC = dict({k: v for k, v in S.VEC.items() if k != "sep_s"}, sep_s=("WSEP_S",), sep_sr=("WSEP_SR",))
MS_VECTORS = S.MS_VECTORS
# What the one-CU probe reads and no vector of the chip chain holds.  ``b00`` of the reference chain: ``sg_cell_faces`` stores 0.0
# as the right-hand side of cell 0 on every chain, and the first GEMM of the pressure solve (``fv_wide_gemm<true, false>``) takes
# b00 = -(the slot sum of the faces launch) and puts it in place of entry (0, 0) as it loads (``fv_gemm_tile``, FIRST); the
# one-CU reference kernel writes it to FV_C[0].  What a wrong b00 does shows in p' (held to 1e-8) and in everything behind it.
NOT_STORED = dict(reference=("b00",), laplacian=(), separable=())


def intermediates(solver, chain):
    """``fv_stretched_probe.intermediates`` on the chip chain's table: the keys of ``FVStretchedState.step(capture)`` plus
    ``omega``, ``y``, ``row`` and ``mdot``, read from ``solver.t["work"]`` after ``_advance(1)``.  A consistent chain adds
    ``mdot_star`` and ``cg_r``; the separable one ``sep_s`` and ``sep_sr``.  No ``b00`` (``NOT_STORED``)."""
    if chain not in CHAINS:
        raise ValueError(chain)
    nx, ny = solver.nx, solver.ny
    n, nf = nx * ny, ny * (nx + 1) + (ny + 1) * nx
    w = solver.t["work"].cpu().numpy()

    def vec(name, count=1):
        k = INDEX[name]
        return w[k * n: (k + count) * n].copy()

    out = {key: np.concatenate([vec(name) for name in VEC[key]]) for key in ("grad_p", "diag", "b", "u_star", "v_star",
                                                                               "u_prime", "v_prime", "omega")}
    rhs = vec("FV_C")                       # (entry 0 is 0.0 on every chain: see NOT_STORED)
    if chain != "reference":
        out["mdot_star"] = vec("PCG_MS", MS_VECTORS)[:nf]
        out["cg_r"] = vec("PCG_R")
    if chain == "separable":
        out["sep_s"], out["sep_sr"] = vec("WSEP_S"), vec("WSEP_SR")
    y = vec("FV_Y")
    out.update(rhs_p=rhs, y=y, p_prime=y - y[0], mdot=solver.t["mdot"].cpu().numpy().copy(),
               row=solver.t["rec"][0].cpu().numpy().copy())
    return out


def phase_solver_kwargs(m, chain):
    """``fv_stretched_probe.phase_solver_kwargs`` with the chip chain's mode."""
    kw = S.phase_solver_kwargs(m, "reference")
    return dict({k: v for k, v in kw.items() if k not in S.REF}, **CHIP_MODE[chain])


# ---------------------------------------------------------------------------------------------- the seeded state
def seeded_stretched(o):
    """``fv_krylov_probe.seeded`` on an ``FVStretchedState``: the same field formula at the stretched centres xc / Lx, yc / Ly,
    the face values through ``o.faces`` (g-weighted), the fluxes rho u_f hy and rho v_f hx, the wall faces exactly 0.  Returns
    (u, v, p, mdot) flattened for ``FVSolver.set_state``."""
    u, v, p = K.seed_fields(*np.meshgrid(o.xc / o.xv[-1], o.yc / o.yv[-1]))         # (the last vertex is Lx, Ly exactly)
    ux, vy = o.faces(u, v)
    fx, fy = o.rho * ux * o.hy[:, None], o.rho * vy * o.hx[None, :]
    fx[:, 0] = fx[:, -1] = 0.0
    fy[0, :] = fy[-1, :] = 0.0
    mdot = np.concatenate([fx.ravel(), fy.ravel()])
    o.set_state(u.ravel(), v.ravel(), p.ravel(), mdot)
    return u.ravel().copy(), v.ravel().copy(), p.ravel().copy(), mdot


def seed_of(nx, ny, grid_stretch=None):
    """The seed alone, for ``set_state`` (the formula needs the mesh only)."""
    return seeded_stretched(_state("reference", nx, ny, None, None, "none", 1e-12, K.PRESSURE_TOL,
                                   BETA if grid_stretch is None else grid_stretch))


# ---------------------------------------------------------------------------------------------- b, c. capped runs
BETA = 1.5
CG_CAPS = K.CG_CAPS                     # (1, 3)
BICG_CAP = K.BICG_CAP                   # 2
CAP_K = K.K                             # 2 SIMPLE iterations from the seed
# several groups and ragged GEMM tiles; one axis past the one-CU range and the other at MIN_N, both ways; 256 work-groups and a
# second pass of the grid-stride loop; 1024 cells on one axis
CG_SHAPES = [(37, 50), (300, 9), (8, 1024), (272, 260), (1024, 72)]
BIG = (1024, 1024)                      # one case: separable, cap 3, the ``rz`` mutant, not cached
BIG_CASE = ("separable", *BIG, 3)
CG_CASES = [(chain, nx, ny, cap) for chain in CONSISTENT for nx, ny in CG_SHAPES for cap in CG_CAPS] + [BIG_CASE]
BICG_SHAPES = [(37, 50), (300, 9), (272, 260)]
BICG_CHAINS = ("reference", "laplacian")
BICG_CASES = [(chain, nx, ny) for chain in BICG_CHAINS for nx, ny in BICG_SHAPES]
BICG_MOVING = ("bicg_rho", "bicg_rv", "bicg_ts", "bicg_tt")


def cg_mutants(nx, ny):
    return ("rz",) if (nx, ny) == BIG else ("rz", "pq")


def case_id(case):
    return "-".join(str(c) for c in case)


def _state(chain, nx, ny, cg_cap, bicg_cap, lost, linear_solver_tol, pressure_tol, grid_stretch):
    """The restatement of ``chain`` with the settings of ``fv_krylov_probe._state`` (TVD, Re 400, 0.4 / 0.2) on a tanh grid."""
    if chain not in CHAINS:
        raise ValueError(chain)
    cls = FVSeparableState if chain == "separable" else FVStretchedState
    if lost != "none":
        cls = lost_share(cls, lost)
    kw = dict(K.SETTINGS, linear_solver_tol=linear_solver_tol, pressure_solver="cg", pressure_tol=pressure_tol,
              pressure_equation="reference" if chain == "reference" else "consistent", grid_stretch=grid_stretch,
              pressure_max_iters=K.UNCAPPED if cg_cap is None else int(cg_cap))
    if bicg_cap is not None:
        kw["max_lin_iters"] = int(bicg_cap)
    return cls(nx, ny, K.RE, **kw)


def capped_reference(chain, nx, ny, cg_cap=None, bicg_cap=None, lost="none", linear_solver_tol=1e-12, iterations=CAP_K,
                     pressure_tol=K.PRESSURE_TOL, grid_stretch=BETA):
    """``fv_krylov_probe.capped_reference`` on a stretched grid: the restatement of ``chain`` run ``iterations`` SIMPLE
    iterations from ``seeded_stretched``, once per case below ``fv_krylov_probe.CACHED_CELLS`` cells, the arrays read-only.
    ``lost``: "none", None (the copied loops with every sum whole) or a mutant's name.  A dict: u, v, p, mdot (flat), rows,
    iters, exits, cg_iters, cg_caps."""
    run = _cached_run if nx * ny < K.CACHED_CELLS else _run
    return run(chain, nx, ny, cg_cap, bicg_cap, lost, linear_solver_tol, iterations, pressure_tol, grid_stretch)


def _run(chain, nx, ny, cg_cap, bicg_cap, lost, linear_solver_tol, iterations, pressure_tol, grid_stretch):
    o = _state(chain, nx, ny, cg_cap, bicg_cap, lost, linear_solver_tol, pressure_tol, grid_stretch)
    seeded_stretched(o)
    rows = o.run(iterations)
    out = dict(S.state_of(o), rows=rows, iters=tuple(o.iters), exits=tuple(o.exits), cg_iters=tuple(o.cg_iters),
               cg_caps=int(o.cg_caps))
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


_cached_run = functools.lru_cache(maxsize=None)(_run)


def errors(rows, st, ref):
    """What a capped test holds to ``TOL``: the four fields relative to their largest entry, the record columns REC_COLS."""
    errs = {k: rel(st[k], ref[k]) for k in K.FIELDS}
    errs["rows"] = rows_rel(rows[:, K.REC_COLS], ref["rows"][:, K.REC_COLS])
    return errs


def away(st, mutant):
    """How far a result is from a mutant of the restatement: the largest of the four fields' distances."""
    return max(rel(st[k], mutant[k]) for k in K.FIELDS)


def hold_capped(what, rows, st, ref, mutants):
    """The comparison of every capped test: ``rows`` and the fields ``st`` within ``TOL`` of the restatement ``ref``, and
    farther than ``TOL`` from each of its ``mutants``.  Prints the largest error and each mutant's distance over ``TOL``."""
    assert rows.shape == ref["rows"].shape and np.all(np.isfinite(rows)), what
    errs = errors(rows, st, ref)
    far = {w: away(st, m) for w, m in mutants.items()}
    print(f"{what}: error / tolerance {max(errs.values()) / TOL:.2e} ({max(errs, key=errs.get)}), mutants / tolerance "
          f"{ {w: float(f'{a / TOL:.2e}') for w, a in far.items()} }")
    for k, e in errs.items():
        assert e <= TOL, (what, k, e)
    assert mutants, what
    for w, a in far.items():
        assert a > TOL, (what, w, a)


def solver_kwargs(chain, nx, ny, grid_stretch=BETA, **kw):
    """The FVSolver arguments of the seeded runs."""
    return K.solver_kwargs(nx, ny, grid_stretch=grid_stretch, **dict(CHIP_MODE[chain], **kw))


# ---------------------------------------------------------------------------------------------- d. the stop test's norms
THRESHOLD_SHAPE = (272, 260)
THRESHOLD_K, THRESHOLD_MARGIN = K.THRESHOLD_K, K.THRESHOLD_MARGIN


@functools.lru_cache(maxsize=None)
def threshold_case(chain, nx, ny):
    """``fv_krylov_probe.threshold_case`` of ``chain``'s first pressure solve from the stretched seed."""
    o = _state(chain, nx, ny, THRESHOLD_K, None, "none", 1e-12, 1e-300, BETA)
    seeded_stretched(o)
    return K.threshold_of(o)


def threshold_count(chain, nx, ny, which, lost="none", linear_solver_tol=1e-12):
    tol = threshold_case(chain, nx, ny)["tol_" + which]
    return capped_reference(chain, nx, ny, None, None, lost, linear_solver_tol, 1, tol)["cg_iters"][0]


# ---------------------------------------------------------------------------------------------- e. edge shapes from rest
# (nx, ny, beta, geometry and lid, K, scheme): Re 400, both tolerances tight, the chain's own CG (``shape_reference``'s rule)
EDGES = [S.SHAPES[0] + ("TVD",),                                            # 37 x 50, beta 1, Lx 2, Ly 0.5, lid 2
         S.COUNTS + ("TVD",),                                               # 24 x 40, beta 2.5
         (131, 77, 1.5, (("corner_treatment", "smoothing"),), 6, "TVD"),
         (1024, 72, 1.5, (), 3, "TVD"),
         (40, 24, 1.5, (), 6, "Upwind")]
EDGE_IDS = [f"{nx}x{ny}-beta{beta}-{scheme}" for nx, ny, beta, _, _, scheme in EDGES]
COUNTS_EDGE = EDGES[1]


def edge_solver_kwargs(edge, chain):
    nx, ny, beta, geo, K_, scheme = edge
    kw = S.shape_solver_kwargs(nx, ny, beta, geo, K_, "reference")
    return dict({k: v for k, v in kw.items() if k not in S.REF}, convection_scheme=scheme, **CHIP_MODE[chain])


@functools.lru_cache(maxsize=None)
def edge_reference(edge, chain):
    nx, ny, beta, geo, K_, scheme = edge
    if scheme == "TVD" and edge[:5] in S.SHAPES:
        return S.shape_reference(*edge[:5], chain)                           # (shared with the one-CU file's cache)
    return S._trajectory(chain, nx, ny, S.SHAPE_RE, K_, convection_scheme=scheme, grid_stretch=beta, pressure_solver="cg",
                         **S.SHAPE_TOL, **dict(geo))


# ---------------------------------------------------------------------------------------------- f. the NaN latch
NAN_AT = S.NAN_AT                       # the restatements are the one-CU file's: reference 11, consistent 10 (rows from 0)
NAN_CHUNK = 32                          # check_every: behind the latch the launches of a chunk are empty but not free


def nan_solver_kwargs(chain):
    kw = S.nan_solver_kwargs("reference", check_every=NAN_CHUNK)
    return dict({k: v for k, v in kw.items() if k not in S.REF}, **CHIP_MODE[chain])


# ---------------------------------------------------------------------------------------------- g. loose linear solves
def loose_solver_kwargs(chain):
    kw = S.small_solver_kwargs("reference", case=S.LOOSE, linear_solver_tol=S.LOOSE["linear_solver_tol"],
                               pressure_tol=S.LOOSE["pressure_tol"])
    return dict({k: v for k, v in kw.items() if k not in S.REF}, **CHIP_MODE[chain])
