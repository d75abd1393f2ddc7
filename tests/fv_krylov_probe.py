"""Krylov iterates accepted at a low cap, as a probe of the sums behind every dot product (test helper, NumPy only; no test in
it).  Cases and references of tests/test_fv_krylov_probe_cpu.py and tests/test_gpu_fv_krylov_caps.py.

A CG or BiCGSTAB solve that converges hides a wrong dot product: it converges to the same x by its own stop test.  An iterate
accepted after 1, 2 or 3 iterations has not converged and is a direct function of alpha, beta and omega, so a sum that lacks a
work-group's share moves u, p and mdot by 1e-4 ... 1e-6, where the rounding of the inputs moves them by 1e-11.  The chip and
shared mappings (csrc/ldc_fv_wide.hip, csrc/ldc_fv_wide_pressure.inc) sum per-work-group slots one launch later
(``wide_slot_put`` / ``wide_slot_sum``); the one-CU mapping (csrc/ldc_fv_kernel.inc, csrc/ldc_fv_cu_pressure.hip) sums inside
its work-group.  Everything here is the restatement (tests/fv_numpy.py, tests/fv_consistent_numpy.py) run from one seeded,
developed state; the mutants are test doubles of the RESTATEMENT, never of a kernel.

``rr`` and ``bb`` of CG and the three norms of BiCGSTAB (``bicg_rr``, ``bicg_ss``, ``bicg_bb``) enter only a stop test.  They
cannot show in an iterate accepted at a cap (the cap ends the loop whatever they say); ``STOP_ONLY`` names them and the CPU test
asserts that they leave a capped run unchanged bit for bit.  Nor do they show in the counts of a run converged to 1e-13: a
share of 1/256 moves |r| by 1e-4 or less, and the counts do not move (measured in the CPU test).  For CG they are caught by the
threshold cases at the end of this file: pressure_tol set just beside |r_5| / |b|, so that the whole sum stops at iteration 5
and the sum without a share does not, or the other way round.  The three BiCGSTAB norms have no such case; what holds them is
that every run here counts exactly the restatement's BiCGSTAB iterations.
"""
from __future__ import annotations

import functools

import numpy as np

from fv_consistent_numpy import FVConsistentState
from fv_numpy import FVState

# ---------------------------------------------------------------------------------------------- the cases
# chip and shared mappings: 8 work-groups; 11, one axis above 256; 32, thin the other way; 277 chunks of 256 cells on 256
# work-groups (21 take a second stride); 288 chunks, north and south neighbours four work-groups away; 16 strides
CHIP_SHAPES = [(37, 50), (300, 9), (8, 1024), (272, 260), (1024, 72), (1024, 1024)]
CU_SHAPES = [(37, 50), (9, 250), (256, 8), (255, 253), (256, 256)]        # the edge shapes of tests/test_gpu_fv_edges.py
CG_CAPS = (1, 3)                        # pressure_max_iters of the CG-capped runs
BICG_CAP = 2                            # max_lin_iters of the BiCGSTAB-capped runs
K = 2                                   # SIMPLE iterations: the second starts from the mapping's own mdot
RE = 400.0
SETTINGS = dict(convection_scheme="TVD", alpha_uv=0.4, alpha_p=0.2, linear_solver_tol=1e-12)
PRESSURE_TOL = 1e-13
UNCAPPED = 200                          # pressure_max_iters of a run whose CG is not capped (the solver's default)

TOL = 1e-9                              # what the GPU tests ask of fields and record rows
SENSITIVITY_BOUND = 1e-10               # restatement at linear_solver_tol 1e-13 against 1e-12: at most this
MUTANT_BOUND = 1e-7                     # a lost share moves a field by at least this
REC_COLS = [0, 1, 2, 4, 5, 6]           # (column 3, |div mdot|, is rounding where the CG converges; column 7 is unused)
FIELDS = ("u", "v", "p", "mdot")

CG_MUTANTS = ("rz", "pq", "rr", "bb")
BICG_MUTANTS = ("bicg_rho", "bicg_rv", "bicg_ts", "bicg_tt", "bicg_rr", "bicg_ss", "bicg_bb")
STOP_ONLY = ("rr", "bb", "bicg_rr", "bicg_ss", "bicg_bb")

COUNT_K = 3                             # SIMPLE iterations of the converged (uncapped) runs
CHIP_COUNT_SHAPES = [(37, 50), (272, 260), (1024, 72)]
CU_COUNT_SHAPES = [(37, 50), (255, 253)]


def cg_cases(shapes):
    """(nx, ny, cap) of the CG-capped runs over ``shapes``."""
    return [(nx, ny, cap) for nx, ny in shapes for cap in CG_CAPS]


def bicg_shapes(shapes, mode):
    """The shapes of the BiCGSTAB-capped runs: the reference equation solves its pressure correction by four dense products
    per axis pair, which the chip mapping tests up to 1024 x 72 here."""
    return [s for s in shapes if mode != "reference" or s != (1024, 1024)]


# ---------------------------------------------------------------------------------------------- the seeded state
def seed_fields(X, Y):
    """(u, v, p) of the seeded state at the cell centres X, Y in [0, 1] (2-D arrays); p of cell 0 is 0."""
    u = 0.5 * np.sin(np.pi * X) * np.cos(2 * np.pi * Y) + 0.1 * np.sin(3 * np.pi * X * Y)
    v = -0.4 * np.cos(np.pi * X) * np.sin(2 * np.pi * Y) + 0.1 * np.cos(2 * np.pi * (X - Y)) * np.sin(np.pi * X) * np.sin(np.pi * Y)
    p = 0.3 * np.cos(np.pi * X) * np.cos(np.pi * Y)
    return u, v, p - p.flat[0]


def seeded(o):
    """A developed, non-solenoidal state on an ``FVState`` (or a subclass): all four face fluxes take both signs.  Returns
    (u, v, p, mdot) flattened as include/ldc_fv.h lays them out, for ``FVSolver.set_state``."""
    nx, ny = o.nx, o.ny
    u, v, p = seed_fields(*np.meshgrid((np.arange(nx) + 0.5) / nx, (np.arange(ny) + 0.5) / ny))
    ux, vy = o.faces(u, v)
    fx, fy = o.rho * ux * o.dy, o.rho * vy * o.dx
    fx[:, 0] = fx[:, -1] = 0.0
    fy[0, :] = fy[-1, :] = 0.0
    mdot = np.concatenate([fx.ravel(), fy.ravel()])
    o.set_state(u.ravel(), v.ravel(), p.ravel(), mdot)
    return u.ravel().copy(), v.ravel().copy(), p.ravel().copy(), mdot


# ---------------------------------------------------------------------------------------------- the mutants
def _tail(which, name, a):
    """``a`` flattened; without its first n // 256 entries when ``name`` is the dot product that loses its share."""
    a = a.ravel()
    return a[a.size // 256:] if name == which else a


def _pcg_copy(self, wx, wy, b, which):
    """``FVConsistentState.pcg``, statement for statement, every dot product through ``_tail``."""
    bn = np.linalg.norm(_tail(which, "bb", b))
    x = np.zeros_like(b)
    if bn == 0:
        return x, 0, False
    r = b.copy()
    p = rz_prev = None
    for k in range(self.pressure_max_iters):
        if np.linalg.norm(_tail(which, "rr", r)) <= self.pressure_tol * bn:
            return x, k, False
        z = self.precondition(r)
        rz = float(np.sum(_tail(which, "rz", r * z)))
        p = z if k == 0 else z + (rz / rz_prev) * p
        q = self.apply(wx, wy, p)
        alpha = rz / float(np.sum(_tail(which, "pq", p * q)))
        x = x + alpha * p
        r = r - alpha * q
        rz_prev = rz
    return x, self.pressure_max_iters, bool(np.linalg.norm(_tail(which, "rr", r)) > self.pressure_tol * bn)


def _bicgstab_copy(self, d, diagP, b, which, maxiter=None):
    """``FVState.bicgstab``, statement for statement, every dot product through ``_tail``."""
    maxiter = self.max_lin_iters if maxiter is None else maxiter
    bn = np.linalg.norm(_tail(which, "bicg_bb", b))
    if bn == 0:
        self.iters.append(0)
        self.exits.append("b0")
        return np.zeros_like(b)
    atol = self.tol * bn
    x = np.zeros_like(b)
    r = b.copy()
    rt = r.copy()
    rhotol = np.finfo(float).eps ** 2
    rho_prev = omega = alpha = None
    p = v = None
    it = 0
    why = "cap"
    for it in range(maxiter):
        if np.linalg.norm(_tail(which, "bicg_rr", r)) < atol:
            why = "r"
            break
        rho = np.vdot(_tail(which, "bicg_rho", rt), _tail(which, "bicg_rho", r))
        if abs(rho) < rhotol:
            why = "rho"
            break
        if it > 0:
            if abs(omega) < rhotol:
                why = "omega"
                break
            beta = (rho / rho_prev) * (alpha / omega)
            p = r + beta * (p - omega * v)
        else:
            p = r.copy()
        phat = p / diagP
        v = self.matvec(d, diagP, phat)
        rv = np.vdot(_tail(which, "bicg_rv", rt), _tail(which, "bicg_rv", v))
        if rv == 0:
            why = "rv"
            break
        alpha = rho / rv
        s = r - alpha * v
        if np.linalg.norm(_tail(which, "bicg_ss", s)) < atol:
            x = x + alpha * phat
            it += 1
            why = "s"
            break
        shat = s / diagP
        t = self.matvec(d, diagP, shat)
        omega = np.vdot(_tail(which, "bicg_ts", t), _tail(which, "bicg_ts", s)) / np.vdot(_tail(which, "bicg_tt", t),
                                                                                            _tail(which, "bicg_tt", t))
        x = x + alpha * phat + omega * shat
        r = s - omega * t
        rho_prev = rho
    else:
        it = maxiter
    self.iters.append(it)
    self.exits.append(why)
    return x


@functools.lru_cache(maxsize=None)
def lost_share(cls, which):
    """A subclass of ``cls`` (``FVState`` or ``FVConsistentState``) whose dot product ``which`` omits the first n // 256 cells:
    ``rz``, ``pq``, ``rr`` and ``bb`` (|b|) of ``pcg``; ``bicg_rho`` (rt . r), ``bicg_rv`` (rt . v), ``bicg_ts``, ``bicg_tt`` and the norms
    ``bicg_rr``, ``bicg_ss``, ``bicg_bb`` of ``bicgstab``.  ``which=None``: the copies with every sum whole, which the CPU
    test holds against the originals bit for bit."""
    if which is not None and which not in CG_MUTANTS + BICG_MUTANTS:
        raise ValueError(which)
    if which in CG_MUTANTS and not issubclass(cls, FVConsistentState):
        raise ValueError(f"{which} is a dot product of FVConsistentState.pcg")
    body = {}
    if which is None or which in BICG_MUTANTS:
        body["bicgstab"] = lambda self, d, diagP, b, maxiter=None: _bicgstab_copy(self, d, diagP, b, which, maxiter)
    if issubclass(cls, FVConsistentState) and (which is None or which in CG_MUTANTS):
        body["pcg"] = lambda self, wx, wy, b: _pcg_copy(self, wx, wy, b, which)
    return type(f"{cls.__name__}_lost_{which}", (cls,), body)


# ---------------------------------------------------------------------------------------------- the references
def _state(nx, ny, mode, cg_cap, bicg_cap, lost, linear_solver_tol, pressure_tol=PRESSURE_TOL):
    if mode not in ("consistent", "reference"):
        raise ValueError(mode)
    cls = FVConsistentState if lost == "none" else lost_share(FVConsistentState, lost)
    kw = dict(SETTINGS, linear_solver_tol=linear_solver_tol, pressure_equation=mode, pressure_solver="cg",
              pressure_tol=pressure_tol, pressure_max_iters=UNCAPPED if cg_cap is None else int(cg_cap))
    if bicg_cap is not None:
        kw["max_lin_iters"] = int(bicg_cap)
    return cls(nx, ny, RE, **kw)


CACHED_CELLS = 1 << 19                  # a 1024 x 1024 result is 40 MB and is asked for once: it is not kept


def capped_reference(nx, ny, mode, cg_cap=None, bicg_cap=None, lost="none", linear_solver_tol=1e-12, iterations=K,
                     pressure_tol=PRESSURE_TOL):
    """The restatement run ``iterations`` SIMPLE iterations from the seed, once per case (``functools.lru_cache`` below
    ``CACHED_CELLS`` cells); never changed by a caller, the arrays are read-only.  ``mode``: "consistent" or "reference" (the
    pressure equation).  ``lost``: "none" (the restatement itself), None (the copies of its loops with every sum whole) or a
    mutant's name.  A dict: u, v, p, mdot (flat), rows, iters, exits, cg_iters, cg_caps."""
    run = _cached_run if nx * ny <= CACHED_CELLS else _run
    return run(nx, ny, mode, cg_cap, bicg_cap, lost, linear_solver_tol, iterations, pressure_tol)


def _run(nx, ny, mode, cg_cap, bicg_cap, lost, linear_solver_tol, iterations, pressure_tol):
    o = _state(nx, ny, mode, cg_cap, bicg_cap, lost, linear_solver_tol, pressure_tol)
    seeded(o)
    rows = o.run(iterations)
    out = dict(u=o.u.ravel().copy(), v=o.v.ravel().copy(), p=o.p.ravel().copy(),
               mdot=np.concatenate([o.fx.ravel(), o.fy.ravel()]), rows=rows, iters=tuple(o.iters), exits=tuple(o.exits),
               cg_iters=tuple(o.cg_iters), cg_caps=int(o.cg_caps))
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


_cached_run = functools.lru_cache(maxsize=None)(_run)


def converged_reference(nx, ny, linear_solver_tol=1e-12):
    """The uncapped consistent run of the count tests: COUNT_K iterations from the seed, pressure_tol 1e-13."""
    return capped_reference(nx, ny, "consistent", None, None, "none", linear_solver_tol, COUNT_K)


def counts_sensitivity(nx, ny):
    """max over the solves of |CG count at linear_solver_tol 1e-13 - count at 1e-12| of the restatement's converged run
    (as tests/fv_stretched_probe.py::counts_sensitivity)."""
    tight, ref = converged_reference(nx, ny, 1e-13), converged_reference(nx, ny)
    assert tight["cg_caps"] == ref["cg_caps"] == 0 and len(ref["cg_iters"]) == COUNT_K
    return max(abs(a - b) for a, b in zip(tight["cg_iters"], ref["cg_iters"]))


def count_bound(nx, ny):
    """What the device's per-solve CG count may differ by: one (a stop test at the threshold) or ten times the restatement's own
    sensitivity, whichever is larger."""
    return max(1, 10 * counts_sensitivity(nx, ny))


# ---------------------------------------------------------------------------------------------- the stop test at a threshold
THRESHOLD_K = 5                         # the CG iteration beside whose residual pressure_tol is set
THRESHOLD_MARGIN = 1e-6                 # the least distance of pressure_tol from |r_5| / |b|, relative: a thousand times the
#                                         1e-9 to which the device's fields follow the restatement


@functools.lru_cache(maxsize=None)
def threshold_case(nx, ny):
    """The first pressure solve from the seed after THRESHOLD_K iterations: rho = |r_K| / |b| (r_K = b - A x_K), the fractions
    ``d_rr`` and ``d_bb`` by which |r_K| and |b| shrink without their first n // 256 entries, and two settings of pressure_tol:

    ``tol_bb`` = rho (1 + d_bb / 2): the whole sums stop at iteration K; |b| without its share makes the threshold smaller than
    |r_K|, and that solve goes on.  ``tol_rr`` = rho (1 - d_rr / 2): the whole sums go on at iteration K; |r_K| without its share
    is below the threshold, and that solve stops at K."""
    o = _state(nx, ny, "consistent", THRESHOLD_K, None, "none", 1e-12, 1e-300)
    seeded(o)
    return threshold_of(o)


def threshold_of(o):
    """``threshold_case`` of a seeded restatement whose CG is capped at THRESHOLD_K with a pressure_tol it cannot meet."""
    o.step()
    b = o.last["b"].ravel()
    r = (o.last["b"] - o.apply(o.last["wx"], o.last["wy"], o.last["x"])).ravel()
    lo = r.size // 256
    rho = float(np.linalg.norm(r) / np.linalg.norm(b))
    d_rr = float(1.0 - np.linalg.norm(r[lo:]) / np.linalg.norm(r))
    d_bb = float(1.0 - np.linalg.norm(b[lo:]) / np.linalg.norm(b))
    return dict(rho=rho, d_rr=d_rr, d_bb=d_bb, tol_bb=rho * (1.0 + 0.5 * d_bb), tol_rr=rho * (1.0 - 0.5 * d_rr))


def threshold_count(nx, ny, which, lost="none", linear_solver_tol=1e-12):
    """The CG count of the first pressure solve from the seed with pressure_tol = ``threshold_case(nx, ny)["tol_" + which]``
    (``which``: "rr" or "bb"), for the restatement (``lost="none"``) or its mutant ``lost``."""
    tol = threshold_case(nx, ny)["tol_" + which]
    return capped_reference(nx, ny, "consistent", None, None, lost, linear_solver_tol, 1, tol)["cg_iters"][0]


# ---------------------------------------------------------------------------------------------- distances
def rel(a, b):
    """The largest deviation relative to the reference field's largest entry."""
    return float(np.max(np.abs(np.asarray(a) - b)) / max(float(np.max(np.abs(b))), 1e-300))


def rows_rel(got, ref):
    den = np.where(ref == 0.0, 1.0, np.abs(ref))
    return float(np.max(np.abs(got - ref) / den))


def distance(a, b):
    """{field: rel} of two results (dicts with u, v, p, mdot), relative to ``b``."""
    return {k: rel(a[k], b[k]) for k in FIELDS}


def tables(shapes=((37, 50), (272, 260), (1024, 72), (1024, 1024))):
    """The two CPU tables of profiles/fv_krylov_caps.md as markdown lines (``python tests/fv_krylov_probe.py``): what the ``rz``
    mutant does to a converged run (counts, fields) and to a run accepted at a cap, beside the restatement's own sensitivity."""
    out = ["| cells | SIMPLE iterations | CG counts, ok | CG counts, rz mutant | largest relative change of u, v, p, mdot |",
           "|---|---|---|---|---|"]
    for nx, ny in CHIP_COUNT_SHAPES:
        ok = converged_reference(nx, ny)
        mu = capped_reference(nx, ny, "consistent", None, None, "rz", 1e-12, COUNT_K)
        out.append(f"| {nx} x {ny} | {COUNT_K} | {' '.join(map(str, ok['cg_iters']))} | {' '.join(map(str, mu['cg_iters']))} | "
                   f"{max(distance(mu, ok).values()):.0e} |")
    out += ["", "| cells | cap | rz mutant vs ok | pq mutant vs ok | restatement at linear_solver_tol 1e-13 vs 1e-12 |",
            "|---|---|---|---|---|"]
    for nx, ny in shapes:
        cells = []
        for cap in CG_CAPS:
            ok = capped_reference(nx, ny, "consistent", cap)
            cells.append([max(distance(capped_reference(nx, ny, "consistent", cap, None, w), ok).values()) for w in ("rz", "pq")]
                         + [max(distance(capped_reference(nx, ny, "consistent", cap, None, "none", 1e-13), ok).values())])
        out.append(f"| {nx} x {ny} | {' / '.join(map(str, CG_CAPS))} | "
                   + " | ".join(" / ".join(f"{c[k]:.1e}" for c in cells) for k in range(3)) + " |")
    return out


def solver_kwargs(nx, ny, **kw):
    """The FVSolver arguments of the seeded runs (two or three ``_advance(1)`` calls)."""
    return dict(dict(name="fv", Re=RE, nx=nx, ny=ny, **SETTINGS, pressure_tol=PRESSURE_TOL, tolerance=1e-30,
                     max_iterations=10**6, check_every=8), **kw)


if __name__ == "__main__":
    print("\n".join(tables()))
