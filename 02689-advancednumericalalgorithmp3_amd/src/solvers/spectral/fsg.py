"""Full-single-grid (FSG) sequence on MI355X: converge on N/2 (and coarser), prolong, converge on N.

Plugin surface: ``solvers.spectral.fsg.FSGSolver`` as in conf/solver/spectral/fsg.yaml:7 (reference
src/solvers/spectral/fsg.py:19-129; driver ``solve_fsg`` multigrid/fsg.py:1053-1221, hierarchy :489-543,
prolongation :551-614, smoother :745-995).  Every level is the same fused RK-stage kernel as SGSolver,
run in *smoother* mode: each stage differentiates its own stage pressure (the reference smoother passes
``p_in`` through, unlike SGSolver -- quirk Q1), no warm-up, NaN/Inf exit.  Prolongation = two NT products
with a precomputed matrix on the GPU; the axis-swapped boundary re-imposition of the reference (quirk Q2)
is reproduced because it changes the first fine-level stage.
"""
from __future__ import annotations

import dataclasses
import logging
import time

import numpy as np

from .chunks import run_to_tolerance
from .operators.transfer_operators import prolongation_matrix
from .sg import SGSolver, refine_vortices_together
from ..base import EN, PN, REL, RP, RU, RV, ZN

log = logging.getLogger(__name__)

COARSEST_N = 12           # multigrid/fsg.py:496


def hierarchy_orders(n_fine: int, n_levels: int, coarsest_n: int = COARSEST_N) -> list:
    """Polynomial orders coarse -> fine: halve while the next order stays >= coarsest_n."""
    orders, n = [], n_fine
    for _ in range(n_levels):
        orders.append(n)
        if n // 2 < coarsest_n:
            break
        n //= 2
    return orders[::-1]


class FSGSolver(SGSolver):
    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        if self.params.initial_guess != "rest":      # (with multigrid="fsg" in the parameters SGSolver has refused already)
            raise ValueError(f"initial_guess={self.params.initial_guess!r} with multigrid='fsg' (FSGSolver): the sequence "
                             f"starts on its coarsest level, which takes no finite-volume seed yet")
        if self.params.nx != self.params.ny:
            # the reference builds its level hierarchy from ONE order (multigrid/fsg.py:490-530, n_fine = nx) and squares
            # every level; with nx != ny it has no defined behaviour to reproduce
            raise NotImplementedError("FSG needs nx == ny (the level hierarchy is built from one polynomial order)")

    def _make_level(self, n: int) -> SGSolver:
        kw = dataclasses.asdict(dataclasses.replace(self.params, nx=n, ny=n))
        lvl = SGSolver(**kw)
        lvl._smoother_mode()
        return lvl

    # ------------------------------------------------------------------ prolongation (device)
    def _prolongate(self, coarse: SGSolver, fine: SGSolver):
        import torch
        LD, Mf, Mc = fine.LD, fine.M, coarse.M
        R = (Mf + 15) // 16
        dev = fine.device
        method = self.params.prolongation_method

        def padded(a):
            out = torch.zeros((LD, LD), dtype=torch.float64, device=dev)
            out[: a.shape[0], : a.shape[1]] = torch.as_tensor(a, device=dev) if not torch.is_tensor(a) else a
            return out

        Pf = padded(prolongation_matrix(method, Mc, Mf))                 # (Mf, Mc)
        Pi = padded(prolongation_matrix(method, Mc - 2, Mf - 2))         # inner grids
        X, Y = fine.d["S0"], fine.d["S1"]

        def apply(P, src_T, n_out):
            """P src P^T for a coarse field given as its transpose (LD-padded); returns LD x LD."""
            # X[i][b] = sum_a P[i][a] src[a][b] = sum_a P[i][a] srcT[b][a]
            fine._abi("ldc_gemm_nt", P.data_ptr(), src_T.data_ptr(), X.data_ptr(), R, R, LD, 0, 0, None, None)
            # out[i][j] = sum_b X[i][b] P[j][b]
            fine._abi("ldc_gemm_nt", X.data_ptr(), P.data_ptr(), Y.data_ptr(), R, R, LD, 0, 0, None, None)
            return Y[:n_out, :n_out].clone()

        uc = padded(coarse.d["UT"][:Mc, :Mc])
        u = apply(Pf, uc, Mf)
        vc = padded(coarse.d["VT"][:Mc, :Mc])
        v = apply(Pf, vc, Mf)
        pc = padded(coarse.d["P"][1: Mc - 1, 1: Mc - 1].t().contiguous())
        p = apply(Pi, pc, Mf - 2)
        # quirk Q2 (multigrid/fsg.py:586-599): [ix, iy] arrays treated as [iy, ix]
        U0 = float(self.params.lid_velocity)
        u[0, :] = 0.0; v[0, :] = 0.0
        u[-1, :] = U0; v[-1, :] = 0.0
        u[:, 0] = 0.0; v[:, 0] = 0.0
        u[:, -1] = 0.0; v[:, -1] = 0.0
        # initialize_lid (:950-954) restores the lid column with the regularised profile
        u[:, -1] = fine.d["ulid"][:Mf]
        v[:, -1] = 0.0
        fine.set_state_device(u, v, p)

    def _finish(self, tolerance, total, converged, wall):
        """One-point histories, like the reference (fsg.py:102-124)."""
        res = self.residual_fields()
        q = self.global_quantities()
        row = np.zeros((1, 8))
        row[0, REL] = tolerance if converged else tolerance * 10
        row[0, RU], row[0, RV], row[0, RP] = (float(np.linalg.norm(res[k])) for k in ("R_u", "R_v", "R_p"))
        row[0, EN], row[0, ZN], row[0, PN] = q["E"], q["Z"], q["P"]
        self.history = row
        self._store_results(row, total, converged, wall, with_diag=True)

    # ------------------------------------------------------------------ driver
    def solve(self, tolerance: float = None, max_iter: int = None):
        tolerance = self.params.tolerance if tolerance is None else tolerance
        max_iter = self.params.max_iterations if max_iter is None else max_iter
        wall = run_ladder([self], self._run_level, [tolerance], [max_iter])
        log.info("FSG completed in %.2fs: %d iterations, converged=%s", wall, self.metrics.iterations,
                 self.metrics.converged)

    @staticmethod
    def _run_level(group, tols, caps):
        """One level of a lone FSG solve, through the level's own handle."""
        (lvl,), (tol,) = group, tols
        lvl._begin(tol)
        return run_to_tolerance(group, lambda k: [lvl._advance(k, diagnostics=False)], caps, batch=False)


def run_ladder(fines, run_level, tolerances, caps) -> float:
    """FSG solves of ``fines`` (FSGSolvers of one hierarchy, fine tolerance and iteration cap per level each), level by level
    (reference multigrid/fsg.py:1053-1221): every level runs in smoother mode to its own coarse tolerance, the coarsest from
    rest, every other from the prolongation of the level below; a trial that diverges on a level (NaN latch) stops there,
    the others go on.  ``run_level(group, tols, caps)`` advances the levels of the trials still alive and returns per-trial
    (latch, iterations, records).  Fills each trial's one-point history (_finish); returns the wall time."""
    t0 = time.perf_counter()
    p0 = fines[0].params
    orders = hierarchy_orders(p0.nx, p0.n_levels)
    log.info("Building %d-level hierarchy: N = %s", len(orders), orders)
    for s in fines:
        s._smoother_mode()
    ladders = [[s._make_level(n) for n in orders[:-1]] + [s] for s in fines]
    nlev = len(orders)
    alive = list(range(len(fines)))
    total = [0] * len(fines)
    last = [0] * len(fines)                       # latch of the last level each trial ran
    for idx in range(nlev):
        if not alive:          # every trial diverged on a coarser level: nothing goes up
            break
        group = [ladders[q][idx] for q in alive]
        for q, lvl in zip(alive, group):
            if idx == 0:
                lvl.reset_state()
            else:
                fines[q]._prolongate(ladders[q][idx - 1], lvl)
        tols = [tolerances[q] * fines[q].params.coarse_tolerance_factor ** (nlev - 1 - idx) for q in alive]
        out = run_level(group, tols, [caps[q] for q in alive])
        for q, (done, its, _) in zip(alive, out):
            total[q] += its
            last[q] = done
        log.info("FSG level %d (N=%d): %d trials, iterations %s", idx, orders[idx], len(alive), [o[1] for o in out])
        alive = [q for q, (done, _, _) in zip(alive, out) if done != 2]
    wall = time.perf_counter() - t0
    its_all = max(1, sum(total))
    refine_vortices_together(fines)       # (one call and one copy for all trials that ask for sub-grid vortex centres)
    for q, s in enumerate(fines):
        for lvl in ladders[q][:-1]:
            lvl.close()
        # a trial's wall time is its share by iteration count (BatchedSGSolver.solve)
        s._finish(tolerances[q], total[q], last[q] == 1, wall * total[q] / its_all)
    return wall
