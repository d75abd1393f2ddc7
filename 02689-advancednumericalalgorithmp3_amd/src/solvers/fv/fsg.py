"""Coarse-to-fine grid sequencing of the finite-volume solver: converge on n // 2 (and coarser), prolong, converge on n.

The counterpart of ``solvers.spectral.fsg`` for ``solver=fv`` (conf/solver/fv/fsg.yaml).  Every level is an ordinary
``FVSolver`` -- the fine trial's parameters at the level's own nx and ny, so its lid profile is that of its own mesh --
solved by the same ``_begin`` / ``_advance`` loop as a lone trial; the coarsest level starts from rest, every other from
the prolongation of the level below (``transfer.prolong``: ``ldc_fv_prolong_enqueue``, one work-group per pair, the state
never leaves the device).  ``start_from`` is the same transfer from ANY other FV trial of the device, whatever its grid
and parameters: continuation in Re is ``start_from`` at equal size.  With ``grid="tanh"`` the trial needs
``transfer="tables"``: every level is then a stretched ``FVSolver`` of the same stretch, pressure equation and preconditioner
at its own size, and the transfer between them reads both grids from tables (``ldc_fv_prolong_tables_enqueue``).
With ``mapping="chip"`` and ``chip_transfer="tables"`` every level is a chip trial with the fine trial's parameters (on
``grid="tanh"`` with ``chip_grid="tables"``: its stretch, pressure equation and ``chip_preconditioner``) and the transfer is
``ldc_fv_wide_prolong_tables_enqueue``, two launches over the whole chip per level: no level needs a one-CU handle, so a
sequence may end at 1024 cells per axis, on either grid.

Sequencing is a capability, not a promised saving: the reference's stop rule (relative change per iteration) is bound
by the asymptotic rate, so the fine level may take as many iterations from the prolonged state as from rest (DESIGN.md
section 7; tools/fv_fsg_perf.py measures it).
"""
from __future__ import annotations

import dataclasses
import logging
import time

from ..datastructures import FVFSGParameters, FVParameters
from . import ldc_fv_lib as F
from .solver import FVSolver, prolong

log = logging.getLogger(__name__)

_LEVEL_FIELDS = tuple(f.name for f in dataclasses.fields(FVParameters))


def hierarchy_sizes(nx: int, ny: int, n_levels: int, coarsest_n: int) -> list:
    """(nx, ny) of the levels, coarse -> fine: nx and ny are halved together (n // 2) while both stay >= coarsest_n and
    >= LDC_FV_MIN_N, at most ``n_levels`` levels."""
    sizes = [(int(nx), int(ny))]
    floor = max(int(coarsest_n), F.MIN_N)
    while len(sizes) < int(n_levels):
        cx, cy = sizes[-1][0] // 2, sizes[-1][1] // 2
        if cx < floor or cy < floor:
            break
        sizes.append((cx, cy))
    return sizes[::-1]


def level_tolerance(tolerance: float, factor: float, levels_above: int) -> float:
    return float(tolerance) * float(factor) ** int(levels_above)


def run_level(lvl: FVSolver, tolerance: float, max_iter: int):
    """One coarse level to its latch or the cap, chunk by chunk as ``LidDrivenCavitySolver.solve`` runs a trial (a NaN
    raises there as it does here); no history, no metrics: only its state goes on.  Returns (latch, iterations)."""
    chunk = max(1, int(lvl.params.check_every))
    lvl._begin(tolerance)
    done, total = 0, 0
    while total < max_iter and not done:
        _, done, total_new = lvl._advance(min(chunk, max_iter - total))
        if total_new == total:
            raise RuntimeError("device loop made no progress")
        total = total_new
    return done, total


class FVFSGSolver(FVSolver):
    """``FVSolver`` whose ``solve()`` runs the level hierarchy of ``hierarchy_sizes`` coarse -> fine.

    ``history``, ``metrics`` and ``fields`` are the FINE level's, filled as a lone solve fills them, and
    ``metrics.iterations`` is the fine level's count; ``level_iterations`` lists the counts of all levels, coarse ->
    fine.  ``metrics.wall_time_seconds`` is the time of the whole sequence."""

    Parameters = FVFSGParameters
    _needs_cu_handle = "an FSG level"         # every level is prolonged through its one-CU handle (not with chip_transfer="tables")

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        p = self.params
        if int(p.n_levels) < 1:
            raise ValueError(f"n_levels={p.n_levels}: at least 1")
        if not float(p.coarse_tolerance_factor) > 0:
            raise ValueError(f"coarse_tolerance_factor={p.coarse_tolerance_factor}: a positive factor")
        self.level_iterations = []
        self._started = False                     # start_from() has put a state into this trial: the next solve is the fine level alone

    def level_sizes(self) -> list:
        """The levels the next ``solve()`` runs, coarse -> fine."""
        p = self.params
        if self._started:
            return [(self.nx, self.ny)]
        return hierarchy_sizes(self.nx, self.ny, p.n_levels, p.coarsest_n)

    def make_level(self, nx: int, ny: int) -> FVSolver:
        """An ordinary FVSolver with this trial's parameters at its own nx and ny, at rest."""
        kw = {k: getattr(self.params, k) for k in _LEVEL_FIELDS}
        kw.update(nx=int(nx), ny=int(ny))
        return FVSolver(**kw)

    def start_from(self, other: FVSolver):
        """This trial's state from ``other``'s (any FV trial of the same device and the same domain Lx, Ly; its grid and its other
        parameters may differ) by one prolongation; the next ``solve()`` then runs the fine level only."""
        prolong([(other, self)])
        self._started = True

    def solve(self, tolerance: float = None, max_iter: int = None):
        p = self.params
        tolerance = p.tolerance if tolerance is None else tolerance
        max_iter = p.max_iterations if max_iter is None else max_iter
        sizes = self.level_sizes()
        t0 = time.perf_counter()
        self.level_iterations = []
        below = None
        try:
            for idx, (nx, ny) in enumerate(sizes[:-1]):
                lvl = self.make_level(nx, ny)
                if below is not None:
                    prolong([(below, lvl)])
                    below.close()
                below = lvl
                tol = level_tolerance(tolerance, p.coarse_tolerance_factor, len(sizes) - 1 - idx)
                _, its = run_level(lvl, tol, max_iter)        # (a NaN raises: the solve ends as a lone NaN does)
                self.level_iterations.append(int(its))
            if below is not None:
                prolong([(below, self)])
        finally:
            if below is not None:
                below.close()
        self._started = False
        super().solve(tolerance, max_iter)
        self.level_iterations.append(int(self.metrics.iterations))
        self.metrics.wall_time_seconds = float(time.perf_counter() - t0)
        log.info("FV sequence %s: iterations per level %s, converged=%s, %.2f s",
                 " -> ".join(f"{a}x{b}" for a, b in sizes), self.level_iterations, self.metrics.converged,
                 self.metrics.wall_time_seconds)
