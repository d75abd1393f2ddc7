"""Finite-volume SIMPLE solver of the lid-driven cavity on MI355X (the reference's ``solvers.fv.solver.FVSolver``).

Contract: reference src/solvers/fv/solver.py (the iteration, :170-257), base.py:202-330 (the loop and its record),
:359-450 (E, Z, P), :569-760 (streamfunction and vortex extrema).  Every SIMPLE iteration runs in the HIP kernels of
include/ldc_fv.h and the host only reads the record rows and the latch: ``advance`` is the chunk of ``mapping="cu"`` trials
(one work-group per trial, ``check_every`` iterations per launch; with ``acceleration="anderson"`` a mixing launch after
every iteration), ``FVSolver._wide_step`` and ``SharedBatch`` the chunk of ``"chip"`` and ``"shared"`` trials (one launch per
phase over the whole chip, under the retry loop of ``budget``).  ``FVSolver`` owns a trial's tensors and device handles and
attaches to them what its options ask for, in the order of ``_make_handle``; once per solve it reads the vortex metrics, on
the host with SciPy's sparse solve or from the result block of ``post.postprocess``.

The rest of the package is imported here under the names it had when it lived in this module: the option values and their
checks (``options``), the host tables and their device cache (``grids``), the retry loop (``budget``), post-processing
(``post``) and the coarse-to-fine transfer (``transfer``).
"""
from __future__ import annotations

import ctypes as C
import logging

import numpy as np

from .. import validation as _val
from ..base import LidDrivenCavitySolver
from ..datastructures import FVParameters
from . import ldc_fv_lib as F
from . import options
from .budget import (advance_batch_with_budget, advance_batch_with_budgets, advance_with_budget,  # noqa: F401
                     advance_with_budgets, advance_with_retries)
from .grids import (axis_tables, device_index, dirichlet_eig_host, generalised_eig_host, grid_axis,  # noqa: F401
                    lid_profile, lid_profile_at, mask_bounds, neumann_eig, separable_axis_host, separable_fit,
                    separable_tables, separable_tables_host, sine_eig, sine_eig_host, stretched_streamfunction_matrix,
                    tanh_vertices, transfer_axis, wall_eig, wall_eig_host, wall_stretched_axis)
from .options import (ACCELERATIONS, CHIP_GRIDS, CHIP_PRECONDITIONERS, CHIP_TRANSFERS, GRIDS, MAPPINGS,  # noqa: F401
                      PRESSURE_EQUATIONS, PRESSURE_PRECONDITIONERS, SCHEMES, STREAMFUNCTIONS, TRANSFERS, VORTEX_METRICS,
                      VORTEX_REFINES, WALL_RULES)
from .post import post_route, postprocess  # noqa: F401
from .transfer import _same_extent, prolong, prolong_route  # noqa: F401

log = logging.getLogger(__name__)

LINEAR_MAX_ITERATIONS = 1000        # scipy_solver.py:15


def advance(trials, k):
    """One chunk for lone trials and batches alike: ``k`` iterations (at most every trial's record ring) for each of
    ``trials`` (FVSolvers on one device) in ONE launch, one work-group each, then ONE copy of their ctrl words and ONE of
    the first ``k`` rows of their record rings (the slices stack whatever the rings' own lengths); per trial (rows of the
    new iterations, latch, nan, iteration count).

    With ``acceleration="anderson"`` on any of the trials the chunk is ``k`` launches of ONE iteration with the mixing
    kernel after each (``ldc_fv_anderson_enqueue``), all enqueued before the one wait; without, the launch of before.

    A work-group holds its CU for the whole chunk, so launch and wait hold the device's resident lock: not beside a
    launch whose work-groups must all be resident (a lone trial in the launcher's pool of streams, next to spectral
    batches; solvers.fv.batched)."""
    import torch
    from solvers.spectral import ldc_lib
    from solvers.spectral.chunks import _words
    dev = trials[0].device
    index = device_index(dev)
    accelerated = any(s.accelerated for s in trials)
    with torch.cuda.device(dev):
        starts = _words([s.t["ctrl"] for s in trials])[:, F.CTRL_ITER]
        with ldc_lib.resident_lock(index):
            if accelerated:     # k launches of one iteration, a mixing launch after each; plain trials ride at depth 0
                F.anderson_enqueue([s.handle for s in trials], [s._anderson_block() for s in trials], k,
                                   torch.cuda.current_stream(dev).cuda_stream)
            else:
                F.batch_enqueue([s.handle for s in trials], k, torch.cuda.current_stream(dev).cuda_stream)
            ctrl = _words([s.t["ctrl"] for s in trials])        # (synchronises the stream)
        rings = _words([s.t["rec"][:k] for s in trials])
    return [(ring[: int(c[F.CTRL_ITER] - start)].copy(), int(c[F.CTRL_DONE]), int(c[F.CTRL_NAN]), int(c[F.CTRL_ITER]))
            for start, c, ring in zip(starts, ctrl, rings)]


class SharedBatch:
    """``solvers`` (FVSolvers with ``mapping="shared"`` on one device, at most ``WIDE_BATCH_MAX``) as ONE batch object of
    the library (``ldc_fv_wide_batch_*``): every phase launch carries the work-groups of all of them, and an enqueue gives
    every trial its own quota of iterations.  The table the kernels look their work-group up in lives in a tensor of this
    object.  A lone shared trial is a batch of one."""

    def __init__(self, solvers, graph=None):
        import torch
        self.solvers = list(solvers)
        if not 1 <= len(self.solvers) <= F.WIDE_BATCH_MAX:
            raise ValueError(f"{len(self.solvers)} trials in one shared batch: 1 ... {F.WIDE_BATCH_MAX}")
        self.device = self.solvers[0].device
        self._wides = [s._wide.value for s in self.solvers]
        self.handle = None
        with torch.cuda.device(self.device):
            self.table = torch.empty(F.wide_batch_table_len([(s.nx, s.ny) for s in self.solvers]), dtype=torch.uint8,
                                     device=self.device)
            torch.cuda.current_stream(self.device).synchronize()      # (create copies the table on the library's stream)
            self.handle = F.wide_batch_create(self._wides, self.table.data_ptr(), self.table.numel())
        if graph is not None:
            self.set_graph(graph)

    def set_graph(self, on: bool):
        F.check(F.lib().ldc_fv_wide_batch_set_graph(self.handle, int(bool(on))), "ldc_fv_wide_batch_set_graph")

    def close(self):
        if self.handle is not None:
            F.lib().ldc_fv_wide_batch_destroy(self.handle)
            self.handle = None

    def _step(self, quotas, budget, pressure_budget=None):
        """ONE enqueue and ONE wait, then one copy each of the control words, the overflow words and the new record rows
        (the step of ``budget.advance_with_retries``, with one budget or two)."""
        import torch
        from solvers.spectral import ldc_lib
        from solvers.spectral.chunks import _words
        dev, ss = self.device, self.solvers
        index = device_index(dev)
        with torch.cuda.device(dev):
            if pressure_budget is not None:
                F.check(F.lib().ldc_fv_wide_batch_set_pressure_budget(self.handle, int(pressure_budget)),
                        "ldc_fv_wide_batch_set_pressure_budget")
            with ldc_lib.resident_lock(index):
                F.wide_batch_enqueue(self.handle, quotas, budget, torch.cuda.current_stream(dev).cuda_stream)
                ctrl = _words([s.t["ctrl"] for s in ss])          # (synchronises the stream)
            overflow = _words([s.t["scratch"][:1].view(torch.int64) for s in ss])[:, 0]
            new = [int(c[F.CTRL_ITER]) - t for c, t in zip(ctrl, self._totals)]
            got = [s.t["rec"][:m] for s, m in zip(ss, new) if m > 0]
            rows = torch.cat(got).cpu().numpy() if got else np.zeros((0, F.REC_LEN))
        out, lo = [], 0
        for q, (c, m) in enumerate(zip(ctrl, new)):
            out.append((rows[lo: lo + m].copy(), int(c[F.CTRL_DONE]), int(c[F.CTRL_NAN]), int(c[F.CTRL_ITER]),
                        int(overflow[q])))
            lo += max(m, 0)
            self._totals[q] = int(c[F.CTRL_ITER])
        return out

    def advance(self, ks):
        """``ks[q]`` iterations of trial q (0: left alone; at most its record ring), all in the same launches, whatever
        budgets they need; per trial (rows of the new iterations, latch, nan, iteration count).  Every trial's
        ``linear_budget`` and ``linear_budget_retries`` go on as a lone trial's do."""
        import torch
        from solvers.spectral.chunks import _words
        ss = self.solvers
        if [s._wide.value if s._wide is not None else None for s in ss] != self._wides:
            raise RuntimeError("a trial of a shared batch has a new device handle: the batch's table is out of date")
        with torch.cuda.device(self.device):
            self._totals = [int(t) for t in _words([s.t["ctrl"] for s in ss])[:, F.CTRL_ITER]]
        # two budgets for all when any trial has the consistent equation (ldc_fv_wide_batch_create has seen to it that
        # those share pressure_max_iters), else one
        caps = next((s for s in ss if s.consistent), ss[0])._budget_caps()
        out = advance_with_retries(self._step, list(self._totals), [int(k) for k in ks],
                                   [(s.linear_budget, s.pressure_budget)[:len(caps)] for s in ss], caps)
        for s, (_, _, _, _, budgets, retries) in zip(ss, out):
            s._keep_budgets(budgets, retries)
        return [(rows, latch, nan, total) for rows, latch, nan, total, _, _ in out]


class FVSolver(LidDrivenCavitySolver):
    """Collocated finite-volume SIMPLE solver; ``nx`` x ``ny`` cells (8 ... 256 each with ``mapping="cu"``, one
    work-group per trial; 8 ... 1024 with ``mapping="chip"``, one launch per phase over the whole chip, and with
    ``mapping="shared"``, the same launches shared by all trials of a batch).  ``streamfunction()``, ``vorticity()``,
    ``vortex_metrics="chip"``, ``prolong`` and ``start_from`` take a chip or shared trial of any of these sizes; a chip trial
    on a stretched mesh (``chip_grid="tables"``) starts from another trial with ``chip_transfer="tables"``."""

    Parameters = FVParameters
    rho = 1.0
    _needs_cu_handle = None                   # (a subclass that cannot do without the one-CU handle names itself here)

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        p = self.params
        # accelerated, mixed_chip, consistent, consistent_cu, transfer_tables, chip_transfer_tables, stretched, chip_tables,
        # stretched_wall, separable, chip_separable, shared, chip, _has_cu_handle: what advance, postprocess and prolong route on
        vars(self).update(vars(options.check(p, self._needs_cu_handle)))
        self.vortex_refine_status = None         # per (primary, BR, BL, TL) after a refined compute_vortex_metrics()
        nx, ny = int(p.nx), int(p.ny)
        self.nx, self.ny, self.n_cells = nx, ny, nx * ny
        self.dx_min, self.dy_min = p.Lx / nx, p.Ly / ny
        self.shape_full = (ny, nx)               # as the reference's FV solver: cells c = j*nx + i
        self.mu = self.rho * p.lid_velocity * p.Lx / p.Re
        xc, yc = (np.arange(nx) + 0.5) * self.dx_min, (np.arange(ny) + 0.5) * self.dy_min
        if self.stretched:                       # (dx_min, dy_min stay the mean widths: the kernel does not read them)
            beta = float(p.grid_stretch)
            self._xv, self._yv = tanh_vertices(nx, p.Lx, beta), tanh_vertices(ny, p.Ly, beta)
            xc, self._hx, self._dxf, self._gxf = axis_tables(self._xv)
            yc, self._hy, self._dyf, self._gyf = axis_tables(self._yv)
        X, Y = np.meshgrid(xc, yc)
        self._init_fields(x=X.ravel(), y=Y.ravel())
        self._mask_bounds = mask_bounds(np.sort(np.unique(self.fields.x)), np.sort(np.unique(self.fields.y)))
        self._post = None                        # the trial's result block of the last postprocess()

        import torch
        from solvers.spectral import ldc_lib
        self.device = torch.device(p.device)
        ldc_lib.require_device(self.device)      # no GPU / not gfx950 -> LdcError: there is no CPU fallback
        L = F.lib()
        if L.ldc_fv_version() != F.VERSION:
            raise ldc_lib.LdcError(f"ldc_fv ABI {L.ldc_fv_version()} != {F.VERSION}: rebuild the library")
        f64 = dict(dtype=torch.float64, device=self.device)
        self.rec_cap = max(1, int(p.check_every))
        if self.stretched:                       # shared per (n, L, beta, device); the lid at the stretched face centres
            gridx, lamx, Qx = grid_axis(nx, p.Lx, float(p.grid_stretch), self.device, self.rho)
            gridy, lamy, Qy = grid_axis(ny, p.Ly, float(p.grid_stretch), self.device, self.rho)
            ulid = lid_profile_at(xc, p.Lx, p.lid_velocity, p.corner_treatment, p.corner_smoothing)
            ops = dict(Qx=Qx, lamx=lamx, Qy=Qy, lamy=lamy, gridx=gridx, gridy=gridy)
            if self.separable or self.chip_separable:     # shared per (nx, ny, Lx, Ly, beta, rho, device): the fit couples the axes
                ops["precx"], ops["precy"] = separable_tables(nx, ny, p.Lx, p.Ly, float(p.grid_stretch), self.device,
                                                              self.rho)
        else:
            lamx, Qx = neumann_eig(nx)
            lamy, Qy = neumann_eig(ny)
            ulid = lid_profile(nx, p.Lx, p.lid_velocity, p.corner_treatment, p.corner_smoothing)
            ops = dict(Qx=torch.tensor(Qx, **f64).contiguous(), lamx=torch.tensor(lamx, **f64),
                       Qy=torch.tensor(Qy, **f64).contiguous(), lamy=torch.tensor(lamy, **f64))
        self._ulid_host = np.asarray(ulid, dtype=np.float64)
        self.t = dict(
            ulid=torch.tensor(ulid, **f64), **ops,
            u=torch.zeros(nx * ny, **f64), v=torch.zeros(nx * ny, **f64), p=torch.zeros(nx * ny, **f64),
            mdot=torch.zeros(F.faces(nx, ny), **f64), work=torch.zeros(F.work_len(nx, ny), **f64),
            rec=torch.zeros((self.rec_cap, F.REC_LEN), **f64),
            ctrl=torch.zeros(F.CTRL_LEN, dtype=torch.int64, device=self.device),
            # the mixing kernel's words: every trial has them (a plain trial rides in an accelerated call at depth 0)
            astate=torch.zeros(F.ANDERSON_STATE_LEN, dtype=torch.int64, device=self.device))
        if self.accelerated or self.mixed_chip:
            self.t["hist"] = torch.zeros(F.anderson_hist_len(nx, ny, int(p.anderson_depth)), **f64)
        if self.mixed_chip:
            self.t["mix_scratch"] = torch.zeros(F.wide_anderson_scratch_len(nx, ny, int(p.anderson_depth)), **f64)
        if self.chip:
            self.t["scratch"] = torch.zeros(F.wide_scratch_len(nx, ny), **f64)
        if self.consistent:                       # CG iterations, solves, cap hits, the last solve's count (pfinish)
            self.t["pstats"] = torch.zeros(F.WIDE_PRESSURE_SCRATCH_LEN, dtype=torch.int64, device=self.device)
        if self.consistent_cu:                    # the same four words, added to by the one-CU kernel with ctrl
            self.t["pstats"] = torch.zeros(F.PRESSURE_STATS_LEN, dtype=torch.int64, device=self.device)
        self.linear_budget = int(p.linear_budget)        # grows when a solve overflows it (budget.advance_with_retries)
        self.linear_budget_retries = 0
        self.pressure_budget = int(p.pressure_budget)    # likewise
        self.pressure_budget_retries = 0
        self._handle = None
        self._wide = None
        self._batch1 = None                      # a "shared" trial alone: the batch object of one it is advanced through
        self.wide_graph = None                   # None: the library's default; set_wide_graph() chooses
        self._handle_tol = None
        self._make_handle(p.tolerance)

    # ---- device handle ----------------------------------------------------------------------------
    def _problem(self, tolerance: float) -> F.Problem:
        p, t = self.params, self.t
        pr = F.Problem(nx=self.nx, ny=self.ny, scheme=SCHEMES[p.convection_scheme], rec_cap=self.rec_cap, warmup=10,
                       max_lin_iters=LINEAR_MAX_ITERATIONS, dx=self.dx_min, dy=self.dy_min, rho=self.rho, mu=self.mu,
                       alpha_uv=float(p.alpha_uv), alpha_p=float(p.alpha_p), lin_tol=float(p.linear_solver_tol),
                       tol=float(tolerance), lid_velocity=float(p.lid_velocity))
        for name in ("ulid", "Qx", "lamx", "Qy", "lamy", "u", "v", "p", "mdot", "work", "rec", "ctrl"):
            setattr(pr, name, t[name].data_ptr())
        return pr

    def _make_handle(self, tolerance: float):
        import torch
        if (self._handle is not None or self._wide is not None) and self._handle_tol == tolerance:
            return
        self._destroy_handle()
        pr = self._problem(tolerance)
        with torch.cuda.device(self.device):
            torch.cuda.current_stream(self.device).synchronize()
            if self._has_cu_handle:
                h = C.c_void_p()
                F.check(F.lib().ldc_fv_create(C.byref(pr), C.byref(h)), "ldc_fv_create")
                self._handle = h
                if self.consistent_cu:
                    F.set_pressure(h, "consistent", float(self.params.pressure_tol), int(self.params.pressure_max_iters),
                                   self.t["pstats"].data_ptr(), self.t["pstats"].numel())
                if self.stretched:
                    F.set_grid(h, self.t["gridx"].data_ptr(), self.t["gridx"].numel(), self.t["gridy"].data_ptr(),
                               self.t["gridy"].numel())
                if self.separable:                # (after the grid: the call refuses a handle without geometry tables)
                    F.set_preconditioner(h, self.t["precx"].data_ptr(), self.t["precx"].numel(),
                                         self.t["precy"].data_ptr(), self.t["precy"].numel())
            if self.chip:
                h = C.c_void_p()
                F.check(F.lib().ldc_fv_wide_create(C.byref(pr), self.t["scratch"].data_ptr(),
                                                   self.t["scratch"].numel(), C.byref(h)), "ldc_fv_wide_create")
                self._wide = h
                if self.wide_graph is not None:
                    F.check(F.lib().ldc_fv_wide_set_graph(h, int(self.wide_graph)), "ldc_fv_wide_set_graph")
                if self.consistent:               # (likewise before the batch of one)
                    F.wide_set_pressure(h, "consistent", float(self.params.pressure_tol),
                                        int(self.params.pressure_max_iters), self.t["pstats"].data_ptr(),
                                        self.t["pstats"].numel())
                if self.chip_tables:              # (the tables of grid_axis; Qx, lamx, Qy, lamy are its eigenpairs already)
                    F.wide_set_grid(h, self.t["gridx"].data_ptr(), self.t["gridx"].numel(), self.t["gridy"].data_ptr(),
                                    self.t["gridy"].numel())
                if self.chip_separable:           # (after the grid: the call refuses a handle without geometry tables)
                    F.wide_set_preconditioner(h, self.t["precx"].data_ptr(), self.t["precx"].numel(),
                                              self.t["precy"].data_ptr(), self.t["precy"].numel())
                if self.mixed_chip:              # (before the batch of one below: a batch copies the block)
                    F.wide_set_anderson(h, self._anderson_block(), self.t["mix_scratch"].data_ptr(),
                                        self.t["mix_scratch"].numel())
                if self.shared:
                    self._batch1 = SharedBatch([self], self.wide_graph)
        self._handle_tol = tolerance

    def _destroy_handle(self):
        if getattr(self, "_batch1", None) is not None:
            self._batch1.close()
            self._batch1 = None
        if self._handle is not None:
            F.lib().ldc_fv_destroy(self._handle)
            self._handle = None
        if getattr(self, "_wide", None) is not None:
            F.lib().ldc_fv_wide_destroy(self._wide)
            self._wide = None
        self._handle_tol = None

    def set_wide_graph(self, on: bool):
        """A ``"chip"`` trial's launches: one replayed hipGraph per iteration (True) or every kernel on its own (False).
        The same kernels in the same order either way (tools/fv_wide_perf.py measures both).  A ``"shared"`` trial
        alone: the same for its batch of one (a batch of several has ``BatchedFVSolver.set_wide_graph``)."""
        if not self.chip:
            raise ValueError("set_wide_graph: only a mapping='chip' trial has launches to capture")
        self.wide_graph = bool(on)
        F.check(F.lib().ldc_fv_wide_set_graph(self._wide, int(self.wide_graph)), "ldc_fv_wide_set_graph")
        if self._batch1 is not None:
            self._batch1.set_graph(self.wide_graph)

    def _require_cu_handle(self, what: str):
        if self._handle is None:
            raise ValueError(f"{what}: a trial of {self.nx} x {self.ny} cells has no one-CU handle "
                             f"(at most {F.MAX_N} cells per axis)")

    def _anderson_block(self) -> F.Anderson:
        """This trial's block of an ``anderson_enqueue`` call (or of ``wide_set_anderson``): its depth and history, depth
        0 for a plain trial."""
        p = self.params
        if not (self.accelerated or self.mixed_chip):
            return F.Anderson(depth=0, start=1, hist=None, hist_len=0, astate=self.t["astate"].data_ptr())
        return F.Anderson(depth=int(p.anderson_depth), start=int(p.anderson_start), hist=self.t["hist"].data_ptr(),
                          hist_len=self.t["hist"].numel(), astate=self.t["astate"].data_ptr())

    def close(self):
        """Release the device handle (the torch tensors go with the object)."""
        self._destroy_handle()

    def __del__(self):
        try:
            self._destroy_handle()
        except Exception:
            pass

    @property
    def handle(self):
        return self._handle

    def _stream(self):
        import torch
        return torch.cuda.current_stream(self.device).cuda_stream

    def start_from(self, other: "FVSolver"):
        """This trial's state from ``other``'s (any FV trial of the same device and the same domain Lx, Ly; its grid and
        its other parameters may differ) by one prolongation (``prolong``): a coarser trial to start from, or a trial of
        this size at another Re to continue from."""
        prolong([(other, self)])

    def _transfer_axes(self):
        """(x, y) tensors [xc | h | d | g] of this trial's mesh (``transfer_axis``: shared per axis, mesh and device); a
        uniform trial is the mesh at beta = 0."""
        p = self.params
        beta = float(p.grid_stretch) if self.stretched else 0.0
        return transfer_axis(self.nx, p.Lx, beta, self.device), transfer_axis(self.ny, p.Ly, beta, self.device)

    def _prolong_tables_job(self, coarse: "FVSolver") -> F.ProlongTablesJob:
        """The job of a ``prolong_tables_enqueue`` call that starts THIS trial from ``coarse``: the coarse state, lid profile
        and centres, this trial's state, geometry tables and centres, the domain and this trial's rho."""
        t, c = self.t, coarse.t
        fx, fy = self._transfer_axes()
        cx, cy = coarse._transfer_axes()
        return F.ProlongTablesJob(
            coarse_u=c["u"].data_ptr(), coarse_v=c["v"].data_ptr(), coarse_p=c["p"].data_ptr(),
            coarse_ulid=c["ulid"].data_ptr(), coarse_xc=cx.data_ptr(), coarse_yc=cy.data_ptr(),
            fine_u=t["u"].data_ptr(), fine_v=t["v"].data_ptr(), fine_p=t["p"].data_ptr(), fine_mdot=t["mdot"].data_ptr(),
            fine_x_grid=fx[self.nx:].data_ptr(), fine_y_grid=fy[self.ny:].data_ptr(), fine_xc=fx.data_ptr(),
            fine_yc=fy.data_ptr(), Lx=float(self.params.Lx), Ly=float(self.params.Ly), rho=float(self.rho),
            coarse_nx=coarse.nx, coarse_ny=coarse.ny, fine_nx=self.nx, fine_ny=self.ny)

    # ---- state access (tests, tools) -------------------------------------------------------------------
    def set_state(self, u, v, p, mdot):
        """Overwrite the device state: u, v, p per cell (c = j*nx + i), mdot in the [fx | fy] face layout."""
        import torch
        for name, val in (("u", u), ("v", v), ("p", p), ("mdot", mdot)):
            self.t[name].copy_(torch.as_tensor(np.asarray(val, dtype=np.float64).ravel()))
        self.t["ctrl"].zero_()
        self.t["astate"].zero_()
        self._reset_budgets()
        self._post = None

    def _reset_budgets(self):
        """The budgets of a new solve, and the statistics words of its pressure solves at zero."""
        p = self.params
        self.linear_budget, self.linear_budget_retries = int(p.linear_budget), 0
        self.pressure_budget, self.pressure_budget_retries = int(p.pressure_budget), 0
        if self.consistent or self.consistent_cu:
            self.t["pstats"].zero_()

    def _budget_caps(self) -> tuple:
        """One cap per budget a chunk of this chip or shared trial carries: max_lin_iters, and with the consistent pressure
        equation pressure_max_iters."""
        return (LINEAR_MAX_ITERATIONS, int(self.params.pressure_max_iters)) if self.consistent else (LINEAR_MAX_ITERATIONS,)

    def _keep_budgets(self, budgets, retries):
        """What the retry loop of a chunk reports for this trial, one entry per cap: the budgets now, the retries added."""
        self.linear_budget = budgets[0]
        self.linear_budget_retries += retries[0]
        if len(budgets) > 1:
            self.pressure_budget = budgets[1]
            self.pressure_budget_retries += retries[1]

    def state(self) -> dict:
        return {k: self.t[k].cpu().numpy().copy() for k in ("u", "v", "p", "mdot")}

    def counters(self) -> dict:
        c = self.t["ctrl"].cpu().numpy()
        a = self.t["astate"].cpu().numpy()
        out = dict(done=int(c[F.CTRL_DONE]), iterations=int(c[F.CTRL_ITER]), nan=int(c[F.CTRL_NAN]),
                   linear_giveups=int(c[F.CTRL_GIVEUP]), linear_iterations=int(c[F.CTRL_LIN_ITERS]),
                   momentum_solves=int(c[F.CTRL_SOLVES]), anderson_fallbacks=int(a[F.ASTATE_FALLBACKS]),
                   linear_budget_retries=int(self.linear_budget_retries))
        if self.consistent or self.consistent_cu:
            ps = self.t["pstats"].cpu().numpy()
            out.update(pressure_iterations=int(ps[F.PSTAT_ITERS]), pressure_solves=int(ps[F.PSTAT_SOLVES]),
                       pressure_caps=int(ps[F.PSTAT_CAPS]), pressure_last=int(ps[F.PSTAT_LAST]))
        if self.consistent:                       # (the one-CU kernel has no budget: no retries to report)
            out.update(pressure_budget_retries=int(self.pressure_budget_retries))
        return out

    def step_debug(self, which=F.DBG) -> dict:
        """One iteration through ldc_fv_step_debug; returns the named intermediates (include/ldc_fv.h)."""
        import torch
        n, nf = self.n_cells, F.faces(self.nx, self.ny)
        size = dict(grad_p=2 * n, diag=5 * n, b=2 * n, mdot_star=nf, mdot=nf)
        bufs = {k: torch.full((size.get(k, n),), float("nan"), dtype=torch.float64, device=self.device) for k in which}
        ptrs = (C.c_void_p * len(F.DBG))(*[bufs[k].data_ptr() if k in bufs else None for k in F.DBG])
        mask = sum(1 << F.DBG.index(k) for k in which)
        with torch.cuda.device(self.device):
            F.check(F.lib().ldc_fv_step_debug(self._handle, mask, ptrs, C.c_void_p(self._stream())), "ldc_fv_step_debug")
            torch.cuda.current_stream(self.device).synchronize()
        return {k: b.cpu().numpy() for k, b in bufs.items()}

    # ---- LidDrivenCavitySolver hooks --------------------------------------------------------------------
    def _begin(self, tolerance: float):
        """A new solve: the trial's control words start at zero (latch, iteration count, NaN flag, the linear-solver
        counters), the fields stay.  Like the reference's loop (base.py:243) and the spectral solvers, every
        ``solve()`` counts from 0 on the current state, with its own warm-up, history and iteration count."""
        self._make_handle(tolerance)
        self.t["ctrl"].zero_()
        self.t["astate"].zero_()                 # (the mixing history starts over with the count: include/ldc_fv.h)
        self._reset_budgets()
        self._post = None

    def _wide_step(self, m: int, budget: int, pressure_budget: int = None):
        """One wide enqueue of up to ``m`` iterations at ``budget`` and ONE wait (the step of ``budget.advance_with_retries``
        for a batch of one; with a ``pressure_budget`` the overflow word tells which budget was too small)."""
        import torch
        from solvers.spectral import ldc_lib
        index = device_index(self.device)
        with torch.cuda.device(self.device):
            start = int(self.t["ctrl"][F.CTRL_ITER].item())
            if pressure_budget is not None:
                F.check(F.lib().ldc_fv_wide_set_pressure_budget(self._wide, int(pressure_budget)),
                        "ldc_fv_wide_set_pressure_budget")
            with ldc_lib.resident_lock(index):
                F.check(F.lib().ldc_fv_wide_enqueue(self._wide, int(m), int(budget), C.c_void_p(self._stream())),
                        "ldc_fv_wide_enqueue")
                c = self.t["ctrl"].cpu().numpy()          # (synchronises the stream)
            total = int(c[F.CTRL_ITER])
            rows = self.t["rec"][: total - start].cpu().numpy().copy()
            overflow = int(self.t["scratch"][:1].view(torch.int64).item())
        return rows, int(c[F.CTRL_DONE]), int(c[F.CTRL_NAN]), total, overflow

    def _advance(self, n_iters: int):
        n_iters = max(1, min(int(n_iters), self.rec_cap))
        if self.shared:
            rows, done, nan, total = self._batch1.advance([n_iters])[0]
            if nan:
                F.check(F.lib().ldc_fv_wide_status(self._wide), f"FV trial at iteration {total}")
            return rows, done, total
        if self.chip:
            start = int(self.t["ctrl"][F.CTRL_ITER].item())
            caps = self._budget_caps()
            (rows, done, nan, total, budgets, retries), = advance_with_retries(
                lambda quotas, *call: [self._wide_step(quotas[0], *call)], [start], [n_iters],
                [(self.linear_budget, self.pressure_budget)[:len(caps)]], caps)
            self._keep_budgets(budgets, retries)
            if nan:
                F.check(F.lib().ldc_fv_wide_status(self._wide), f"FV trial at iteration {total}")
            return rows, done, total
        rows, done, nan, total = advance([self], n_iters)[0]
        if nan:
            F.check(F.lib().ldc_fv_status(self._handle), f"FV trial at iteration {total}")
        return rows, done, total

    def _finalize_fields(self):
        st = self.state()
        self.fields.u, self.fields.v, self.fields.p = st["u"], st["v"], st["p"]

    # ---- vortex metrics (reference base.py:569-760), on the host once per solve ----------------------------
    def _ghost_gradient(self, f2, bc_lid):
        g = np.zeros((self.ny + 2, self.nx + 2))
        g[1:-1, 1:-1] = f2
        g[0, 1:-1] = -f2[0, :]
        g[-1, 1:-1] = 2 * bc_lid - f2[-1, :]
        g[1:-1, 0] = -f2[:, 0]
        g[1:-1, -1] = -f2[:, -1]
        return ((g[1:-1, 2:] - g[1:-1, :-2]) / (2 * self.dx_min), (g[2:, 1:-1] - g[:-2, 1:-1]) / (2 * self.dy_min))

    def _gauss_gradient(self, f2, lid):
        """(d f / dx, d f / dy) on the stretched grid: (f_e - f_w) / hx with g-weighted face values, 0 on the walls and
        ``lid`` (nx values) on the lid: the rule of the kernel's record (include/ldc_fv.h)."""
        ny, nx = self.shape_full
        gx, gy = self._gxf[1:-1][None, :], self._gyf[1:-1][:, None]
        fx, fy = np.zeros((ny, nx + 1)), np.zeros((ny + 1, nx))
        fx[:, 1:-1] = gx * f2[:, 1:] + (1.0 - gx) * f2[:, :-1]
        fy[1:-1, :] = gy * f2[1:, :] + (1.0 - gy) * f2[:-1, :]
        fy[-1, :] = lid
        return (fx[:, 1:] - fx[:, :-1]) / self._hx[None, :], (fy[1:, :] - fy[:-1, :]) / self._hy[:, None]

    def _vorticity(self) -> np.ndarray:
        U, V = self.fields.u.reshape(self.shape_full), self.fields.v.reshape(self.shape_full)
        if getattr(self, "stretched", False):
            dvdx, _ = self._gauss_gradient(V, 0.0)
            _, dudy = self._gauss_gradient(U, self._ulid_host)
            return dvdx - dudy
        dvdx, _ = self._ghost_gradient(V, 0.0)
        _, dudy = self._ghost_gradient(U, float(getattr(self.params, "lid_velocity", 1.0)))
        return dvdx - dudy

    def _streamfunction(self, omega):
        """psi from the 5-point Dirichlet Poisson problem on the interior cells (base.py:569-630)."""
        from scipy.sparse import diags
        from scipy.sparse.linalg import spsolve
        ny, nx = self.shape_full
        if getattr(self, "stretched", False):
            A = stretched_streamfunction_matrix(self._dxf, self._dyf)
            psi = np.zeros((ny, nx))
            psi[1:-1, 1:-1] = spsolve(A, -omega[1:-1, 1:-1].ravel()).reshape(ny - 2, nx - 2)
            return psi
        dx, dy = self.dx_min, self.dy_min
        ni = (ny - 2) * (nx - 2)
        cx, cy = 1.0 / (dx * dx), 1.0 / (dy * dy)
        dmain = np.full(ni, -2.0 * (cx + cy))
        dxo = np.full(ni - 1, cx)
        dyo = np.full(ni - (nx - 2), cy)
        for i in range(1, ny - 2):
            idx = i * (nx - 2) - 1
            if idx < len(dxo):
                dxo[idx] = 0.0
        A = diags([dyo, dxo, dmain, dxo, dyo], [-(nx - 2), -1, 0, 1, (nx - 2)], format="csr")
        psi = np.zeros((ny, nx))
        psi[1:-1, 1:-1] = spsolve(A, -omega[1:-1, 1:-1].ravel()).reshape(ny - 2, nx - 2)
        return psi

    def compute_vortex_metrics(self) -> dict:
        # (getattr: tests/fv_post_numpy.py calls this method on a bare namespace that has only the host branch's parameters)
        if getattr(self.params, "streamfunction", "reference") in WALL_RULES:
            return self._wall_vortex_metrics()
        if self.params.vortex_metrics in ("device", "chip"):
            return self._device_vortex_metrics()
        omega = self._vorticity()
        psi = self._streamfunction(omega)
        xs, ys = np.sort(np.unique(self.fields.x)), np.sort(np.unique(self.fields.y))
        imin = np.unravel_index(np.argmin(psi), psi.shape)
        imax = np.unravel_index(np.argmax(np.abs(omega)), omega.shape)
        out = dict(psi_min=float(psi[imin]), psi_min_x=float(xs[imin[1]]), psi_min_y=float(ys[imin[0]]),
                   omega_center=float(omega[imin]), omega_max=float(omega[imax]),
                   omega_max_x=float(xs[imax[1]]), omega_max_y=float(ys[imax[0]]))
        X, Y = np.meshgrid(xs, ys)
        regions = {"BR": (X > 0.5) & (Y < 0.5), "BL": (X < 0.5) & (Y < 0.5), "TL": (X < 0.5) & (Y > 0.5)}
        for name, mask in regions.items():
            k = np.unravel_index(np.argmax(np.where(mask, psi, -np.inf)), psi.shape)
            if psi[k] > 0:
                out.update({f"psi_{name}": float(psi[k]), f"psi_{name}_x": float(xs[k[1]]),
                            f"psi_{name}_y": float(ys[k[0]])})
            else:
                out.update({f"psi_{name}": 0.0, f"psi_{name}_x": 0.0, f"psi_{name}_y": 0.0})
        return out

    # ---- the same on the device (ldc_fv_post_enqueue, ldc_fv_wide_post_enqueue) ------------------------------
    def _device_vortex_metrics(self) -> dict:
        """The host branch's dict from the trial's result block: the block ``postprocess`` left (a batch post-processes
        its trials together), or one of a launch of its own."""
        if self._post is None:
            postprocess([self])
        r, self._post = self._post, None
        if r[F.POST_NONFINITE] != 0:
            raise FloatingPointError("vortex metrics: omega or psi is not finite")
        xs, ys = np.sort(np.unique(self.fields.x)), np.sort(np.unique(self.fields.y))
        xy = lambda c: (float(xs[int(c) % self.nx]), float(ys[int(c) // self.nx]))        # noqa: E731
        (x0, y0), (x1, y1) = xy(r[F.POST_PSI_MIN_CELL]), xy(r[F.POST_OMEGA_MAX_CELL])
        out = dict(psi_min=float(r[F.POST_PSI_MIN]), psi_min_x=x0, psi_min_y=y0,
                   omega_center=float(r[F.POST_OMEGA_CENTER]), omega_max=float(r[F.POST_OMEGA_MAX]),
                   omega_max_x=x1, omega_max_y=y1)
        for q, name in enumerate(("BR", "BL", "TL")):
            val, cell = float(r[F.POST_PSI_BR + q]), r[F.POST_PSI_BR_CELL + q]
            if val > 0:
                x, y = xy(cell)
                out.update({f"psi_{name}": val, f"psi_{name}_x": x, f"psi_{name}_y": y})
            else:
                out.update({f"psi_{name}": 0.0, f"psi_{name}_x": 0.0, f"psi_{name}_y": 0.0})
        return out

    # ---- the wall rule (ldc_fv_wall_post_enqueue) ---------------------------------------------------------------
    def _wall_buffers(self) -> dict:
        """``self.t`` with this trial's psi, omega and scratch of the wall rules, made at the first call."""
        import torch
        for name, size in (("psi", self.n_cells), ("omega", self.n_cells),
                           ("wall_scratch", F.wall_scratch_len(self.nx, self.ny))):
            if name not in self.t:
                self.t[name] = torch.zeros(size, dtype=torch.float64, device=self.device)
        return self.t

    def _wall_job(self, result_ptr: int) -> F.WallJob:
        """This trial's job of a ``wall_post_enqueue`` call: the state, the tables of its sizes (shared per device), its own
        psi, omega and scratch, and the row of the call's result tensor."""
        dev, t = self.device, self._wall_buffers()
        lamx, Cx = wall_eig(self.nx, dev)
        lamy, Cy = wall_eig(self.ny, dev)
        ix_lt, ix_gt, jy_lt, jy_gt = self._mask_bounds
        return F.WallJob(u=t["u"].data_ptr(), v=t["v"].data_ptr(), ulid=t["ulid"].data_ptr(), Cx=Cx.data_ptr(),
                         lamx=lamx.data_ptr(), Cy=Cy.data_ptr(), lamy=lamy.data_ptr(), psi=t["psi"].data_ptr(),
                         omega=t["omega"].data_ptr(), scratch=t["wall_scratch"].data_ptr(), result=result_ptr,
                         dx=self.dx_min, dy=self.dy_min, nx=self.nx, ny=self.ny, ix_lt=ix_lt, ix_gt=ix_gt, jy_lt=jy_lt,
                         jy_gt=jy_gt, refine=int(self.params.vortex_refine == "quadratic"), pad=0)

    def _wall_stretched_job(self, result_ptr: int) -> F.WallStretchedJob:
        """This trial's job of a ``wall_stretched_post_enqueue`` call: the state, the geometry tables its handle reads, the
        post tables of its axes (shared per mesh and device), its own psi, omega and scratch, and the row of the call's
        result tensor."""
        dev, t, p = self.device, self._wall_buffers(), self.params
        postx = wall_stretched_axis(self.nx, p.Lx, float(p.grid_stretch), dev)
        posty = wall_stretched_axis(self.ny, p.Ly, float(p.grid_stretch), dev)
        ix_lt, ix_gt, jy_lt, jy_gt = self._mask_bounds
        return F.WallStretchedJob(u=t["u"].data_ptr(), v=t["v"].data_ptr(), ulid=t["ulid"].data_ptr(),
                                  x_grid=t["gridx"].data_ptr(), y_grid=t["gridy"].data_ptr(), x_post=postx.data_ptr(),
                                  y_post=posty.data_ptr(), psi=t["psi"].data_ptr(), omega=t["omega"].data_ptr(),
                                  scratch=t["wall_scratch"].data_ptr(), result=result_ptr, nx=self.nx, ny=self.ny,
                                  ix_lt=ix_lt, ix_gt=ix_gt, jy_lt=jy_lt, jy_gt=jy_gt,
                                  refine=int(p.vortex_refine == "quadratic"), pad=0)

    def _wall_vortex_metrics(self) -> dict:
        """The metrics dict of a wall trial from its result block: the primary minimum and the corners from the groups
        (refined, or the cell's own values), under the existing rule that a corner counts when its grid value is > 0;
        ``omega_max`` stays on the grid.  ``omega_BR`` / ``omega_BL`` / ``omega_TL`` are filled."""
        if self._post is None or len(self._post) < F.WALL_RESULT_LEN:
            postprocess([self])
        r, self._post = self._post, None
        if r[F.POST_NONFINITE] != 0:
            raise FloatingPointError("vortex metrics: omega or psi is not finite")
        groups = r[F.POST_RESULT_LEN: F.WALL_RESULT_LEN].reshape(4, F.WALL_GROUP_LEN)
        refined = self.params.vortex_refine == "quadratic"
        self.vortex_refine_status = tuple(int(g[F.WALL_STATUS]) for g in groups) if refined else None
        cmax = int(r[F.POST_OMEGA_MAX_CELL])
        xs, ys = np.sort(np.unique(self.fields.x)), np.sort(np.unique(self.fields.y))      # (as the other two routes)
        g = groups[0]
        out = dict(psi_min=float(g[F.WALL_PSI]), psi_min_x=float(g[F.WALL_X]), psi_min_y=float(g[F.WALL_Y]),
                   omega_center=float(g[F.WALL_OMEGA]), omega_max=float(r[F.POST_OMEGA_MAX]),
                   omega_max_x=float(xs[cmax % self.nx]), omega_max_y=float(ys[cmax // self.nx]))
        for q, name in enumerate(("BR", "BL", "TL")):
            g = groups[1 + q]
            keep = float(r[F.POST_PSI_BR + q]) > 0
            vals = (g[F.WALL_PSI], g[F.WALL_OMEGA], g[F.WALL_X], g[F.WALL_Y]) if keep else (0.0, 0.0, 0.0, 0.0)
            out.update({f"psi_{name}": float(vals[0]), f"omega_{name}": float(vals[1]), f"psi_{name}_x": float(vals[2]),
                        f"psi_{name}_y": float(vals[3])})
        return out

    def _post_field(self, name) -> np.ndarray:
        if self.stretched and not self.stretched_wall:      # the reference's rule: on the host, from the current device state
            self._finalize_fields()
            omega = self._vorticity()
            return omega if name == "omega" else self._streamfunction(omega)
        postprocess([self])
        self._post = None
        return self.t[name].cpu().numpy().reshape(self.shape_full).copy()

    def streamfunction(self) -> np.ndarray:
        """psi (ny, nx) of the current device state, computed on the device."""
        return self._post_field("psi")

    def vorticity(self) -> np.ndarray:
        """omega (ny, nx) of the current device state, computed on the device."""
        return self._post_field("omega")

    # ---- Ghia centrelines: linear interpolation, as the reference plots FV fields ----------------------------
    def ghia_error(self) -> dict:
        ny, nx = self.shape_full
        x, y = self.fields.x.reshape(ny, nx)[0, :], self.fields.y.reshape(ny, nx)[:, 0]
        U, V = self.fields.u.reshape(ny, nx).T, self.fields.v.reshape(ny, nx).T        # -> [ix, iy]
        return _val.ghia_centerline_error(x, y, U, V, int(self.params.Re), interpolation="linear")
