"""Boundary types of the solver plugin surface.

Field names, defaults and the ``to_mlflow`` conventions are the contract the reference's
launcher relies on (reference src/solvers/datastructures.py:29-51 Parameters, :59-109
Metrics, :117-143 TimeSeries, :151-165 Fields, :257-279 SpectralParameters); only the
names are shared, the implementation is this project's own.  YAML values override the
dataclass defaults (e.g. ``CFL: 1.5`` in conf/solver/spectral/sg.yaml).
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass, field, fields
from typing import List, Optional

import numpy as np


def _mlflow_scalar(v):
    return int(v) if isinstance(v, bool) else v


class _Record:
    """Shared helpers: dict/DataFrame views of a dataclass."""

    def as_dict(self) -> dict:
        return {f.name: getattr(self, f.name) for f in fields(self)}

    def to_dataframe(self):
        import pandas as pd
        return pd.DataFrame([self.to_mlflow()])


@dataclass
class Parameters(_Record):
    name: str = ""
    Re: float = 100
    lid_velocity: float = 1.0
    Lx: float = 1.0
    Ly: float = 1.0
    nx: int = 64
    ny: int = 64
    max_iterations: int = 500
    tolerance: float = 1e-4
    method: str = ""

    def to_mlflow(self) -> dict:
        return {k: _mlflow_scalar(v) for k, v in self.as_dict().items()}


@dataclass
class SpectralParameters(Parameters):
    """nx/ny are the polynomial order N (N+1 collocation nodes per axis)."""
    basis_type: str = "legendre"
    CFL: float = 0.1
    beta_squared: float = 5.0
    method: str = "Spectral-AC"
    corner_treatment: str = "smoothing"
    corner_smoothing: float = 0.15
    multigrid: str = "none"
    n_levels: int = 3
    coarse_tolerance_factor: float = 10.0
    prolongation_method: str = "fft"
    restriction_method: str = "fft"
    # --- additions of the MI355X build (all optional, defaults keep reference behaviour) ---
    device: str = "cuda:0"
    check_every: int = 2048        # iterations enqueued between host polls of the latch
    graph_iters: int = 64          # iterations captured per hipGraph (32 -> 64: -0.2 us per N=256 iteration, flat beyond)
    nan_guard: bool = False        # quirk Q6: the reference SG spins on NaN; True = exit early
    diagnostics: bool = True       # E/Z/P every iteration, as base.py:274-276 does
    persistent: int = -1           # iteration loop: 0 = one launch per RK stage (hipGraph), 3 = the small-N kernel (one
                                   # launch per chunk, the trial on one XCD, N <= 79), 4 = the trial-per-CU kernel (M <= 44),
                                   # 5 = the chip-wide kernel (one launch per chunk, N = 81 ... 256), -1 = the library's
                                   # choice (include/ldc_hip.h): 3 / 5 where they apply; same results to rounding
    # where the reported vortices sit: "none" (the collocation node of the grid extremum, as the reference) or "newton"
    # (the stationary point of the interpolant of psi, ldc_vortex_refine).  Changes reported metrics: it goes to MLflow
    vortex_refine: str = "none"
    # where a solve() starts: "rest" (the fluid at rest under the lid, as the reference) or "fv" (a finite-volume solve of
    # the same cavity first -- mapping "chip", a batch's seeds together as mapping "shared"; TVD, the consistent pressure
    # equation -- sampled at the collocation nodes by ldc_fv_sample_nodes; solvers.spectral.warm_start).  The seed has
    # initial_guess_cells cells per axis (0: max(16, N), each axis by its own order), runs to initial_guess_tolerance
    # with the relaxation initial_guess_alpha_uv / _alpha_p, and a seed that fails leaves the trial at rest.  The stop
    # rule then ends another path to the same fixed point: all five change results and go to MLflow
    initial_guess: str = "rest"
    initial_guess_cells: int = 0
    initial_guess_tolerance: float = 1e-4
    initial_guess_alpha_uv: float = 0.7
    initial_guess_alpha_p: float = 0.3

    def to_mlflow(self) -> dict:
        skip = {"device", "check_every", "graph_iters", "nan_guard", "diagnostics", "persistent"}
        return {k: _mlflow_scalar(v) for k, v in self.as_dict().items() if k not in skip}


@dataclass
class FVParameters(Parameters):
    """Finite-volume SIMPLE solver (solvers.fv.solver.FVSolver); nx/ny are cell counts.  Defaults as the reference's
    (src/solvers/datastructures.py:174-186); conf/solver/fv.yaml overrides several (TVD, 0.4 / 0.2, 1e-9)."""
    convection_scheme: str = "Upwind"
    limiter: str = "MUSCL"
    alpha_uv: float = 0.6
    alpha_p: float = 0.4
    linear_solver_tol: float = 1e-6
    method: str = "FV-SIMPLE"
    corner_treatment: str = "none"
    corner_smoothing: float = 0.15
    # --- additions of the MI355X build (optional, defaults keep reference behaviour) ---
    device: str = "cuda:0"
    check_every: int = 2048        # iterations enqueued between host polls of the latch
    # streamfunction and vortex metrics after a solve: "host" (SciPy sparse solve, one trial after another), "device"
    # (ldc_fv_post_enqueue, all trials of a batch in one launch, one work-group per trial, at most 256 cells per axis) or
    # "chip" (ldc_fv_wide_post_enqueue, the whole chip per trial, 8 ... 1024 cells per axis, mapping "chip" or "shared"
    # only); not given: LDC_FV_VORTEX_METRICS may choose
    vortex_metrics: str = field(default_factory=lambda: os.environ.get("LDC_FV_VORTEX_METRICS", "host"))
    # Anderson acceleration of the outer iteration: "none", "anderson" (ldc_fv_anderson_enqueue, mapping "cu") or
    # "anderson_chip" (ldc_fv_wide_set_anderson: the same mixing as three launches over the whole chip, mapping "chip"
    # or "shared"), the number of difference columns kept (1 ... 16) and the iteration count from which the iterates
    # are mixed.  Real parameters of a run: they go to MLflow
    acceleration: str = "none"
    anderson_depth: int = 5
    anderson_start: int = 10
    # how a trial is laid on the device: "cu" (one work-group on one CU for its whole life; batches of them fill the
    # chip), "chip" (one kernel launch per phase over all CUs, 8 ... 1024 cells per axis, lone trials only) or "shared"
    # (the chip mapping's launches shared by all trials of a batch: for sweeps of fewer trials than CUs; bit-identical
    # to "chip"), and the BiCGSTAB iterations the first chunk of a "chip" or "shared" solve carries per SIMPLE iteration
    # (doubled when a solve needs more).  Neither changes what is computed beyond rounding: they stay out of MLflow,
    # like device
    mapping: str = "cu"
    linear_budget: int = 12
    # the pressure-correction equation: "reference" (the constant-coefficient Laplacian rho |S| / d, solved exactly: the
    # reference's, whose corrected face fluxes do not conserve mass) or "consistent" (the operator that also corrects the
    # fluxes, w_f = rho D_f |S| / d with D = V / a_P, by preconditioned CG to pressure_tol, at most pressure_max_iters
    # iterations per solve; mapping "chip" or "shared" only) or "consistent_cu" (the same equation inside the work-group of a
    # mapping "cu" trial).  They change results: they go to MLflow.  pressure_budget is the CG iterations the first chunk of
    # a chip or shared trial carries per SIMPLE iteration (doubled when a solve needs more; "consistent_cu" has no budget);
    # it changes nothing
    pressure_equation: str = "reference"
    pressure_tol: float = 1e-8
    pressure_max_iters: int = 200
    pressure_budget: int = 12
    # how the vortices are read off the result.  streamfunction: "reference" (psi = 0 at the centres of the boundary ring
    # of cells, the reference's rule, by whichever vortex_metrics route) or "wall" (psi = 0 on the wall faces and the lid
    # profile in omega's ghost row: second order; ldc_fv_wall_post_enqueue, always on the device, any mapping and size).
    # vortex_refine: "none" (every centre is a cell centre) or "quadratic" (the extremum of the quadratic through the
    # 3 x 3 cells around it; with a wall rule only).  Both change the reported metrics: they go to MLflow
    streamfunction: str = "reference"
    vortex_refine: str = "none"
    # the mesh: "uniform" (the reference's) or "tanh" (wall-clustered in both axes: vertices x_k = Lx s(k / nx),
    # s(xi) = (1 + tanh(beta (2 xi - 1)) / tanh(beta)) / 2 with beta = grid_stretch >= 0, read only then; 0 gives uniform
    # vertices through the stretched kernel).  mapping "cu" (or "chip" with chip_grid "tables", below), either pressure equation; no acceleration, device or chip
    # vortex metrics by the reference's rule, or streamfunction "wall" (the equal-spacing kernel); sequencing (solver=fv/fsg)
    # and start_from with transfer "tables" only (below);
    # streamfunction "wall_stretched" (tanh only, with or without the refinement) is the wall rule on the stretched mesh, on
    # the device (ldc_fv_wall_stretched_post_enqueue).  Both change results: they go to MLflow
    grid: str = "uniform"
    grid_stretch: float = 1.5
    # what prolong, start_from and the levels of solver=fv/fsg read the geometry from when THIS trial is the fine one of a pair:
    # "uniform" (dx, dy: ldc_fv_prolong_enqueue and its chip twin, equal spacing on both trials) or "tables" (per-axis tables
    # of centres, widths and face weights: ldc_fv_prolong_tables_enqueue; mapping "cu" only, either grid on either side, so a
    # grid "tanh" trial can be sequenced, continued in Re, or started from a uniform one).  On a uniform pair the two agree to
    # rounding, not bit for bit (the centres are vertex midpoints here and (k + 1/2) h there): it goes to MLflow
    transfer: str = "uniform"
    # what preconditions the CG of the consistent pressure equation: "laplacian" (the operator with D left out, exactly
    # inverted) or "separable" (D fitted by a product a_i b_j, that operator exactly inverted, and the rest of D taken by a
    # diagonal scaling: ldc_fv_set_preconditioner; grid "tanh" with pressure_equation "consistent_cu" only, where it takes a
    # third of the CG iterations; on a uniform grid nothing is gained).  Both solve the same equation to pressure_tol, so the
    # results differ at that level: it goes to MLflow
    pressure_preconditioner: str = "laplacian"
    # what the phase kernels of a mapping "chip" trial read the geometry from: "uniform" (dx, dy) or "tables" (the per-axis
    # tables of grid "tanh": ldc_fv_wide_set_grid; accepted only with grid "tanh" and mapping "chip", a lone trial of
    # 8 ... 1024 cells per axis, pressure_equation "reference" or "consistent"; no acceleration; sequencing and start_from
    # with chip_transfer "tables" only (below),
    # and pressure_preconditioner stays "laplacian" (the separable preconditioner of such a trial is chip_preconditioner,
    # below); vortex metrics on the host, or streamfunction "wall_stretched" at every size).  With the
    # default a grid "tanh" trial takes mapping "cu" as before.  Like mapping it names where the same iteration runs (the
    # two agree to rounding): it stays out of MLflow
    chip_grid: str = "uniform"
    # what preconditions the CG of such a trial (mapping "chip", grid "tanh", chip_grid "tables") with pressure_equation
    # "consistent": "laplacian" (the operator with D left out) or "separable" (the fit, the tables and the scaling of
    # pressure_preconditioner "separable", on the chip chain: ldc_fv_wide_set_preconditioner; a fifth to a twentieth of the CG
    # iterations per solve).  "separable" is accepted only with all of those and pressure_preconditioner "laplacian".  Both
    # solve the same equation to pressure_tol, so the results differ at that level: it goes to MLflow
    chip_preconditioner: str = "laplacian"
    # what prolong, start_from and the levels of solver=fv/fsg read the geometry from when THIS trial, a lone mapping "chip"
    # trial, is the fine one of a pair: "uniform" (the routes of `transfer` above: equal spacing, and a grid "tanh" chip trial
    # starts from rest only) or "tables" (per-axis tables on both sides through ldc_fv_wide_prolong_tables_enqueue, two
    # launches over the whole chip per pair, 8 ... 1024 cells per axis on either side; accepted only with mapping "chip", on
    # grid "uniform" or on grid "tanh" with chip_grid "tables", and with transfer "uniform"; the coarse trial of a pair may be
    # of any mapping and grid).  With it solver=fv/fsg sequences a stretched chip trial up to 1024 cells.  Like transfer it
    # changes the start of a solve (on a uniform pair to rounding): it goes to MLflow
    chip_transfer: str = "uniform"

    def to_mlflow(self) -> dict:
        skip = {"device", "check_every", "vortex_metrics", "mapping", "linear_budget", "chip_grid"}
        return {k: _mlflow_scalar(v) for k, v in self.as_dict().items() if k not in skip}


@dataclass
class FVFSGParameters(FVParameters):
    """Coarse-to-fine grid sequencing of the finite-volume solver (solvers.fv.fsg.FVFSGSolver): converge on n // 2 (and
    coarser), prolong, converge on n.  All three are real parameters of a run and go to MLflow."""
    n_levels: int = 2                        # at most this many levels, the fine one included
    coarsest_n: int = 16                     # no level has fewer cells per axis
    coarse_tolerance_factor: float = 1.0     # a level k levels below the fine one runs to tolerance * factor^k


_VORTEX_KEYS = (
    "psi_min", "psi_min_x", "psi_min_y", "omega_center",
    "omega_max", "omega_max_x", "omega_max_y",
    "psi_BR", "omega_BR", "psi_BR_x", "psi_BR_y",
    "psi_BL", "omega_BL", "psi_BL_x", "psi_BL_y",
    "psi_TL", "omega_TL", "psi_TL_x", "psi_TL_y",
)


@dataclass
class Metrics(_Record):
    iterations: int = 0
    converged: bool = False
    final_residual: float = float("inf")
    wall_time_seconds: float = 0.0
    u_momentum_residual: float = 0.0
    v_momentum_residual: float = 0.0
    continuity_residual: float = 0.0
    final_energy: float = 0.0
    final_enstrophy: float = 0.0
    final_palinstrophy: float = 0.0
    psi_min: float = 0.0
    psi_min_x: float = 0.0
    psi_min_y: float = 0.0
    omega_center: float = 0.0
    omega_max: float = 0.0
    omega_max_x: float = 0.0
    omega_max_y: float = 0.0
    psi_BR: float = 0.0
    omega_BR: float = 0.0
    psi_BR_x: float = 0.0
    psi_BR_y: float = 0.0
    psi_BL: float = 0.0
    omega_BL: float = 0.0
    psi_BL_x: float = 0.0
    psi_BL_y: float = 0.0
    psi_TL: float = 0.0
    omega_TL: float = 0.0
    psi_TL_x: float = 0.0
    psi_TL_y: float = 0.0

    def to_mlflow(self) -> dict:
        """Bools as ints; values equal to +inf (unset) are dropped."""
        return {k: _mlflow_scalar(v) for k, v in self.as_dict().items() if v != math.inf}


@dataclass
class TimeSeries:
    rel_iter_residual: List[float] = field(default_factory=list)
    u_residual: List[float] = field(default_factory=list)
    v_residual: List[float] = field(default_factory=list)
    continuity_residual: Optional[List[float]] = field(default_factory=list)
    energy: List[float] = field(default_factory=list)
    enstrophy: List[float] = field(default_factory=list)
    palinstrophy: List[float] = field(default_factory=list)

    def items(self):
        return [(f.name, getattr(self, f.name)) for f in fields(self)]

    def to_records(self) -> list:
        """(key, step, value) triples; what the reference turns into mlflow Metric objects."""
        return [(k, step, v) for k, vals in self.items() if vals
                for step, v in enumerate(vals) if v is not None]

    def to_mlflow_batch(self) -> list:
        try:
            from mlflow.entities import Metric
        except ImportError:          # MLflow is optional in this build
            return self.to_records()
        return [Metric(key=k, value=v, timestamp=0, step=s) for k, s, v in self.to_records()]

    def to_dataframe(self):
        import pandas as pd
        return pd.DataFrame({k: v for k, v in self.items() if v})


@dataclass
class Fields:
    """Flat solution arrays of length (N+1)^2, C order of [ix, iy]."""
    u: np.ndarray
    v: np.ndarray
    p: np.ndarray
    x: np.ndarray
    y: np.ndarray

    def to_dataframe(self):
        import pandas as pd
        return pd.DataFrame({"x": self.x, "y": self.y, "u": self.u, "v": self.v, "p": self.p})
