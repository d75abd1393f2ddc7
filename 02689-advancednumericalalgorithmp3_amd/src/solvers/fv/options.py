"""The options of a finite-volume trial: their values, which of them go together, and the flags the solver routes on.

``check`` is what ``FVSolver.__init__`` asks before it allocates anything: every refusal is a ``ValueError`` that names the
option, the value and what to give instead.  The first check that fails decides the message, so the order below is part of
the behaviour (tests/test_fv_options_cpu.py holds it against a record of every combination); each option's enumeration check
stands next to its compatibility checks as far as that order allows."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from . import ldc_fv_lib as F

SCHEMES = {"Upwind": 0, "TVD": 1}
VORTEX_METRICS = ("host", "device", "chip")
ACCELERATIONS = ("none", "anderson", "anderson_chip")
MAPPINGS = ("cu", "chip", "shared")
# "consistent": the chain of launches over the whole chip (mapping "chip" / "shared"); "consistent_cu": the same equation
# inside the work-group of a one-CU trial (mapping "cu"); both are LDC_FV_PRESSURE_CONSISTENT to the library
PRESSURE_EQUATIONS = ("reference", "consistent", "consistent_cu")
STREAMFUNCTIONS = ("reference", "wall", "wall_stretched")
WALL_RULES = ("wall", "wall_stretched")      # the wall rule on equal spacing, and on the tables of grid="tanh"
VORTEX_REFINES = ("none", "quadratic")
GRIDS = ("uniform", "tanh")
# what the phase kernels of a mapping "chip" trial read the geometry from: "uniform" (dx, dy) or "tables" (the per-axis tables
# of grid="tanh": ldc_fv_wide_set_grid, a lone chip trial of 8 ... 1024 cells per axis)
CHIP_GRIDS = ("uniform", "tables")
# what preconditions the CG of such a trial with pressure_equation "consistent": "laplacian" (the operator with D left out) or
# "separable" (the tables of pressure_preconditioner "separable" on the chip chain: ldc_fv_wide_set_preconditioner)
CHIP_PRECONDITIONERS = ("laplacian", "separable")
PRESSURE_PRECONDITIONERS = ("laplacian", "separable")
# what prolong / start_from / the levels of solver=fv/fsg read the geometry from: "uniform" (dx, dy: the equal-spacing kernels)
# or "tables" (per-axis tables of centres, widths and face weights: ldc_fv_prolong_tables_enqueue, either grid, mapping "cu")
TRANSFERS = ("uniform", "tables")
# the same choice for a lone mapping "chip" trial as the fine one of a pair: "uniform" (the routes of `transfer`) or "tables"
# (ldc_fv_wide_prolong_tables_enqueue: both grids from per-axis tables, two launches over the chip, 8 ... 1024 cells per axis)
CHIP_TRANSFERS = ("uniform", "tables")


def check(p, needs_cu_handle=None) -> SimpleNamespace:
    """The parameters ``p`` of one trial, checked; ``needs_cu_handle`` is the name of a solver that cannot do without the
    one-CU handle (``FVFSGSolver``: "an FSG level"), or None.  Returns the flags derived from them."""
    # ---- scheme, post-processing -----------------------------------------------------------------------------------
    if p.convection_scheme not in SCHEMES:
        raise ValueError(f"convection_scheme={p.convection_scheme!r}: 'Upwind' or 'TVD'")
    if p.convection_scheme == "TVD" and p.limiter != "MUSCL":
        raise ValueError(f"limiter={p.limiter!r}: the TVD scheme of the reference is MUSCL")
    if p.vortex_metrics not in VORTEX_METRICS:
        raise ValueError(f"vortex_metrics={p.vortex_metrics!r}: 'host', 'device' or 'chip'")
    if p.streamfunction not in STREAMFUNCTIONS:
        raise ValueError(f"streamfunction={p.streamfunction!r}: 'reference', 'wall' or 'wall_stretched'")
    if p.vortex_refine not in VORTEX_REFINES:
        raise ValueError(f"vortex_refine={p.vortex_refine!r}: 'none' or 'quadratic'")
    if p.vortex_refine == "quadratic" and p.streamfunction not in WALL_RULES:
        raise ValueError("vortex_refine='quadratic' with streamfunction='reference': the ring rule's O(h) error in psi "
                         "makes sub-cell centres moot, give the trial streamfunction='wall'")
    # ---- acceleration, mapping (their compatibility waits for the sizes, below) --------------------------------------
    if p.acceleration not in ACCELERATIONS:
        raise ValueError(f"acceleration={p.acceleration!r}: 'none', 'anderson' or 'anderson_chip'")
    if not 1 <= int(p.anderson_depth) <= F.ANDERSON_MAX_DEPTH:
        raise ValueError(f"anderson_depth={p.anderson_depth}: 1 ... {F.ANDERSON_MAX_DEPTH} columns")
    if int(p.anderson_start) < 1:
        raise ValueError(f"anderson_start={p.anderson_start}: an iteration count, at least 1")
    accelerated = p.acceleration == "anderson"       # the one-CU mixing path: advance() routes on it
    mixed_chip = p.acceleration == "anderson_chip"   # the mixing chain of the chip mapping, attached to the handle
    if p.mapping not in MAPPINGS:
        raise ValueError(f"mapping={p.mapping!r}: 'cu', 'chip' or 'shared'")
    if int(p.linear_budget) < 1:
        raise ValueError(f"linear_budget={p.linear_budget}: BiCGSTAB iterations per SIMPLE iteration, at least 1")
    # ---- pressure equation ---------------------------------------------------------------------------------------------
    if p.pressure_equation not in PRESSURE_EQUATIONS:
        raise ValueError(f"pressure_equation={p.pressure_equation!r}: 'reference', 'consistent' or 'consistent_cu'")
    consistent = p.pressure_equation == "consistent"          # the chip chain, with its budget protocol
    consistent_cu = p.pressure_equation == "consistent_cu"    # the one-CU kernel: no budget, no retries
    if consistent_cu and p.mapping != "cu":
        raise ValueError(f"pressure_equation='consistent_cu' with mapping={p.mapping!r}: the one-CU kernel of the "
                         f"consistent pressure equation takes mapping='cu' trials (a chip or shared trial takes "
                         f"pressure_equation='consistent')")
    if consistent and p.mapping == "cu":
        raise ValueError("pressure_equation='consistent' with mapping='cu': the consistent pressure equation is solved "
                         "by launches over the whole chip, give the trial mapping=chip (or mapping=shared)")
    if not 0.0 < float(p.pressure_tol) < 1.0:
        raise ValueError(f"pressure_tol={p.pressure_tol}: a relative residual, between 0 and 1")
    if int(p.pressure_max_iters) < 1:
        raise ValueError(f"pressure_max_iters={p.pressure_max_iters}: CG iterations per pressure solve, at least 1")
    if int(p.pressure_budget) < 1:
        raise ValueError(f"pressure_budget={p.pressure_budget}: CG iterations per SIMPLE iteration, at least 1")
    # ---- transfers -----------------------------------------------------------------------------------------------------
    if p.transfer not in TRANSFERS:
        raise ValueError(f"transfer={p.transfer!r}: 'uniform' or 'tables'")
    transfer_tables = p.transfer == "tables"         # prolong() routes the pairs this trial is the FINE one of on it
    if p.chip_transfer not in CHIP_TRANSFERS:
        raise ValueError(f"chip_transfer={p.chip_transfer!r}: 'uniform' or 'tables'")
    chip_transfer_tables = p.chip_transfer == "tables"       # likewise, through ldc_fv_wide_prolong_tables_enqueue
    if chip_transfer_tables:
        if p.mapping != "chip":
            raise ValueError(f"chip_transfer='tables' with mapping={p.mapping!r}: the transfer over the whole chip that "
                             f"reads the grids from tables starts a lone mapping='chip' trial (a one-CU trial takes "
                             f"transfer='tables')")
        if transfer_tables:
            raise ValueError("chip_transfer='tables' beside transfer='tables': one transfer per trial, and transfer="
                             "'tables' is the one-CU kernel's (mapping='cu')")
        if p.grid == "tanh" and p.chip_grid != "tables":
            raise ValueError(f"chip_transfer='tables' with grid='tanh' and chip_grid={p.chip_grid!r}: a stretched chip "
                             f"trial takes chip_grid='tables'")
    if transfer_tables and p.mapping != "cu":
        raise ValueError(f"transfer='tables' with mapping={p.mapping!r}: the transfer that reads the grids from tables "
                         f"takes mapping='cu' trials")
    # ---- grid ----------------------------------------------------------------------------------------------------------
    if p.grid not in GRIDS:
        raise ValueError(f"grid={p.grid!r}: 'uniform' or 'tanh'")
    stretched = p.grid == "tanh"             # geometry tables on the handle: fv_stretched_kernel advances the trial
    if p.chip_grid not in CHIP_GRIDS:
        raise ValueError(f"chip_grid={p.chip_grid!r}: 'uniform' or 'tables'")
    chip_tables = p.chip_grid == "tables"    # ... or, on the wide handle, the stretched twins of the chip chain
    if chip_tables and not stretched:
        raise ValueError(f"chip_grid='tables' with grid={p.grid!r}: the tables are those of a wall-clustered mesh, give the "
                         f"trial grid='tanh' (or chip_grid='uniform')")
    if chip_tables and p.mapping != "chip":
        raise ValueError(f"chip_grid='tables' with mapping={p.mapping!r}: the stretched phase kernels advance a lone "
                         f"mapping='chip' trial (a shared batch has no room for the tables in its table entry; a one-CU "
                         f"trial reads them without the option)")
    if stretched:
        if not float(p.grid_stretch) >= 0.0 or not np.isfinite(float(p.grid_stretch)):
            raise ValueError(f"grid_stretch={p.grid_stretch}: the tanh clustering parameter, a finite number >= 0")
        if p.mapping != "cu" and not chip_tables:
            raise ValueError(f"grid='tanh' with mapping={p.mapping!r}: stretched grids run on the one-CU kernel only "
                             f"(mapping='cu')")
        if p.acceleration != "none":
            raise ValueError(f"grid='tanh' with acceleration={p.acceleration!r}: Anderson mixing has not been tested "
                             f"on stretched grids, give the trial acceleration='none'")
        if needs_cu_handle and not (transfer_tables or chip_transfer_tables):
            raise ValueError("grid='tanh' with solver=fv/fsg: the prolongation between the levels assumes equal "
                             "spacing, run the trial with solver=fv (or give it transfer='tables', the transfer that "
                             "reads the grids of both levels from tables)")
        # (streamfunction="wall_stretched" is served on the device by ldc_fv_wall_stretched_post_enqueue and does not
        # consult vortex_metrics, as "wall" does not for uniform trials)
        if p.vortex_metrics != "host" and p.streamfunction != "wall_stretched":
            raise ValueError(f"grid='tanh' with vortex_metrics={p.vortex_metrics!r}: the post-processing kernels of the "
                             f"reference's rule assume equal spacing, give the trial vortex_metrics='host' (or "
                             f"streamfunction='wall_stretched')")
        if p.streamfunction == "wall":
            raise ValueError("grid='tanh' with streamfunction='wall': that kernel assumes equal spacing, give the trial "
                             "streamfunction='wall_stretched' (the wall rule on the stretched mesh)")
    elif p.streamfunction == "wall_stretched":
        raise ValueError(f"streamfunction='wall_stretched' with grid={p.grid!r}: it reads the tables of a stretched mesh, "
                         f"give the trial grid='tanh' (or streamfunction='wall')")
    stretched_wall = p.streamfunction == "wall_stretched"     # postprocess() routes on it
    # ---- preconditioners -----------------------------------------------------------------------------------------------
    if p.pressure_preconditioner not in PRESSURE_PRECONDITIONERS:
        raise ValueError(f"pressure_preconditioner={p.pressure_preconditioner!r}: 'laplacian' or 'separable'")
    separable = p.pressure_preconditioner == "separable"      # tables on the handle: fv_stretched_sep_kernel
    if separable and not (stretched and consistent_cu):
        raise ValueError(f"pressure_preconditioner='separable' with grid={p.grid!r}, pressure_equation="
                         f"{p.pressure_equation!r}: it preconditions the CG of a stretched one-CU trial, give the trial "
                         f"grid='tanh' and pressure_equation='consistent_cu'")
    if p.chip_preconditioner not in CHIP_PRECONDITIONERS:
        raise ValueError(f"chip_preconditioner={p.chip_preconditioner!r}: 'laplacian' or 'separable'")
    chip_separable = p.chip_preconditioner == "separable"     # tables on the wide handle: the twins of the CG launches
    if chip_separable and not (chip_tables and consistent):
        raise ValueError(f"chip_preconditioner='separable' with mapping={p.mapping!r}, grid={p.grid!r}, chip_grid="
                         f"{p.chip_grid!r}, pressure_equation={p.pressure_equation!r}: it preconditions the CG of a lone "
                         f"stretched chip trial, give the trial mapping='chip', grid='tanh', chip_grid='tables' and "
                         f"pressure_equation='consistent' (a one-CU trial takes pressure_preconditioner='separable')")
    # ---- sizes, and what hangs on the mapping ----------------------------------------------------------------------------
    shared = p.mapping == "shared"           # the phase kernels of csrc/ldc_fv_wide.hip: a launch of its own per
    chip = p.mapping == "chip" or shared     # phase ("chip") or one for all trials of a batch ("shared")
    nx, ny = int(p.nx), int(p.ny)
    max_n = F.WIDE_MAX_N if chip else F.MAX_N
    if not (F.MIN_N <= nx <= max_n and F.MIN_N <= ny <= max_n):
        raise ValueError(f"nx, ny = {nx}, {ny}: the FV kernel takes {F.MIN_N} ... {max_n} cells per axis "
                         f"with mapping={p.mapping!r}")
    if chip and accelerated:
        raise ValueError(f"acceleration='anderson' with mapping={p.mapping!r}: the mixing kernel follows the one-CU "
                         f"kernel's launches only (a chip or shared trial takes acceleration='anderson_chip')")
    if mixed_chip and not chip:
        raise ValueError(f"acceleration='anderson_chip' with mapping={p.mapping!r}: the mixing chain over the whole "
                         f"chip takes mapping='chip' or 'shared' trials (a one-CU trial takes acceleration='anderson')")
    if p.vortex_metrics == "chip" and not chip:
        raise ValueError(f"vortex_metrics='chip' with mapping={p.mapping!r}: the post-processing chain over the whole "
                         f"chip takes mapping='chip' or 'shared' trials")
    # the one-CU handle beside the wide one wherever it exists: postprocess, prolong and start_from use it
    has_cu_handle = not chip or max(nx, ny) <= F.MAX_N
    # (with chip_transfer="tables" the levels are prolonged over the whole chip: no level needs the one-CU handle)
    if needs_cu_handle and not has_cu_handle and not chip_transfer_tables:
        raise ValueError(f"{needs_cu_handle} of {nx} x {ny} cells: the prolongation takes at most {F.MAX_N} "
                         f"cells per axis")
    if p.vortex_metrics == "device" and not has_cu_handle:
        raise ValueError(f"vortex_metrics='device' at {nx} x {ny}: device post-processing takes at most {F.MAX_N} "
                         f"cells per axis")
    return SimpleNamespace(
        accelerated=accelerated, mixed_chip=mixed_chip, consistent=consistent, consistent_cu=consistent_cu,
        transfer_tables=transfer_tables, chip_transfer_tables=chip_transfer_tables, stretched=stretched,
        chip_tables=chip_tables, stretched_wall=stretched_wall, separable=separable, chip_separable=chip_separable,
        shared=shared, chip=chip, _has_cu_handle=has_cu_handle)
