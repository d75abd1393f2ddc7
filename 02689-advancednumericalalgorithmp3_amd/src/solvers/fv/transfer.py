"""Coarse-to-fine transfer between finite-volume trials on the device: ``prolong`` and its routes.

The default ``transfer="uniform"`` is the equal-spacing transfer (``ldc_fv_prolong_enqueue``, one work-group per pair; above
256 cells per axis ``ldc_fv_wide_prolong_enqueue``, two launches over the whole chip).  ``transfer="tables"`` on the FINE
trial of a pair reads both grids from per-axis tables (``ldc_fv_prolong_tables_enqueue``: one work-group per pair, 23 pairs
per launch), so stretched trials are sequenced, continued in Re and started from uniform ones.  ``chip_transfer="tables"`` is
the same for a lone ``mapping="chip"`` trial on either grid (``ldc_fv_wide_prolong_tables_enqueue``: the same arithmetic, two
launches over the whole chip per pair, 8 ... 1024 cells per axis on both sides, a source of any mapping and grid), so a
stretched chip trial is sequenced up to 1024 cells.  What ``prolong`` asks of a trial is its flags, handles and job builder,
so this module does not know ``FVSolver``."""
from __future__ import annotations

from . import ldc_fv_lib as F
from .grids import device_index


def prolong_route(coarse_has_cu: bool, fine_has_cu: bool, coarse_chip: bool, fine_chip: bool, fine_tables: bool = False) -> str:
    """The entry that prolongs a (coarse, fine) pair: ``"tables"`` (``ldc_fv_prolong_tables_enqueue``: the geometry of both
    from per-axis tables) when the FINE trial has ``transfer="tables"``, whatever the coarse one's grid and option; else
    ``"cu"`` (``ldc_fv_prolong_enqueue``) when both trials have a one-CU
    handle; else ``"chip"`` (``ldc_fv_wide_prolong_enqueue``), which takes the whole-chip handles of both: a trial without
    one is a ``ValueError``."""
    if fine_tables:
        if not (coarse_has_cu and fine_has_cu):
            raise ValueError(f"prolong: transfer='tables' takes trials of at most {F.MAX_N} cells per axis on both sides")
        return "tables"
    if coarse_has_cu and fine_has_cu:
        return "cu"
    if coarse_chip and fine_chip:
        return "chip"
    raise ValueError(f"prolong: a trial above {F.MAX_N} cells per axis is prolonged through the whole-chip handles of both "
                     f"trials, and one of them has none: give the coarse trial mapping='chip' (or 'shared')")


def _same_extent(a: float, b: float) -> bool:
    """One domain length, to the rounding the equal-spacing kernels allow (1e-12 relative)."""
    return abs(float(a) - float(b)) <= 1e-12 * max(abs(float(a)), abs(float(b)))


def prolong(pairs):
    """Start every fine trial from the state of its coarse one: ``pairs`` of (coarse, fine) FVSolvers on one device, of
    any sizes and parameters but one domain (Lx, Ly), none in flight (``ldc_fv_prolong_enqueue``: bilinear in u, v, p from the coarse cell
    centres and the boundary values, p pinned at cell 0, mdot from the new u and v).  One call of the library for all pairs, which it checks together and
    launches ``PROLONG_LAUNCH_MAX`` (128) at a time, one work-group each; the fine trials' control words, records and work vectors are left alone (a ``solve()`` zeroes the
    control words itself), and so are the coarse trials.  A fine trial must not be the coarse or the fine trial of
    another pair of the same call: chain levels with one call per level.

    A pair with a trial above 256 cells per axis (no one-CU handle) goes through ``ldc_fv_wide_prolong_enqueue`` instead,
    two launches over the whole chip per pair, the same arithmetic; both its trials must then be ``mapping="chip"`` or
    ``"shared"`` trials (``prolong_route``).

    A pair whose FINE trial has ``transfer="tables"`` goes through ``ldc_fv_prolong_tables_enqueue``: the same transfer with
    the geometry of both trials read from per-axis tables, so either may be a ``grid="tanh"`` trial (the coarse one with any
    ``transfer``); all such pairs of a call are one call of the library, 23 per launch, one work-group each.  A pair with a
    stretched trial whose fine trial lacks the option is refused.

    A pair whose FINE trial has ``chip_transfer="tables"`` (a lone ``mapping="chip"`` trial on either grid) goes through
    ``ldc_fv_wide_prolong_tables_enqueue``: the same arithmetic, two launches over the whole chip per pair, 8 ... 1024 cells per
    axis on both sides; the coarse trial may be of any mapping and grid.  All routes may stand in one call."""
    import torch
    from solvers.spectral import ldc_lib
    pairs = list(pairs)
    if not pairs:
        return
    # (getattr: a trial built before the option, or a stand-in that has only `stretched`, is a transfer="uniform" trial)
    by_tables = [bool(getattr(f, "transfer_tables", False)) for _, f in pairs]
    by_chip_tables = [bool(getattr(f, "chip_transfer_tables", False)) for _, f in pairs]
    for (c, f), tables, chip_tables in zip(pairs, by_tables, by_chip_tables):
        if (c.stretched or f.stretched) and not (tables or chip_tables):
            raise ValueError("prolong / start_from with grid='tanh': the prolongation kernel assumes equal spacing on both "
                             "trials; give the FINE trial transfer='tables' (the transfer that reads both grids from tables)")
    dev = pairs[0][1].device
    index = device_index(dev)
    # (a fine trial with chip_transfer="tables" takes raw pointers of both trials: no handle of a particular kind is needed)
    routes = ["chip_tables" if chip_tables else prolong_route(c._has_cu_handle, f._has_cu_handle, c.chip, f.chip, tables)
              for (c, f), tables, chip_tables in zip(pairs, by_tables, by_chip_tables)]
    for (c, f), route in zip(pairs, routes):
        for s in (c, f):
            if route in ("cu", "tables"):
                s._require_cu_handle("prolong")
            elif route == "chip" and s._wide is None:
                raise ValueError(f"prolong: a trial of {s.nx} x {s.ny} cells has no whole-chip handle")
            if device_index(s.device) != index:
                raise ValueError("prolong: all trials must be on one device")
        if route in ("tables", "chip_tables") and not (_same_extent(c.params.Lx, f.params.Lx) and _same_extent(c.params.Ly, f.params.Ly)):
            raise ValueError(f"prolong: the trials of a pair cover one domain, got Lx, Ly = {c.params.Lx}, {c.params.Ly} and "
                             f"{f.params.Lx}, {f.params.Ly}")
    cu = [pair for pair, route in zip(pairs, routes) if route == "cu"]
    chip = [pair for pair, route in zip(pairs, routes) if route == "chip"]
    tables = [pair for pair, route in zip(pairs, routes) if route == "tables"]
    chip_tables = [pair for pair, route in zip(pairs, routes) if route == "chip_tables"]
    if chip or tables or chip_tables:  # (the library checks the pairs of ONE of its calls together; with others beside them the rule is kept here)
        for q, (_, f) in enumerate(pairs):
            if any(f is c2 or (r != q and f is f2) for r, (c2, f2) in enumerate(pairs)):
                raise ValueError("prolong: a fine trial is the coarse or the fine trial of another pair of the call")
    with torch.cuda.device(dev):
        jobs = [f._prolong_tables_job(c) for c, f in tables]
        chip_jobs = [f._prolong_tables_job(c) for c, f in chip_tables]
        with ldc_lib.resident_lock(index):
            stream = torch.cuda.current_stream(dev).cuda_stream
            if cu:
                F.prolong_enqueue([c.handle for c, _ in cu], [f.handle for _, f in cu], stream)
            for c, f in chip:
                F.wide_prolong_enqueue(c._wide, f._wide, stream)
            if jobs:
                F.prolong_tables_enqueue(jobs, stream)
            if chip_jobs:
                F.wide_prolong_tables_enqueue(chip_jobs, stream)
            torch.cuda.current_stream(dev).synchronize()      # (the lock goes back with the CUs free)
    for _, f in pairs:
        f._post = None
