"""A spectral trial started from a finite-volume solution of the same cavity (``initial_guess="fv"``).

The spectral solver's cost is its iteration count (59 649 pseudo-time iterations from rest at N = 32, Re = 100); the
finite-volume solver converges the same cavity in a few hundred SIMPLE iterations.  ``start_from_fv`` moves FV states to
the collocation nodes of spectral trials on the device (``ldc_fv_sample_nodes``, include/ldc_fv.h: the bilinear
interpolant of the ring-extended FV field at the interior nodes, the spectral trial's own boundary values on the
boundary) and hands them to ``SGSolver.set_state_device``; the spectral iteration itself is not touched.

``seed_alone`` and ``seed_together`` are what ``SGSolver.solve`` and ``BatchedSGSolver.solve`` call for trials with
``initial_guess="fv"``: build the FV trial(s) of the same Re, lid, domain and corner treatment (``seed_kwargs``), run them
to ``initial_guess_tolerance``, transfer, close.  A seed that ends on a NaN or at its cap without latching is logged and
its spectral trial starts from rest: a failed seed is never an error of the spectral trial.
"""
from __future__ import annotations

import logging
import time

log = logging.getLogger(__name__)

INITIAL_GUESSES = ("rest", "fv")
SEED_MIN_CELLS = 16               # initial_guess_cells = 0: max(SEED_MIN_CELLS, N) cells per axis
SEED_MAX_ITERATIONS = 20000       # the seed's cap: ten times what a 64 x 64 seed needs at 0.7 / 0.3
SEED_CHECK_EVERY = 256            # iterations per chunk of a seed (a latched chip trial's launches are empty, not free)
SEED_LINEAR_TOL = 1e-9            # conf/solver/fv.yaml's, the one the counts of DESIGN.md 3 were taken with


def validate(params) -> None:
    """The keys of ``SpectralParameters`` that belong to the initial guess; needs no device."""
    if params.initial_guess not in INITIAL_GUESSES:
        raise ValueError(f"Unknown initial_guess: {params.initial_guess!r}. Use one of {INITIAL_GUESSES}")
    if params.initial_guess == "rest":
        return
    if str(params.multigrid).lower() == "fsg":
        raise ValueError("initial_guess='fv' with multigrid='fsg': the sequence starts on its coarsest level, which "
                         "takes no finite-volume seed yet; use multigrid='none' or initial_guess='rest'")
    cells = int(params.initial_guess_cells)
    if cells != 0 and not 8 <= cells <= 1024:
        raise ValueError(f"initial_guess_cells={cells}: 0 (max({SEED_MIN_CELLS}, N) per axis) or 8 ... 1024")
    if not float(params.initial_guess_tolerance) > 0:
        raise ValueError(f"initial_guess_tolerance={params.initial_guess_tolerance}: a relative change, above 0")
    for key in ("initial_guess_alpha_uv", "initial_guess_alpha_p"):
        if not 0.0 < float(getattr(params, key)) <= 1.0:
            raise ValueError(f"{key}={getattr(params, key)}: an under-relaxation factor in (0, 1]")


def seed_cells(params) -> tuple:
    """Cells per axis of the seed: ``initial_guess_cells`` on both, or with 0 each axis by its own order."""
    cells = int(params.initial_guess_cells)
    if cells:
        return cells, cells
    return max(SEED_MIN_CELLS, int(params.nx)), max(SEED_MIN_CELLS, int(params.ny))


def seed_kwargs(params, mapping: str) -> dict:
    """Keyword arguments of the FVSolver that seeds a spectral trial with ``params``: the same Re, lid velocity, domain
    and corner treatment; TVD, the consistent pressure equation, the relaxation and tolerance of the initial_guess_* keys."""
    nx, ny = seed_cells(params)
    return dict(name="fv", Re=float(params.Re), lid_velocity=float(params.lid_velocity), Lx=float(params.Lx),
                Ly=float(params.Ly), nx=nx, ny=ny, corner_treatment=params.corner_treatment,
                corner_smoothing=float(params.corner_smoothing), convection_scheme="TVD", limiter="MUSCL",
                alpha_uv=float(params.initial_guess_alpha_uv), alpha_p=float(params.initial_guess_alpha_p),
                linear_solver_tol=SEED_LINEAR_TOL, tolerance=float(params.initial_guess_tolerance),
                max_iterations=SEED_MAX_ITERATIONS, check_every=SEED_CHECK_EVERY, mapping=mapping,
                pressure_equation="consistent", vortex_metrics="host", device=str(params.device))


def _same_extent(a: float, b: float) -> bool:
    return abs(a - b) <= 1e-12 * max(abs(a), abs(b))


def start_from_fv(pairs) -> None:
    """The state of every spectral trial from its finite-volume trial: ``pairs`` of (FVSolver, SGSolver) on one device
    and one domain each, neither in flight.  ONE ``ldc_fv_sample_nodes`` call for all pairs under the device's resident
    lock, then ``set_state_device`` per spectral trial (the packing, the stage buffers and the tail layout's edges).  Any
    FV mapping, Chebyshev and Legendre nodes, nx != ny and every ``persistent`` mode.  A pair on two domains (Lx or Ly
    differ beyond 1e-12 relative) is a ``ValueError`` before anything is launched."""
    import torch
    from solvers.fv import ldc_fv_lib as F
    from . import ldc_lib
    pairs = list(pairs)
    if not pairs:
        return
    dev = pairs[0][1].device
    index = torch.cuda.current_device() if dev.index is None else dev.index
    for fv, sg in pairs:
        if not (_same_extent(fv.nx * fv.dx_min, float(sg.params.Lx)) and _same_extent(fv.ny * fv.dy_min, float(sg.params.Ly))):
            raise ValueError(f"start_from_fv: the finite-volume trial covers {fv.nx * fv.dx_min:g} x {fv.ny * fv.dy_min:g}, "
                             f"the spectral trial Lx, Ly = {sg.params.Lx:g}, {sg.params.Ly:g}: two domains")
        for s in (fv, sg):
            if (torch.cuda.current_device() if s.device.index is None else s.device.index) != index:
                raise ValueError("start_from_fv: all trials must be on one device")
    with torch.cuda.device(dev):
        sizes = [(sg.Mx * sg.My, (sg.Mx - 2) * (sg.My - 2)) for _, sg in pairs]
        out = torch.empty(sum(2 * full + inner for full, inner in sizes), dtype=torch.float64, device=dev)
        jobs, views, lo = [], [], 0
        for (fv, sg), (full, inner) in zip(pairs, sizes):
            U, V, P = out[lo: lo + full], out[lo + full: lo + 2 * full], out[lo + 2 * full: lo + 2 * full + inner]
            lo += 2 * full + inner
            views.append((U.view(sg.Mx, sg.My), V.view(sg.Mx, sg.My), P.view(sg.Mx - 2, sg.My - 2)))
            jobs.append(F.SampleJob(u=fv.t["u"].data_ptr(), v=fv.t["v"].data_ptr(), p=fv.t["p"].data_ptr(),
                                    ulid=fv.t["ulid"].data_ptr(), nx=fv.nx, ny=fv.ny, dx=fv.dx_min, dy=fv.dy_min,
                                    x=sg.d["x"].data_ptr(), y=sg.d["y"].data_ptr(), ulid_nodes=sg.d["ulid"].data_ptr(),
                                    Mx=sg.Mx, My=sg.My, U=U.data_ptr(), V=V.data_ptr(), P=P.data_ptr()))
        with ldc_lib.resident_lock(index):
            F.sample_nodes(jobs, torch.cuda.current_stream(dev).cuda_stream)
            torch.cuda.current_stream(dev).synchronize()      # (the lock goes back with the CUs free)
        for (_, sg), (U, V, P) in zip(pairs, views):
            sg.set_state_device(U, V, P)


# ---------------------------------------------------------------------------------------------- the seeds of solve()
def _info(fv, iterations: int, wall: float, latched: bool, nan: bool) -> dict:
    ok = bool(latched) and not nan
    reason = "" if ok else ("the seed produced a NaN" if nan else f"the seed did not reach its tolerance in {iterations} iterations")
    return dict(cells=(int(fv.nx), int(fv.ny)), iterations=int(iterations), wall_time_seconds=float(wall),
                converged=bool(latched), used=ok, reason=reason)


def _report(sg, info: dict) -> None:
    sg.initial_guess_info = info
    if info["used"]:
        log.info("initial guess: finite-volume seed of %d x %d cells, %d iterations, %.3f s", *info["cells"],
                 info["iterations"], info["wall_time_seconds"])
    else:
        log.warning("initial guess: finite-volume seed of %d x %d cells failed (%s); the trial starts from rest",
                    *info["cells"], info["reason"])


def _lone_trial(kwargs: dict):
    from solvers.fv.solver import FVSolver
    return FVSolver(**kwargs)


def run_lone(fv) -> tuple:
    """A lone FV trial to its tolerance or its cap, without the post-processing of ``solve()``: (latch, nan, iterations)."""
    from . import ldc_lib
    cap = int(fv.params.max_iterations)
    fv._begin(fv.params.tolerance)
    done, total = 0, 0
    try:
        while total < cap and not done:
            _, done, new_total = fv._advance(min(fv.rec_cap, cap - total))
            if new_total == total:
                raise RuntimeError("device loop made no progress")
            total = new_total
    except ldc_lib.LdcError as exc:              # (what a lone _advance raises for a NaN: ldc_fv_wide_status)
        if int(fv.counters()["nan"]) == 0:
            raise
        log.debug("seed: %s", exc)
        return 0, 1, int(fv.counters()["iterations"])
    return int(done), 0, int(total)


def seed_alone(sg, make_trial=None, transfer=None) -> None:
    """The seed of ONE spectral trial: an FV trial of ``mapping="chip"``, solved, transferred (``start_from_fv``) and
    closed.  ``sg.initial_guess_info`` says what it took; a failed seed leaves the trial at rest."""
    make_trial = _lone_trial if make_trial is None else make_trial
    transfer = start_from_fv if transfer is None else transfer
    t0 = time.perf_counter()
    fv = make_trial(seed_kwargs(sg.params, "chip"))
    try:
        latch, nan, total = run_lone(fv)
        ok = bool(latch) and not nan
        if ok:
            transfer([(fv, sg)])
        else:
            sg.reset_state()
    finally:
        fv.close()
    _report(sg, _info(fv, total, time.perf_counter() - t0, latch, nan))


class _SharedSeeds:
    """The seeds of a batch as ONE ``BatchedFVSolver`` of ``mapping="shared"`` trials, run without the post-processing of
    its ``solve()``."""

    def __init__(self, trials: list):
        from solvers.fv.batched import BatchedFVSolver
        self.batch = BatchedFVSolver(trials)
        self.solvers = self.batch.solvers

    def run(self) -> list:
        """Per trial (latch, nan, iterations)."""
        from solvers.fv.batched import run_chunks
        for s in self.solvers:
            s._begin(s.params.tolerance)
        out = run_chunks([s.rec_cap for s in self.solvers], [int(s.params.max_iterations) for s in self.solvers],
                         self.batch._step)
        return [(latch, nan, total) for latch, nan, total, _ in out]

    def close(self):
        self.batch.close()


SHARED_MAX = 256                  # LDC_FV_WIDE_BATCH_MAX: trials of one shared batch


def seed_together(solvers, make_batch=None, transfer=None) -> float:
    """The seeds of every trial of ``solvers`` that asks for one: ONE batch of ``mapping="shared"`` FV trials (one per
    ``SHARED_MAX`` trials), then ONE ``start_from_fv`` call for the seeds that latched; a seed that failed leaves its own
    trial at rest and disturbs nobody.  A trial's ``initial_guess_info`` carries the batch's wall time in proportion to
    its seed's work (iterations x cells).  Returns the wall time of the lot."""
    todo = [s for s in solvers if getattr(s.params, "initial_guess", "rest") == "fv"]
    if not todo:
        return 0.0
    make_batch = _SharedSeeds if make_batch is None else make_batch
    transfer = start_from_fv if transfer is None else transfer
    t0 = time.perf_counter()
    for lo in range(0, len(todo), SHARED_MAX):
        part = todo[lo: lo + SHARED_MAX]
        t1 = time.perf_counter()
        batch = make_batch([seed_kwargs(s.params, "shared") for s in part])
        try:
            out = batch.run()
            good = [(fv, sg) for fv, sg, (latch, nan, _) in zip(batch.solvers, part, out) if latch and not nan]
            if good:
                transfer(good)
            for sg, (latch, nan, _) in zip(part, out):
                if not (latch and not nan):
                    sg.reset_state()
        finally:
            batch.close()
        wall = time.perf_counter() - t1
        work = [max(1, total) * fv.nx * fv.ny for fv, (_, _, total) in zip(batch.solvers, out)]
        for fv, sg, (latch, nan, total), w in zip(batch.solvers, part, out, work):
            _report(sg, _info(fv, total, wall * w / sum(work), latch, nan))
    return time.perf_counter() - t0
