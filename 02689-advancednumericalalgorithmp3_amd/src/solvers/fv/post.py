"""Post-processing of finite-volume trials on the device: omega, psi and the vortex extrema.

``vortex_metrics="device"`` (``ldc_fv_post_enqueue``, one work-group per trial) and ``"chip"`` (``ldc_fv_wide_post_enqueue``,
the whole chip per trial, for ``mapping="chip"`` and ``"shared"`` trials of up to 1024 cells per axis, the same bits as
``"device"`` where both exist) compute what the host route does by the same rules.  ``streamfunction="wall"`` reads the
vortices by a second-order rule instead (psi = 0 on the wall faces, the lid profile in omega's ghost row;
``vortex_refine="quadratic"``: sub-cell centres), always on the device and for every mapping and size
(``ldc_fv_wall_post_enqueue``: the wall trials of a call share seven launches per 24 of them);
``streamfunction="wall_stretched"`` is that rule on the mesh of ``grid="tanh"`` (``ldc_fv_wall_stretched_post_enqueue``: the
Dirichlet generalised eigenpairs of each axis, the quadratic fit with unequal spacing; seven launches per 32 trials).
``postprocess`` takes trials of all routes in one call; what it asks of a trial is its flags, tensors and job builders, so
this module does not know ``FVSolver``."""
from __future__ import annotations

from . import ldc_fv_lib as F
from .grids import device_index, sine_eig
from .options import WALL_RULES


def post_route(vortex_metrics: str, has_cu_handle: bool, streamfunction: str = "reference") -> str:
    """The entry that post-processes a trial: ``"wall"`` (``ldc_fv_wall_post_enqueue``, launches shared by the wall trials
    of the call) for a ``streamfunction="wall"`` trial, whatever ``vortex_metrics`` says and for every mapping and size,
    ``"wall_stretched"`` (``ldc_fv_wall_stretched_post_enqueue``, likewise) for a ``streamfunction="wall_stretched"`` one;
    else ``"chip"`` (``ldc_fv_wide_post_enqueue``, a chain of launches over the
    whole chip for this trial alone) when the trial asks for it or has no one-CU handle, else ``"cu"``
    (``ldc_fv_post_enqueue``, one work-group, beside the other such trials of the call)."""
    if streamfunction in WALL_RULES:
        return streamfunction
    return "chip" if vortex_metrics == "chip" or not has_cu_handle else "cu"


def postprocess(trials):
    """omega, psi and the vortex extrema of ``trials`` (FVSolvers on one device, none in flight) on the device: one
    launch per 256 trials of the one-CU route, one chain of launches per trial of the chip route, one chain per 24
    trials of the wall route and one per 32 of the stretched wall route (``post_route``), then ONE copy of all result blocks (rows of ``WALL_RESULT_LEN`` doubles when
    the call has a wall trial: the ``POST_*`` slots come first either way).  ``psi`` and ``omega`` stay on the device as ``t["psi"]``, ``t["omega"]``; every
    trial keeps its row of the result blocks for ``compute_vortex_metrics``."""
    import torch
    from solvers.spectral import ldc_lib
    if not trials:
        return
    for s in trials:
        if s.stretched and not getattr(s, "stretched_wall", False):
            raise ValueError("postprocess: grid='tanh' trials with streamfunction='reference' are post-processed on the host "
                             "(those device kernels assume equal spacing); give the trial vortex_metrics='host', or "
                             "streamfunction='wall_stretched'")
    routes = [post_route(s.params.vortex_metrics, s._has_cu_handle, s.params.streamfunction) for s in trials]
    for s, route in zip(trials, routes):
        if route == "cu":
            s._require_cu_handle("postprocess")
        elif route == "chip" and s._wide is None:
            raise ValueError(f"postprocess: a trial of {s.nx} x {s.ny} cells with mapping={s.params.mapping!r} has no "
                             f"whole-chip handle")
    dev = trials[0].device
    index = device_index(dev)
    with torch.cuda.device(dev):
        width = F.WALL_RESULT_LEN if "wall" in routes or "wall_stretched" in routes else F.POST_RESULT_LEN
        results = torch.zeros((len(trials), width), dtype=torch.float64, device=dev)
        posts, jobs, stretched_jobs = [], [], []
        for q, s in enumerate(trials):
            if device_index(s.device) != index:
                raise ValueError("postprocess: all trials must be on one device")
            if routes[q] == "wall":
                posts.append(None)
                jobs.append(s._wall_job(results[q].data_ptr()))
                continue
            if routes[q] == "wall_stretched":
                posts.append(None)
                stretched_jobs.append(s._wall_stretched_job(results[q].data_ptr()))
                continue
            lamx, Sx = sine_eig(s.nx - 2, dev)
            lamy, Sy = sine_eig(s.ny - 2, dev)
            for name in ("psi", "omega"):
                if name not in s.t:
                    s.t[name] = torch.zeros(s.n_cells, dtype=torch.float64, device=dev)
            ix_lt, ix_gt, jy_lt, jy_gt = s._mask_bounds
            posts.append(F.Post(Sx=Sx.data_ptr(), lamx=lamx.data_ptr(), Sy=Sy.data_ptr(), lamy=lamy.data_ptr(),
                                ix_lt=ix_lt, ix_gt=ix_gt, jy_lt=jy_lt, jy_gt=jy_gt, psi=s.t["psi"].data_ptr(),
                                omega=s.t["omega"].data_ptr(), result=results[q].data_ptr()))
        cu = [q for q, route in enumerate(routes) if route == "cu"]
        chip = [q for q, route in enumerate(routes) if route == "chip"]
        for q in chip:
            if "post_scratch" not in trials[q].t:
                trials[q].t["post_scratch"] = torch.zeros(F.wide_post_scratch_len(trials[q].nx, trials[q].ny),
                                                          dtype=torch.float64, device=dev)
        with ldc_lib.resident_lock(index):
            stream = torch.cuda.current_stream(dev).cuda_stream
            for lo in range(0, len(cu), F.LAUNCH_MAX):
                part = cu[lo: lo + F.LAUNCH_MAX]
                F.post_enqueue([trials[q].handle for q in part], [posts[q] for q in part], stream)
            for q in chip:
                scratch = trials[q].t["post_scratch"]
                F.wide_post_enqueue(trials[q]._wide, posts[q], scratch.data_ptr(), scratch.numel(), stream)
            if jobs:
                F.wall_post_enqueue(jobs, stream)
            if stretched_jobs:
                F.wall_stretched_post_enqueue(stretched_jobs, stream)
            rows = results.cpu().numpy()          # (synchronises the stream)
    for s, row in zip(trials, rows):
        s._post = row.copy()
