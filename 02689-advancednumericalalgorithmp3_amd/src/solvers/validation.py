"""Validation metrics and sweep objectives (host side, post-processing).

Contract: the callers of the hot path in the reference --
* ``compute_fv_l2_objective`` / ``compute_botella_vortex_objective`` / ``compute_optuna_objective``
  (main.py:142-225),
* the Botella & Peyret comparison table (``mlflow_log_validation_table``, base.py:890-964),
* the Ghia et al. centreline comparison, which the reference only *plots*
  (src/shared/plotting/ldc/validation.py:297-322); the numeric metric is defined in SURVEY.md 8(d).
"""
from __future__ import annotations

import csv
import logging
import math
from pathlib import Path

import numpy as np

from .spectral.basis.polynomial import spectral_interpolate

log = logging.getLogger(__name__)

DATA_DIR = Path(__file__).resolve().parents[2] / "data" / "validation"
GHIA_RE = (100, 400, 1000, 3200, 5000, 7500, 10000)


def _read_csv(path: Path) -> dict:
    rows = [ln for ln in Path(path).read_text().splitlines() if ln.strip() and not ln.lstrip().startswith("#")]
    rd = csv.DictReader(rows)
    cols = {k: [] for k in rd.fieldnames}
    for r in rd:
        for k, v in r.items():
            cols[k].append(float(v))
    return {k: np.array(v) for k, v in cols.items()}


def find_data_dir(*candidates) -> Path:
    """``data/validation`` relative to the CWD (the reference's convention) or the packaged copy."""
    for c in candidates + (Path("data/validation"), DATA_DIR):
        if c is not None and Path(c).exists():
            return Path(c)
    return DATA_DIR


def load_ghia(Re: int, data_dir=None):
    d = find_data_dir(data_dir) / "ghia"
    u = _read_csv(d / f"ghia_Re{int(Re)}_u_centerline.csv")
    v = _read_csv(d / f"ghia_Re{int(Re)}_v_centerline.csv")
    return (u["y"], u["u"]), (v["x"], v["v"])


def ghia_centerline_error(x_nodes, y_nodes, U, V, Re, data_dir=None, interpolation: str = "legendre") -> dict:
    """RMS and relative-L2 error of the centreline profiles at the tabulated Ghia points.

    U, V are [ix, iy].  u is taken on the grid line nearest x = centre (exact for even N),
    v on the line nearest y = centre, both interpolated with the Legendre-modal interpolant
    the reference uses for its Ghia plots of spectral fields; ``interpolation="linear"`` is its
    choice for FV fields (np.interp, constant beyond the outermost nodes;
    src/shared/plotting/ldc/validation.py:308-312)."""
    if interpolation not in ("legendre", "linear"):
        raise ValueError(f"interpolation={interpolation!r}: 'legendre' or 'linear'")
    (yu, ug), (xv, vg) = load_ghia(Re, data_dir)
    ic = int(np.argmin(np.abs(x_nodes - 0.5 * (x_nodes.min() + x_nodes.max()))))
    jc = int(np.argmin(np.abs(y_nodes - 0.5 * (y_nodes.min() + y_nodes.max()))))
    if interpolation == "linear":
        eu = np.interp(yu, y_nodes, U[ic, :]) - ug
        ev = np.interp(xv, x_nodes, V[:, jc]) - vg
    else:
        eu = spectral_interpolate(y_nodes, U[ic, :], yu, basis="legendre") - ug
        ev = spectral_interpolate(x_nodes, V[:, jc], xv, basis="legendre") - vg
    return dict(u_rms=float(np.sqrt(np.mean(eu**2))), v_rms=float(np.sqrt(np.mean(ev**2))),
                u_rel=float(np.linalg.norm(eu) / np.linalg.norm(ug)),
                v_rel=float(np.linalg.norm(ev) / np.linalg.norm(vg)),
                u_max=float(np.max(np.abs(eu))), v_max=float(np.max(np.abs(ev))))


# ------------------------------------------------------------------------------- objectives
def compute_fv_l2_objective(validation_errors: dict) -> float:
    """sqrt(u_L2_error^2 + v_L2_error^2); +inf when a key is missing (main.py:142-154)."""
    u = validation_errors.get("u_L2_error", float("inf"))
    v = validation_errors.get("v_L2_error", float("inf"))
    return math.sqrt(u**2 + v**2)


def load_botella(Re: int, data_dir=None) -> dict:
    path = find_data_dir(data_dir) / "botella" / f"botella_Re{int(Re)}_vortex.csv"
    if not path.exists():
        return {}
    cols = _read_csv(path)
    return {k: float(v[0]) for k, v in cols.items()}


def compute_botella_vortex_objective(metrics, Re: int, data_dir=None, strict_reference_objective: bool = False) -> float:
    """RMS of [|psi_min - ref| / |ref|, |x - x_ref|, |y - y_ref|]  (main.py:157-203).

    The reference reads the keys ``psi_min, psi_min_x, psi_min_y``; the Re=1000 table uses
    ``psi_primary, x_primary, y_primary`` (magnitudes, and x in the mirrored frame of Botella &
    Peyret), so the reference objective there is a constant +inf.
    ``strict_reference_objective=True`` reproduces that; the default maps the evident intent."""
    ref = load_botella(Re, data_dir)
    if not ref:
        return float("inf")
    if not strict_reference_objective and "psi_min" not in ref and "psi_primary" in ref:
        ref = dict(ref, psi_min=-abs(ref["psi_primary"]), psi_min_x=1.0 - ref["x_primary"],
                   psi_min_y=ref["y_primary"])
    errs = []
    if ref.get("psi_min"):
        errs.append(abs(metrics.psi_min - ref["psi_min"]) / abs(ref["psi_min"]))
    if ref.get("psi_min_x"):
        errs.append(abs(metrics.psi_min_x - ref["psi_min_x"]))
    if ref.get("psi_min_y"):
        errs.append(abs(metrics.psi_min_y - ref["psi_min_y"]))
    return math.sqrt(sum(e * e for e in errs) / len(errs)) if errs else float("inf")


def compute_optuna_objective(objective: str, validation_errors: dict, solver, Re: int, **kw) -> float:
    if objective == "multi":
        raise ValueError(
            "Multi-objective optimization is not supported by hydra-optuna-sweeper 1.x. "
            "Use objective=fv_l2_error or objective=botella_vortex instead.")
    if objective == "botella_vortex":
        return compute_botella_vortex_objective(solver.metrics, int(Re), **kw)
    return compute_fv_l2_objective(validation_errors)


def botella_table(metrics, Re: int, data_dir=None) -> list:
    """Rows of the comparison table the reference logs to MLflow (base.py:920-962)."""
    ref = load_botella(Re, data_dir)
    if not ref:
        return []
    rows = []

    def add(vortex, name, computed, reference, fmt=".6f"):
        if reference:
            err = abs(abs(computed) - abs(reference)) / abs(reference) * 100
            ref_s = f"{reference:{fmt}}" if abs(reference) >= 1e-3 else f"{reference:.4e}"
            err_s = f"{err:.2f}"
        else:
            ref_s, err_s = "-", "-"
        comp_s = f"{computed:{fmt}}" if abs(computed) >= 1e-3 else f"{computed:.4e}"
        rows.append({"Vortex": vortex, "Metric": name, "Computed": comp_s, "Botella": ref_s, "Error (%)": err_s})

    m = metrics
    add("Primary", "|ψ|", abs(m.psi_min), ref.get("psi_primary"))
    add("Primary", "|ω|", abs(m.omega_center), ref.get("omega_primary"))
    add("Primary", "x", m.psi_min_x, ref.get("x_primary"))
    add("Primary", "y", m.psi_min_y, ref.get("y_primary"))
    for tag in ("BL", "BR"):
        add(tag, "|ψ|", abs(getattr(m, f"psi_{tag}")), ref.get(f"psi_{tag}"))
        add(tag, "|ω|", abs(getattr(m, f"omega_{tag}")), ref.get(f"omega_{tag}"))
        add(tag, "x", getattr(m, f"psi_{tag}_x"), ref.get(f"x_{tag}"))
        add(tag, "y", getattr(m, f"psi_{tag}_y"), ref.get(f"y_{tag}"))
    return rows
