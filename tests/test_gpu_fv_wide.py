"""A lone finite-volume trial on the whole chip (mapping="chip", csrc/ldc_fv_wide.hip) on the GPU: one iteration's
intermediates read out of the work vectors and the upwind trajectories against the reference's fixtures (g14), the TVD
path against the NumPy restatement up to sizes the one-CU kernel does not take, bit equality across repeats, chunkings and
BiCGSTAB budgets, capped linear solves, solve() to the latch against the one-CU mapping, and the launcher."""
import ctypes as C
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"
sys.path.insert(0, str(Path(__file__).resolve().parent))
from fv_numpy import FVState  # noqa: E402

from conftest import PKG  # noqa: E402

pytestmark = pytest.mark.gpu

# work vectors (FvVec of csrc/ldc_fv_common.inc) that hold the intermediates of ldc_fv_step_debug
GPX, AP, XU, XV, C_RHS, Y, UP, VP, BU = 0, 2, 7, 8, 23, 26, 27, 28, 30


@pytest.fixture(scope="module")
def fv():
    import __graft_entry__ as g
    g.build()
    from solvers.fv.solver import FVSolver
    return FVSolver


def _make(FVSolver, m, **kw):
    args = dict(name="fv", Re=m["Re"], nx=m["nx"], ny=m["ny"], corner_treatment=m.get("lid", "none"),
                alpha_uv=m["alpha_uv"], alpha_p=m["alpha_p"], linear_solver_tol=m["linear_solver_tol"],
                convection_scheme=m["convection_scheme"], tolerance=1e-30, max_iterations=10**6, check_every=256,
                mapping="chip")
    args.update(kw)
    return FVSolver(**args)


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def _rows_rel(got, ref):
    """The largest relative deviation of the record entries E, Z, P, ... (0 where both are exactly 0)."""
    den = np.where(ref == 0.0, 1.0, np.abs(ref))
    return float(np.max(np.abs(got - ref) / den))


@pytest.mark.parametrize("tag", ["N16", "12x20"])
def test_one_iteration_from_the_work_vectors_matches_reference_intermediates(fv, tag):
    g = np.load(GOLD / "g14_fv_step.npz")
    m = json.loads((GOLD / "g14_fv_step.json").read_text())[tag]
    s = _make(fv, m)
    s.set_state(g[f"{tag}_u0"], g[f"{tag}_v0"], g[f"{tag}_p0"], g[f"{tag}_mdot0"])
    rows, done, total = s._advance(1)
    assert total == 1 and rows.shape == (1, 8) and np.all(np.isfinite(rows))
    n = s.n_cells
    w = s.t["work"].cpu().numpy()
    vec = lambda k, count=1: w[k * n: (k + count) * n]        # noqa: E731
    st = s.state()
    out = dict(grad_p=vec(GPX, 2), diag=vec(AP, 5), b=vec(BU, 2), u_star=vec(XU), v_star=vec(XV), rhs_p=vec(C_RHS),
               p_prime=vec(Y) - vec(Y)[0], u_prime=vec(UP), v_prime=vec(VP), mdot=st["mdot"])
    assert out["rhs_p"][0] == 0.0
    for k, v in out.items():
        assert np.all(np.isfinite(v)), k
        bound = 1e-8 if k == "p_prime" else 1e-10
        print(f"{tag} {k}: {_rel(v, g[f'{tag}_{k}']):.2e}")
        assert _rel(v, g[f"{tag}_{k}"]) <= bound, (k, _rel(v, g[f"{tag}_{k}"]))
    for k in ("u", "v", "p"):
        assert _rel(st[k], g[f"{tag}_{k}"]) <= 1e-10, k
    s.close()


@pytest.mark.parametrize("tag", ["N16", "12x20", "13x17 TVD"])
def test_assembly_leaves_the_same_bits_under_both_mappings(fv, tag):
    """The assembly of a cell is one function (csrc/ldc_fv_cells.inc) for the one-CU and the chip mapping, and its
    results depend on no sum over cells: after one iteration from the same state the nine work vectors grad p (2), the
    five diagonals and the deferred-correction sources b_u, b_v are equal bit for bit.  States: the two of g14_fv_step
    (Upwind) and the seeded 13 x 17 state of g15_fv_step under TVD (both signs of the face fluxes)."""
    if tag.endswith("TVD"):
        tag = tag.split()[0]
        g = np.load(GOLD / "g15_fv_step.npz")
        m = dict(json.loads((GOLD / "g15_fv_step.json").read_text())[tag], convection_scheme="TVD")
    else:
        g = np.load(GOLD / "g14_fv_step.npz")
        m = json.loads((GOLD / "g14_fv_step.json").read_text())[tag]
    seed = [g[f"{tag}_{k}0"] for k in ("u", "v", "p", "mdot")]
    left = {}
    for mapping in ("cu", "chip"):
        s = _make(fv, m, mapping=mapping, Lx=m.get("Lx", 1.0), Ly=m.get("Ly", 1.0),
                  lid_velocity=m.get("lid_velocity", 1.0))
        s.set_state(*seed)
        _, _, total = s._advance(1)
        assert total == 1
        n = s.n_cells
        w = s.t["work"].cpu().numpy()
        left[mapping] = {name: w[k * n: (k + count) * n].copy()
                         for name, (k, count) in dict(grad_p=(GPX, 2), diag=(AP, 5), b=(BU, 2)).items()}
        s.close()
    for name, v in left["cu"].items():
        assert np.all(np.isfinite(v)) and np.any(v != 0.0), name
        diff = float(np.max(np.abs(left["chip"][name] - v)))
        print(f"{tag} {m['convection_scheme']} {name}: max |chip - cu| = {diff:.2e}")
        assert np.array_equal(left["chip"][name], v), name


def test_upwind_trajectories_match_reference(fv):
    g = np.load(GOLD / "g14_fv_traj.npz")
    for tag, m in json.loads((GOLD / "g14_fv_traj.json").read_text()).items():
        s = _make(fv, m, max_iterations=m["K"])
        s.solve()
        ref = g[f"{tag}_rec"]
        assert s.history.shape == ref.shape
        print(f"{tag}: records {_rows_rel(s.history[:, :7], ref[:, :7]):.2e}")
        assert _rows_rel(s.history[:, :7], ref[:, :7]) <= 1e-8, tag
        st = s.state()
        for k in ("u", "v", "p", "mdot"):
            assert _rel(st[k], g[f"{tag}_{k}"]) <= 1e-8, (tag, k)
        s.close()


@pytest.mark.parametrize("nx,ny,Re,lid,K", [(16, 16, 100.0, "none", 60), (32, 24, 400.0, "saad", 80),
                                            (13, 17, 400.0, "none", 6), (8, 300, 400.0, "none", 6),
                                            (300, 9, 400.0, "saad", 6), (272, 260, 400.0, "none", 6)])
def test_tvd_trajectories_match_restatement(fv, nx, ny, Re, lid, K):
    """Fewer cells than threads, sizes that are no multiple of 16, thin rectangles, and sizes above 256."""
    m = dict(nx=nx, ny=ny, Re=Re, lid=lid, alpha_uv=0.4, alpha_p=0.2, linear_solver_tol=1e-12,
             convection_scheme="TVD")
    s = _make(fv, m, max_iterations=K)
    s.solve()
    o = FVState(nx, ny, Re, corner_treatment=lid, linear_solver_tol=1e-12, convection_scheme="TVD")
    rec = o.run(K)
    st = s.state()
    devs = {k: _rel(st[k], ref.ravel()) for k, ref in (("u", o.u), ("v", o.v), ("p", o.p))}
    print(f"{nx}x{ny}: records {_rows_rel(s.history[:, :7], rec[:, :7]):.2e}, fields {devs}, {s.counters()}")
    assert s.history.shape == rec.shape
    assert _rows_rel(s.history[:, :7], rec[:, :7]) <= 1e-9
    for k, d in devs.items():
        assert d <= 1e-9, k
    s.close()


def _run37(fv, chunks, graph=None, **kw):
    m = dict(nx=37, ny=50, Re=400.0, alpha_uv=0.4, alpha_p=0.2, linear_solver_tol=1e-9, convection_scheme="TVD")
    s = _make(fv, m, check_every=64, **kw)
    if graph is not None:
        s.set_wide_graph(graph)
    s._begin(1e-30)
    rows = np.concatenate([s._advance(k)[0] for k in chunks], axis=0)
    out = (rows, s.state(), s.counters())
    s.close()
    return out


def test_runs_repeat_bit_for_bit_whatever_the_chunks_and_the_budget(fv):
    rows, st, c = _run37(fv, [40])
    assert rows.shape == (40, 8) and c["iterations"] == 40 and c["linear_giveups"] == 0
    cases = dict(again=_run37(fv, [40]), chunks=_run37(fv, [7, 7, 7, 7, 7, 5]),
                 budget2=_run37(fv, [40], linear_budget=2), budget16=_run37(fv, [40], linear_budget=16),
                 eager=_run37(fv, [40], graph=False), graph=_run37(fv, [40], graph=True),
                 graph_chunks_budget2=_run37(fv, [7, 7, 7, 7, 7, 5], graph=True, linear_budget=2))
    for name, (rows2, st2, c2) in cases.items():
        assert np.array_equal(rows2, rows), name
        for k in ("u", "v", "p", "mdot"):
            assert np.array_equal(st2[k], st[k]), (name, k)
        for k in ("iterations", "linear_giveups", "linear_iterations", "momentum_solves"):
            assert c2[k] == c[k], (name, k)
    print(f"retries: default {c['linear_budget_retries']}, 2 -> {cases['budget2'][2]['linear_budget_retries']}, "
          f"16 -> {cases['budget16'][2]['linear_budget_retries']}; BiCGSTAB iterations {c['linear_iterations']} "
          f"in {c['momentum_solves']} solves")
    assert cases["budget2"][2]["linear_budget_retries"] > 0
    assert cases["budget16"][2]["linear_budget_retries"] == 0


def test_an_overflow_touches_neither_the_state_nor_the_control_words(fv):
    """One BiCGSTAB iteration is not enough at rtol 1e-9: the enqueue reports the overflow and leaves u, v, p, mdot and
    ctrl as they were; the same iterations enqueued again with enough budget then give what a run without overflow
    gives."""
    import torch
    from solvers.fv import ldc_fv_lib as F
    rows, st, _ = _run37(fv, [5])
    m = dict(nx=37, ny=50, Re=400.0, alpha_uv=0.4, alpha_p=0.2, linear_solver_tol=1e-9, convection_scheme="TVD")
    s = _make(fv, m, check_every=64)
    s._begin(1e-30)
    s._advance(2)
    before, ctrl = s.state(), s.t["ctrl"].cpu().numpy().copy()
    L, stream = F.lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.ldc_fv_wide_enqueue(s._wide, 3, 1, stream) == 0
    torch.cuda.synchronize()
    assert L.ldc_fv_wide_status(s._wide) == F.E_BUDGET
    assert np.array_equal(s.t["ctrl"].cpu().numpy(), ctrl)
    for k in ("u", "v", "p", "mdot"):
        assert np.array_equal(s.state()[k], before[k]), k
    assert L.ldc_fv_wide_enqueue(s._wide, 3, 16, stream) == 0
    torch.cuda.synchronize()
    assert L.ldc_fv_wide_status(s._wide) == 0
    assert np.array_equal(s.t["rec"][:3].cpu().numpy(), rows[2:])
    for k in ("u", "v", "p", "mdot"):
        assert np.array_equal(s.state()[k], st[k]), k
    s.close()


def test_capped_linear_solves_are_counted_as_the_one_cu_mapping_counts_them(fv, monkeypatch):
    import solvers.fv.solver as S
    monkeypatch.setattr(S, "LINEAR_MAX_ITERATIONS", 3)
    m = dict(nx=13, ny=17, Re=100.0, alpha_uv=0.4, alpha_p=0.2, linear_solver_tol=1e-12, convection_scheme="TVD")
    out = {}
    for mapping in ("cu", "chip"):
        s = _make(fv, m, mapping=mapping, max_iterations=30)
        s.solve()
        out[mapping] = (s.history.copy(), s.state(), s.counters())
        s.close()
    (h0, st0, c0), (h1, st1, c1) = out["cu"], out["chip"]
    print(f"cu {c0}\nchip {c1}")
    assert c0["linear_giveups"] > 0 and c1["linear_budget_retries"] == 0
    for k in ("iterations", "linear_giveups", "linear_iterations", "momentum_solves"):
        assert c1[k] == c0[k], k
    assert h1.shape == h0.shape == (30, 8)
    for k in ("u", "v", "p", "mdot"):
        assert _rel(st1[k], st0[k]) <= 1e-9, k


def test_solve_to_the_latch_agrees_with_the_one_cu_mapping(fv):
    """The stop rule bounds one iteration's change by 1e-6 (relative, fields of order 1); the runs may stop one
    iteration apart, and the margin is ten times that."""
    out = {}
    for mapping in ("cu", "chip"):
        s = fv(name="fv", Re=100.0, nx=32, ny=32, convection_scheme="TVD", alpha_uv=0.4, alpha_p=0.2,
               linear_solver_tol=1e-9, tolerance=1e-6, max_iterations=40000, check_every=256, mapping=mapping)
        s.solve()
        assert s.metrics.converged, mapping
        out[mapping] = (int(s.metrics.iterations), s.fields.u.copy(), s.fields.v.copy(), s.counters())
        s.close()
    (n0, u0, v0, c0), (n1, u1, v1, c1) = out["cu"], out["chip"]
    print(f"iterations cu {n0} chip {n1}; max|du| {np.max(np.abs(u1 - u0)):.2e} max|dv| {np.max(np.abs(v1 - v0)):.2e}")
    assert abs(n1 - n0) <= 1
    assert np.max(np.abs(u1 - u0)) <= 1e-5 and np.max(np.abs(v1 - v0)) <= 1e-5
    assert c1["done"] == 1 and c1["nan"] == 0 and c1["linear_giveups"] == 0


def test_chip_trial_keeps_postprocess_and_prolong_below_257_cells(fv):
    """Both handles exist at 24 x 24: the device streamfunction of a chip trial is that of the one-CU trial in the same
    state, and a chip trial can be started from another trial."""
    from solvers.fv.solver import prolong
    m = dict(nx=24, ny=24, Re=100.0, alpha_uv=0.4, alpha_p=0.2, linear_solver_tol=1e-9, convection_scheme="TVD")
    a, b = _make(fv, m), _make(fv, m, mapping="cu")
    a._begin(1e-30)
    a._advance(20)
    st = a.state()
    b.set_state(st["u"], st["v"], st["p"], st["mdot"])
    assert np.array_equal(a.streamfunction(), b.streamfunction())
    fine = _make(fv, dict(m, nx=40, ny=40))
    prolong([(a, fine)])
    assert np.all(np.isfinite(fine.state()["u"])) and np.max(np.abs(fine.state()["u"])) > 0
    for s in (a, b, fine):
        s.close()


def test_main_runs_a_chip_trial(tmp_path):
    r = subprocess.run([sys.executable, str(PKG / "main.py"), "solver=fv", "+solver.mapping=chip", "N=24", "Re=100"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    res = list(tmp_path.rglob("results.json"))
    assert res, r.stderr[-3000:]
    rec = json.loads(res[0].read_text())
    assert rec["solver"] == "fv" and rec["metrics"]["converged"] == 1
    assert rec["metrics"]["psi_min"] < 0 and rec["metrics"]["iterations"] > 10
