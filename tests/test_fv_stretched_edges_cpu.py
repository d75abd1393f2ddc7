"""CPU side of tests/test_gpu_fv_stretched_edges.py: the work-vector layout that tests/fv_stretched_probe.py reads is pinned
against the device sources, and every restatement run that a GPU test compares with is made here once and its preconditions
asserted (finite rows, the BiCGSTAB and CG exits that the case is about, seeded states with both signs among the face fluxes).
The case lists are the probe's: the GPU file imports the same ones."""
import re

import numpy as np
import pytest

from conftest import PKG  # noqa: E402
import fv_stretched_probe as P

CSRC = PKG / "csrc"


# ---------------------------------------------------------------------------------------------- the layout
def _enum_fvvec():
    text = (CSRC / "ldc_fv_common.inc").read_text()
    body = re.search(r"enum FvVec \{(.*?)\};", text, re.S).group(1)
    names = [w for w in re.sub(r"//[^\n]*", "", body).replace("\n", " ").split(",") if w.strip()]
    return {name.strip(): k for k, name in enumerate(names)}


def _aliases(text, names):
    """``NAME = FV_...`` of a ``constexpr FvVec`` line."""
    out = {}
    for line in text.splitlines():
        if line.startswith("constexpr FvVec "):
            out.update(re.findall(r"(\w+) = (FV_\w+)", line))
    assert set(names) <= set(out), (names, out)
    return {k: out[k] for k in names}


def test_the_probe_reads_the_vectors_the_kernels_write():
    enum = _enum_fvvec()
    assert enum["FV_GPX"] == 0 and enum["FV_NVEC"] == len(enum) - 1 == 32
    pcg = _aliases((CSRC / "ldc_fv_pressure_cells.inc").read_text(), ("PCG_MS", "PCG_R", "PCG_Z", "PCG_P", "PCG_Q"))
    sep = _aliases((CSRC / "ldc_fv_stretched_sep.hip").read_text(), ("SEP_S", "SEP_SR"))
    index = dict(enum, **{k: enum[v] for k, v in dict(pcg, **sep).items()})
    for name, k in P.INDEX.items():
        assert index[name] == k, (name, index[name], k)
    # the table of the work vectors, number by number
    want = dict(grad_p=(0, 1), diag=(2, 3, 4, 5, 6), b=(30, 31), u_star=(7,), v_star=(8,), mdot_star=(9,), rhs_p=(23,),
                p_prime=(26,), u_prime=(27,), v_prime=(28,), omega=(29,), sep_s=(15,), cg_r=(12,))
    assert {k: tuple(P.INDEX[n] for n in v) for k, v in P.VEC.items()} == want
    # mdot* spreads over PCG_MS and the two vectors behind it, which end where the CG residual begins; s and s . r are
    # clear of everything the probe reads
    assert index["PCG_MS"] + P.MS_VECTORS == index["PCG_R"]
    for nx, ny in ((8, 8), (8, 256), (256, 256)):
        assert ny * (nx + 1) + (ny + 1) * nx <= P.MS_VECTORS * nx * ny
    read = {k for v in want.values() for k in v} | {10, 11}
    assert index["SEP_SR"] not in read and len(read) == sum(len(v) for v in want.values()) + 2
    assert set(P.STEP_KEYS) <= set(P.VEC) | {"mdot"}


def test_the_case_lists_hold_the_planned_cases():
    assert [(nx, ny, beta, K) for nx, ny, beta, _, K in P.SHAPES] == [
        (37, 50, 1.0, 12), (131, 77, 1.5, 6), (8, 256, 1.5, 6), (256, 8, 1.5, 6), (24, 40, 2.5, 12), (255, 253, 1.5, 3),
        (256, 256, 1.5, 3)]
    assert dict(P.SHAPES[0][3]) == dict(Lx=2.0, Ly=0.5, lid_velocity=2.0) and all(not s[3] for s in P.SHAPES[1:])
    assert P.SHAPE_TOL == dict(linear_solver_tol=1e-12, pressure_tol=1e-13, pressure_max_iters=2000) and P.SHAPE_RE == 400.0
    assert min(K for *_, K in P.SHAPES) >= 2
    assert P.PHASE_TOL == dict(linear_solver_tol=1e-12, pressure_tol=1e-13) and P.PHASE_MORE == 10
    assert P.COUNTS[:3] == (24, 40, 2.5) and P.COUNTS in P.SHAPES
    assert (P.SMALL["nx"], P.SMALL["ny"], P.SMALL["beta"], P.SMALL["K"]) == (13, 17, 1.5, 30)
    assert (P.CAPPED_CG["pressure_tol"], P.CAPPED_CG["pressure_max_iters"]) == (1e-10, 3)
    assert P.CAPPED_LINEAR["max_lin_iters"] == 3 and P.LOOSE["linear_solver_tol"] == 1e-6
    c = P.NAN_CASE
    assert (c["nx"], c["ny"], c["beta"], c["Re"], c["alpha_uv"], c["alpha_p"]) == (16, 16, 1.5, 1000.0, 1.0, 1.0)
    # more than one stride of the 512 threads where a case is there for that
    assert 37 * 50 > 3 * 512 and 24 * 40 > 512 and 13 * 17 < 512


# ---------------------------------------------------------------------------------------------- a. phases
@pytest.mark.parametrize("consistent", [False, True], ids=["reference", "consistent"])
@pytest.mark.parametrize("tag", P.PHASE_TAGS)
def test_phase_references_are_finite_and_seeded_with_both_signs(tag, consistent):
    m, seed = P.phase_case(tag)
    assert (m["nx"], m["ny"], m["beta"]) == dict([("13x17", (13, 17, 1.5)), ("37x50", (37, 50, 1.0))])[tag]
    if tag == "37x50":
        assert (m["Lx"], m["Ly"], m["lid_velocity"], m["Re"]) == (2.0, 0.5, 2.0, 400.0)
    nx, ny = m["nx"], m["ny"]
    fx, fy = seed[3][: ny * (nx + 1)].reshape(ny, nx + 1), seed[3][ny * (nx + 1):].reshape(ny + 1, nx)
    for inner in (fx[:, 1:-1], fy[1:-1, :]):               # both signs among the inner faces of either direction
        assert (inner > 0).sum() >= inner.size // 8 and (inner < 0).sum() >= inner.size // 8
    r = P.phase_reference(tag, consistent)
    assert set(r["cap"]) == set(P.STEP_KEYS)
    for k, v in r["cap"].items():
        assert np.all(np.isfinite(v)), k
    assert np.all(np.isfinite(r["row"])) and np.all(np.isfinite(r["omega"])) and np.all(np.isfinite(r["rows"]))
    assert r["rows"].shape == (P.PHASE_MORE, 8) and len(r["exits"]) == 2 * (1 + P.PHASE_MORE)
    assert "cap" not in r["exits"]
    assert r["cap"]["rhs_p"][0] == 0.0
    if consistent:
        ms, md = r["cap"]["mdot_star"], r["cap"]["mdot"]
        for f in (ms, md):
            gx, gy = f[: ny * (nx + 1)].reshape(ny, nx + 1), f[ny * (nx + 1):].reshape(ny + 1, nx)
            assert not gx[:, 0].any() and not gx[:, -1].any() and not gy[0].any() and not gy[-1].any()
        assert r["lam1"] > 0 and r["s"].shape == (nx * ny,) and np.all(r["s"] > 0)
        assert abs(r["b"].sum()) <= 64 * np.finfo(float).eps * np.abs(r["b"]).sum()


# ---------------------------------------------------------------------------------------------- b. edge shapes
@pytest.mark.parametrize("shape", P.SHAPES, ids=P.SHAPE_IDS)
def test_shape_references_are_finite_and_uncapped(shape):
    """The three restatement runs of a shape.  The two consistent ones solve the same equation to pressure_tol with two
    preconditioners: their distance is the solver-tolerance noise of the reference side (7e-15 in the fields, 1e-14 in the
    record columns when the cases were chosen), far inside the 1e-9 that the card is held to."""
    nx, ny, beta, geo, K = shape
    runs = {kernel: P.shape_reference(*shape, kernel) for kernel in P.KERNELS}
    for kernel, r in runs.items():
        assert r["rows"].shape == (K, 8) and np.all(np.isfinite(r["rows"])), kernel
        assert all(np.all(np.isfinite(v)) for v in r["state"].values()), kernel
        assert "cap" not in r["exits"] and len(r["exits"]) == 2 * K, kernel
        assert r["cg_caps"] == 0 and len(r["cg_iters"]) == (0 if kernel == "reference" else K), kernel
    a, b = runs["laplacian"], runs["separable"]
    cols = [0, 1, 2, 4, 5, 6]
    fields = max(float(np.max(np.abs(a["state"][k] - b["state"][k]))) for k in a["state"])
    rows = float(np.max(np.abs(a["rows"][:, cols] - b["rows"][:, cols]) / np.abs(b["rows"][:, cols])))
    print(f"{nx}x{ny}: laplacian against separable restatement: fields {fields:.1e}, record columns {rows:.1e}; CG "
          f"{a['cg_iters'][-1]} and {b['cg_iters'][-1]}")
    assert fields <= 1e-11 and rows <= 1e-11


# ---------------------------------------------------------------------------------------------- c. CG counts
def test_count_references_do_not_cap():
    sep, lap = P.counts_reference("separable"), P.counts_reference("laplacian")
    K = P.COUNTS[4]
    for r in (sep, lap):
        assert r["cg_caps"] == 0 and len(r["cg_iters"]) == K and np.all(np.isfinite(r["rows"])) and "cap" not in r["exits"]
    print("separable", sep["cg_iters"], "laplacian", lap["cg_iters"])
    assert 20 <= min(sep["cg_iters"]) and max(sep["cg_iters"]) <= 35
    assert 400 <= min(lap["cg_iters"]) and max(lap["cg_iters"]) <= 480 < P.SHAPE_TOL["pressure_max_iters"]


@pytest.mark.parametrize("kernel", ["separable", "laplacian"])
def test_the_count_bound_rests_on_the_restatements_own_sensitivity(kernel):
    """The bound of tests/test_gpu_fv_stretched_edges.py::test_cg_counts_follow_the_restatement_at_beta_2_5: one for the
    separable preconditioner, whose counts do not move with the restatement's linear_solver_tol; ten times the measured 2 for
    the laplacian one."""
    assert P.counts_sensitivity(kernel) == P.COUNT_SENSITIVITY[kernel]
    assert P.count_bound(kernel) == dict(separable=1, laplacian=20)[kernel]


# ---------------------------------------------------------------------------------------------- d, e. the exits
@pytest.mark.parametrize("kernel", ["laplacian", "separable"])
def test_the_capped_cg_reference_caps_every_solve(kernel):
    r = P.capped_cg_reference(kernel)
    K = P.SMALL["K"]
    assert r["cg_caps"] == K == 30 and r["cg_iters"] == (3,) * K and sum(r["cg_iters"]) == 90
    assert np.all(np.isfinite(r["rows"])) and "cap" not in r["exits"]


@pytest.mark.parametrize("kernel", P.KERNELS)
def test_the_capped_bicgstab_reference_gives_up_59_times(kernel):
    r = P.capped_linear_reference(kernel)
    assert r["exits"].count("cap") == 59 and r["exits"].count("b0") == 1 and sum(r["iters"]) == 177
    assert np.all(np.isfinite(r["rows"])) and r["cg_caps"] == 0


@pytest.mark.parametrize("kernel", P.KERNELS)
def test_the_loose_reference_has_both_exits_and_unequal_counts(kernel):
    r = P.loose_reference(kernel)
    it = np.array(r["iters"]).reshape(-1, 2)
    assert "r" in r["exits"] and "s" in r["exits"] and "cap" not in r["exits"] and r["cg_caps"] == 0
    assert int((it[:, 0] != it[:, 1]).sum()) >= 10
    assert np.all(np.isfinite(r["rows"]))


# ---------------------------------------------------------------------------------------------- f. the NaN latch
@pytest.mark.parametrize("kernel", P.KERNELS)
def test_the_nan_case_goes_non_finite_within_a_chunk(kernel):
    at = P.nan_reference(kernel)
    assert at == P.NAN_AT[kernel] and at + 1 < P.nan_solver_kwargs(kernel)["check_every"]


# ---------------------------------------------------------------------------------------------- g. more than one launch
@pytest.mark.parametrize("kernel", P.KERNELS)
def test_the_trials_of_the_long_launch_stay_finite(kernel):
    assert P.LAUNCH_N == P.LAUNCH_MAX + 2 == 258 and P.LAUNCH_CHECKED == (0, 255, 256, 257)
    assert (P.launch_re(0), P.launch_re(P.LAUNCH_N - 1)) == (100.0, 1000.0)
    for q in P.LAUNCH_CHECKED:
        r = P.launch_reference(kernel, q)
        assert r["rows"].shape == (P.LAUNCH_K, 8) and np.all(np.isfinite(r["rows"])) and r["cg_caps"] == 0
        assert max(float(np.max(np.abs(r["state"][k]))) for k in ("u", "v")) < 1.0
