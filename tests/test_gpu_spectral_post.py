"""The spectral post-processing kernels called through the C ABI, each against its extended-precision statement of
tests/spectral_post_numpy.py: ``ldc_gemm_nt`` (gemm_nt_kernel) and ``ldc_poisson_fastdiag`` elementwise within bounds that
are derived, not measured; ``ldc_vortex_extrema_xy`` (extrema_kernel) exactly, on the fields where its rules decide; then
psi and the vortex table of ``SGSolver`` off the square grid against the oracle, and a NaN state.

Every test prints its largest error / bound (run with -s): profiles/spectral_post.md keeps the table."""
import functools

import numpy as np
import pytest

import spectral_post_numpy as P
from oracle import ldc_oracle as orc

pytestmark = pytest.mark.gpu

SENTINEL = -12345.6789


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _call(name, *args):
    import torch
    from solvers.spectral import ldc_lib as L
    L.require_device()
    L.check(getattr(L.lib(), name)(*args, L.stream_ptr()), name)
    torch.cuda.synchronize()


def _padded(a, shape, fill=0.0):
    out = np.full(shape, fill)
    out[tuple(slice(0, n) for n in a.shape)] = a
    return out


@pytest.mark.parametrize("R16,K16,LD", P.GEMM_SHAPES, ids=lambda v: str(v))
def test_gemm_nt_against_long_double(R16, K16, LD):
    """Every element of the 16 R16 x 16 R16 result within gamma_n |A| |B|^T (plus the quotient's rounding), for the plain,
    the transposed, the scaled and the scaled-and-transposed product; inputs whose sums cancel (six decades of
    magnitudes); NaN in every element of A, B and lam that the product must not read; and a sentinel, kept bit for bit, in
    every element of C that it must not write."""
    rng = np.random.default_rng(1000 * R16 + K16)
    r, k = 16 * R16, 16 * K16
    A = _padded(P.wide_range(rng, (r, k)), (LD, LD), np.nan)
    B = _padded(P.wide_range(rng, (r, k)), (LD, LD), np.nan)
    lam_r = _padded(-rng.uniform(0.5, 500.0, r), (LD,), np.nan)
    lam_c = _padded(-rng.uniform(0.5, 500.0, r), (LD,), np.nan)
    dA, dB, dr, dc = _dev(A), _dev(B), _dev(lam_r), _dev(lam_c)
    outside = np.ones((LD, LD), dtype=bool)
    outside[:r, :r] = False
    for tr in (0, 1):
        for mode in (0, 1):
            want, bound = P.gemm_nt(A, B, R16, K16, tr, lam_r if mode else None, lam_c if mode else None)
            dC = _dev(np.full((LD, LD), SENTINEL))
            _call("ldc_gemm_nt", dA.data_ptr(), dB.data_ptr(), dC.data_ptr(), R16, K16, LD, tr, mode,
                  dr.data_ptr() if mode else None, dc.data_ptr() if mode else None)
            got = dC.cpu().numpy()
            assert P.same_bits(got[outside], np.full(int(outside.sum()), SENTINEL)), (tr, mode)
            ratio = np.abs(got[:r, :r] - want) / bound          # (NaN in got: the comparison below is False)
            print(f"gemm_nt R16={R16} K16={K16} LD={LD} transpose={tr} scale={mode}: max error / bound = {np.max(ratio):.4f}")
            assert np.all(ratio <= 1.0), (tr, mode, float(np.max(ratio)))


FASTDIAG_CASES = [(kind, s) for kind in ("chebyshev", "legendre") for s in P.FASTDIAG_SIZES] + [("synthetic", (17, 33))]


@pytest.mark.parametrize("kind,size", FASTDIAG_CASES, ids=lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]}")
def test_fastdiag_against_long_double(kind, size):
    """psi of ``ldc_poisson_fastdiag`` elementwise within the running bound of its four products on the live block, exactly
    0 on the padded rows and columns inside the 16 R blocks, nothing written beyond them.  Operators padded as
    ``SGSolver._eigenbasis`` pads them (zero-filled Q, lam padded with -1); F zero in the padding."""
    mx, my = size
    Qx, Qxi, Qy, Qyi, lamx, lamy, F = P.fastdiag_case(kind, mx, my)
    Mi = max(mx, my)
    r = 16 * ((Mi + 15) // 16)
    LD = r + 16
    want, bound = P.fastdiag(Qx, Qxi, Qy, Qyi, lamx, lamy, F)
    scale = float(np.max(np.abs(want)))
    assert float(np.max(bound)) <= 1e-11 * scale            # the comparison below cannot go slack
    sq = (LD, LD)
    dev = [_dev(_padded(a, sq)) for a in (Qx, Qxi, Qy, Qyi)] + [_dev(_padded(a, (LD,), -1.0)) for a in (lamx, lamy)]
    dF = _dev(_padded(F, sq))
    w0, w1, dPsi = (_dev(np.full(sq, SENTINEL)) for _ in range(3))
    _call("ldc_poisson_fastdiag", *[t.data_ptr() for t in dev], dF.data_ptr(), w0.data_ptr(), w1.data_ptr(),
          dPsi.data_ptr(), Mi, LD)
    got = dPsi.cpu().numpy()
    ratio = np.abs(got[:mx, :my] - want) / bound
    print(f"fastdiag {kind} {mx}x{my}: max error / bound = {np.max(ratio):.4f}, bound / max|psi| = {float(np.max(bound)) / scale:.2e}")
    assert np.all(ratio <= 1.0), float(np.max(ratio))
    assert np.all(got[mx:r, :r] == 0.0) and np.all(got[:r, my:r] == 0.0)
    for t in (w0, w1, dPsi):
        a = t.cpu().numpy()
        assert P.same_bits(a[r:, :], np.full((LD - r, LD), SENTINEL)) and P.same_bits(a[:r, r:], np.full((r, LD - r), SENTINEL))


@functools.lru_cache(maxsize=None)
def _extrema_cases(Mx, My):
    return {c[0]: c[1:] for c in P.extrema_cases(Mx, My)}


EXTREMA_FIELDS = ["random", "ties_one_thread_two_strides", "ties_last_thread_then_first", "constant", "nodes_at_one_half",
                  "region_without_positive_psi", "empty_regions", "omega_max_is_negative", "signed_zeros", "some_nan", "all_nan"]


@pytest.mark.parametrize("field", EXTREMA_FIELDS)
@pytest.mark.parametrize("Mx,My,LD", P.EXTREMA_SIZES, ids=lambda v: str(v))
def test_extrema_rules(Mx, My, LD, field):
    """Values (as bits) and indices equal ``extrema()``: first node in C order on ties, within a thread's strides and across
    threads; strict regions; the signed omega; NaN never chosen; -1 / NaN without a candidate.  The arrays beyond the
    Mx x My nodes hold values that would win every list if they were read."""
    Psi, W, x, y = _extrema_cases(Mx, My)[field]
    assert set(_extrema_cases(Mx, My)) == set(EXTREMA_FIELDS)
    want_val, want_idx = P.extrema(Psi, W, x, y, LD)
    pad = np.full((LD, LD), 1e300)           # rows beyond Mx: the largest psi and |omega|, inside BL (x = y = 0.25 there)
    pad[:Mx, My:] = -1e300                   # columns beyond My: the smallest psi
    dPsi, dW = pad.copy(), pad.copy()
    dPsi[:Mx, :My], dW[:Mx, :My] = Psi, W
    val, idx = _dev(np.full(8, SENTINEL)), _dev(np.full(8, 777, dtype=np.int32))
    tensors = [_dev(dPsi), _dev(dW), _dev(_padded(x, (LD,), 0.25)), _dev(_padded(y, (LD,), 0.25))]
    _call("ldc_vortex_extrema_xy", *[t.data_ptr() for t in tensors], Mx, My, LD, val.data_ptr(), idx.data_ptr())
    got_val, got_idx = val.cpu().numpy(), idx.cpu().numpy()
    assert list(got_idx[:5]) == list(want_idx), (got_idx, want_idx)
    assert P.same_bits(got_val[:5], want_val), (got_val, want_val)
    assert np.all(got_idx[5:] == 777) and P.same_bits(got_val[5:], np.full(3, SENTINEL))
    if field == "all_nan":
        assert list(got_idx[:5]) == [-1] * 5 and np.all(np.isnan(got_val[:5]))


def make(nx, ny, **kw):
    from solvers.spectral.sg import SGSolver
    args = dict(name="spectral", Re=100.0, lid_velocity=1.0, Lx=1.0, Ly=1.0, nx=nx, ny=ny, tolerance=1e-6,
                max_iterations=1000, basis_type="chebyshev", CFL=1.5, beta_squared=5.0, corner_treatment="smoothing",
                corner_smoothing=0.15, multigrid="none", check_every=64, graph_iters=8)
    args.update(kw)
    return SGSolver(**args)


TABLE_ITERATIONS = 30
PSI_RTOL, TABLE_TOL = 1e-10, 1e-9            # the tolerances of test_gpu_parity.py::test_trajectory_vs_reference


def developed_oracle(nx, ny):
    """An oracle whose vortex table is decided (``table_is_decided``): 30 iterations, not from rest -- there psi is 1e-3
    after 30 iterations and still 1e-2 after 800, the flow is all but symmetric about x = 0.5 and the runner-up gaps are
    1e-12 ... 1e-7 -- but from a seeded developed flow: a primary vortex of psi = -0.1 off the centre and a positive eddy in
    each of the three corners, u = psi_y and v = -psi_x by the oracle's own derivative matrices.  The iterations impose the
    lid and make it a state of the solver."""
    o = orc.OracleSG(nx, 100.0, ny=ny)
    X, Y = np.meshgrid(o.ax.x, o.ay.x, indexing="ij")

    def eddy(x0, x1, y0, y1):
        inside = (X > x0) & (X < x1) & (Y > y0) & (Y < y1)
        return np.where(inside, (np.sin(np.pi * (X - x0) / (x1 - x0)) * np.sin(np.pi * (Y - y0) / (y1 - y0))) ** 2, 0.0)
    psi = -0.1 * (np.sin(np.pi * X ** 1.3) * np.sin(np.pi * Y ** 1.6)) ** 2
    psi += 0.005 * (eddy(0.7, 1.0, 0.0, 0.3) + eddy(0.0, 0.25, 0.0, 0.25)) + 0.02 * eddy(0.0, 0.3, 0.6, 0.9)
    o.u, o.v = psi @ o.ay.D.T, -(o.ax.D @ psi)
    o.apply_bc(o.u, o.v)
    for _ in range(TABLE_ITERATIONS):
        o.step()
    return o


def table_is_decided(o, psi):
    """The oracle's table does not hang on a node choice that the tolerances leave open: each chosen extremum -- argmin psi,
    argmax |omega|, argmax psi of each corner region, which has to be positive -- beats its runner-up node by more than
    1e3 TABLE_TOL max(|value|, 1).  Returns the failures."""
    w = o.vorticity()
    X, Y = np.meshgrid(o.ax.x, o.ay.x, indexing="ij")
    everywhere = np.ones(psi.shape, dtype=bool)
    bad = []

    def clear(name, key, mask):
        gap, need = P.runner_up_gap(key, mask), 1e3 * TABLE_TOL * max(float(np.max(key[mask])), 1.0)
        if not (gap > need and np.max(key[mask]) > 0):
            bad.append((name, gap, need))
    clear("psi_min", -psi, everywhere)
    clear("omega_max", np.abs(w), everywhere)
    for name, mask in (("BR", (X > 0.5) & (Y < 0.5)), ("BL", (X < 0.5) & (Y < 0.5)), ("TL", (X < 0.5) & (Y > 0.5))):
        clear(name, psi, mask)
    return bad


@pytest.mark.parametrize("nx,ny", [(20, 28), (48, 129), (129, 48), (128, 128), (100, 100)], ids=lambda v: str(v))
def test_streamfunction_and_vortex_table_off_the_square(nx, ny):
    """The state of ``developed_oracle``, uploaded, so that only post-processing is compared: psi within 1e-10 max|psi| of the oracle's Sylvester
    solve and every key of the vortex table within 1e-9 max(|ref|, 1) -- with x longer than y, y longer than x, at the
    headline size 128 (library's own kernel choice) and at a size that is no multiple of 16."""
    o = developed_oracle(nx, ny)
    want_psi = o.streamfunction()
    assert table_is_decided(o, want_psi) == []
    want = o.vortex_metrics(want_psi)
    s = make(nx, ny)
    s.set_state(u=o.u, v=o.v, p=o.p)
    psi, _, _ = s._compute_streamfunction()
    vm = s.compute_vortex_metrics()
    s.close()
    scale = float(np.max(np.abs(want_psi)))
    err = float(np.max(np.abs(psi - want_psi)))
    print(f"psi {nx}x{ny}: max error / max|psi| = {err / scale:.2e}")
    assert psi.shape == want_psi.shape and err <= PSI_RTOL * scale
    assert set(vm) == set(want)
    for k, v in want.items():
        print(f"  {k}: {vm[k]!r} vs {v!r}")
        assert abs(vm[k] - v) <= TABLE_TOL * max(abs(v), 1.0), k


def test_a_nan_state_gives_empty_vortex_metrics():
    """No node of a NaN state's omega is a candidate (psi keeps the 0 of its wall nodes): the kernel returns -1 for omega_max
    and loads nothing, ``compute_vortex_metrics`` raises, and ``_store_results`` stores empty vortex metrics as the
    reference's try/except does."""
    from solvers.base import _VORTEX_KEYS
    s = make(16, 16)
    nan = np.full((17, 17), np.nan)
    s.set_state(u=nan, v=nan, p=np.full((15, 15), np.nan))
    with pytest.raises(ValueError, match="no finite node"):
        s.compute_vortex_metrics()
    assert int(s.d["ext_idx"][1]) == -1 and bool(s.d["ext_val"][1].isnan())
    s._store_results(np.zeros((0, 8)), 0, False, 0.0)
    assert len(_VORTEX_KEYS) == 19 and all(getattr(s.metrics, k) == 0.0 for k in _VORTEX_KEYS)
    s.close()
