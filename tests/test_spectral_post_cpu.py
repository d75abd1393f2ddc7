"""The extended-precision statements of tests/spectral_post_numpy.py against the oracle, the extrema rule against its NumPy
spelling on the fields where the rule decides, and the argument refusals of ``ldc_gemm_nt``, ``ldc_poisson_fastdiag`` and
``ldc_vortex_extrema_xy``.  No device is needed: tests/test_gpu_spectral_post.py holds the kernels to these statements."""
import ctypes as C

import numpy as np
import pytest

import spectral_post_numpy as P
from oracle import ldc_oracle as orc


@pytest.fixture(scope="module", params=[(16, 16), (20, 28), (64, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def oracle(request):
    """A state 20 iterations from rest."""
    nx, ny = request.param
    o = orc.OracleSG(nx, 100.0, ny=ny)
    for _ in range(20):
        o.step()
    return o


def test_fastdiag_statement_equals_the_sylvester_solve(oracle):
    """The long-double fast diagonalisation with the solver's own eigenbases is the oracle's psi (SciPy's Sylvester solve)
    within 1e-12 max|psi| (measured: 5e-15 ... 5e-14), and its fp64 bound stays below the 1e-11 max|psi| that the GPU
    test requires of its cases."""
    from solvers.spectral.sg import _interior_eigenbasis
    o = oracle
    lamx, Qx, Qxi = _interior_eigenbasis(o.ax.D2)
    lamy, Qy, Qyi = _interior_eigenbasis(o.ay.D2)
    want = o.streamfunction()[1:-1, 1:-1]
    got, bound = P.fastdiag(Qx, Qxi, Qy, Qyi, lamx, lamy, -o.vorticity()[1:-1, 1:-1])
    scale = float(np.max(np.abs(want)))
    err = float(np.max(np.abs(got - want)))
    print(f"fastdiag vs sylvester {o.M}x{o.My}: err/max|psi| = {err / scale:.2e}, bound/max|psi| = {float(np.max(bound)) / scale:.2e}")
    assert err <= 1e-12 * scale
    assert float(np.max(bound)) <= 1e-11 * scale


def test_extrema_statement_equals_the_oracle_table(oracle):
    """Key for key and exactly: both pick nodes of the same arrays."""
    o = oracle
    psi = o.streamfunction()
    want = o.vortex_metrics(psi)
    got = P.vortex_table(psi, o.vorticity(), o.ax.x, o.ay.x)
    assert set(got) == set(want)
    for k, v in want.items():
        assert got[k] == v, k


def _numpy_spelling(Psi, W, x, y):
    """The five flat node indices as NumPy spells them (oracle/ldc_oracle.py, vortex_metrics)."""
    X, Y = np.meshgrid(x, y, indexing="ij")
    regions = ((X > 0.5) & (Y < 0.5), (X < 0.5) & (Y < 0.5), (X < 0.5) & (Y > 0.5))
    return [int(np.argmin(Psi)), int(np.argmax(np.abs(W)))] + [int(np.argmax(np.where(m, Psi, -np.inf))) for m in regions], regions


@pytest.mark.parametrize("size", P.EXTREMA_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_extrema_statement_on_the_deciding_fields(size):
    """Where NumPy's argmin / argmax and the rule agree by construction (no NaN in the field, the region not empty) they
    agree; NaN nodes are never chosen; a list without a candidate gives -1 / NaN; the value is the field's own bits."""
    Mx, My, _ = size
    for name, Psi, W, x, y in P.extrema_cases(Mx, My):
        val, idx = P.extrema(Psi, W, x, y)
        spelled, regions = _numpy_spelling(Psi, W, x, y)
        masks = [np.ones((Mx, My), bool)] * 2 + list(regions)
        for k in range(5):
            field = W if k == 1 else Psi
            live = masks[k] & ~np.isnan(field)
            if not live.any():
                assert idx[k] == -1 and np.isnan(val[k]), (name, k)
                continue
            assert P.same_bits(val[k], field.ravel()[idx[k]]) and live.ravel()[idx[k]], (name, k)
            if not np.isnan(field).any():
                assert idx[k] == spelled[k], (name, k)
            key = np.abs(field) if k == 1 else (-field if k == 0 else field)
            best = np.max(key[live])
            assert key.ravel()[idx[k]] == best and not np.any(live.ravel()[: idx[k]] & (key.ravel()[: idx[k]] == best)), (name, k)
        if name == "all_nan":
            assert np.all(idx == -1) and np.all(np.isnan(val))
            with pytest.raises(ValueError, match="no finite node"):
                P.vortex_table(Psi, W, x, y)
        if name == "empty_regions":
            assert idx[3] == -1 and idx[4] == -1 and (idx[2] >= 0 or Mx * My < 4)
        if name == "nodes_at_one_half":
            assert all(val[k] < 10.0 or np.isnan(val[k]) for k in (2, 3, 4))
        if name == "omega_max_is_negative":
            assert val[1] == -5.0
        if name == "ties_last_thread_then_first" and Mx * My > 1024:
            assert idx[0] == 1023 and idx[1] == 1023 and val[1] == -9.0
        if name == "ties_one_thread_two_strides" and Mx * My > 5 + 1024:
            assert idx[0] == 5 and idx[1] == 5 and val[1] == -9.0


def test_gemm_statement_and_its_bound():
    """The long-double product is NumPy's fp64 product within the derived bound, which is sharp: fp64 uses a few per cent
    of it, and one dropped k-group exceeds it by orders of magnitude."""
    rng = np.random.default_rng(7)
    R16, K16, LD = 2, 5, 96
    A, B = P.wide_range(rng, (LD, LD)), P.wide_range(rng, (LD, LD))
    lam = -rng.uniform(0.5, 50.0, LD)
    for tr in (0, 1):
        for lam_r in (None, lam):
            want, bound = P.gemm_nt(A, B, R16, K16, tr, lam_r, lam_r)
            got = A[:32, :80] @ B[:32, :80].T
            short = A[:32, :64] @ B[:32, :64].T
            if lam_r is not None:
                den = lam[:32, None] + lam[None, :32]
                got, short = got / den, short / den
            if tr:
                got, short = got.T, short.T
            assert want.shape == bound.shape == (32, 32)
            assert np.all(np.abs(got - want) <= bound)
            assert np.median(np.abs(short - want) / bound) > 1e6


def _ptr(nonzero=True):
    return C.c_void_p(4096 if nonzero else None)


def test_the_three_entry_points_refuse_bad_arguments_without_a_device():
    """Every refusal is LDC_E_ARG (-1), decided before anything is launched: the pointers are never dereferenced."""
    import __graft_entry__ as g
    g.build()
    from solvers.spectral import ldc_lib
    L = ldc_lib.lib()
    p = _ptr()
    gemm = lambda R16, K16, LD, mode, lr, lc: L.ldc_gemm_nt(p, p, p, R16, K16, LD, 0, mode, lr, lc, None)       # noqa: E731
    assert gemm(1, 1, 24, 0, None, None) == -1              # LD no multiple of 16
    assert gemm(3, 1, 32, 0, None, None) == -1              # LD < 16 R16
    assert gemm(1, 3, 32, 0, None, None) == -1              # LD < 16 K16
    assert gemm(1, 1, 16, 2, p, p) == -1                    # no such scale mode
    assert gemm(1, 1, 16, 1, None, p) == -1 and gemm(1, 1, 16, 1, p, None) == -1      # scaling without eigenvalues
    assert gemm(0, 1, 16, 0, None, None) == -1 and gemm(1, 0, 16, 0, None, None) == -1
    assert L.ldc_poisson_fastdiag(p, p, p, p, p, p, p, p, p, p, 0, 16, None) == -1          # Mi < 1
    assert L.ldc_poisson_fastdiag(p, p, p, p, p, p, p, p, p, p, 17, 16, None) == -1         # LD < 16 ceil(Mi / 16)
    ext = lambda Mx, My, LD: L.ldc_vortex_extrema_xy(p, p, p, p, Mx, My, LD, p, p, None)    # noqa: E731
    assert ext(1, 4, 16) == -1 and ext(4, 1, 16) == -1      # fewer than 2 nodes on an axis
    assert ext(4, 20, 16) == -1 and ext(20, 4, 16) == -1    # LD < My, LD < Mx
    assert L.ldc_vortex_extrema_xy(None, p, p, p, 4, 4, 16, p, p, None) == -1
