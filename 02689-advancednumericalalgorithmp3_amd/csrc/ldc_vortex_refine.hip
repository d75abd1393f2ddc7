// ldc_vortex_refine.hip -- sub-grid vortex centres of the spectral solver (include/ldc_hip.h, ldc_vortex_refine): Newton's
// method on the gradient of the tensor-product Lagrange interpolant of psi, started at the grid extrema that
// ldc_vortex_extrema_xy left in device memory.  A translation unit of its own, linked into libldc_hip.so beside
// ldc_kernels.hip: the code object of the solve kernels is the same with and without this file.
//
// Mapping: ONE work-group of 256 threads per (job, extremum), grid (4, jobs of the launch); extremum 0 the primary minimum,
// 1, 2, 3 the BR, BL, TL maxima.  Work-groups share nothing: no flags, no atomics, nobody waits for anybody.  Every thread
// of a work-group carries the same z, the same sums and the same decisions (block_sum hands every thread the same totals).
//
// One evaluation at z (refine_eval), twelve vectors of at most LDC_REFINE_MAX_M doubles in LDS:
//   1. a = l_x(z_x), b = l_y(z_y)    barycentric formula with the caller's weights; the unit vector when z sits on a node
//   2. a1 = a Dx, a2 = a1 Dx, b1 = b Dy, b2 = b1 Dy    thread j takes column j (coalesced); the derivative of the
//                                    interpolant is the interpolant of D psi, so first-derivative matrices are all it takes
//   3. w0 = Psi b, w1 = Psi b1, w2 = Psi b2    one wave per row, all three in one pass (the closing evaluation: w2 = W b)
//   4. g = (a1.w0, a.w1), H = [[a2.w0, a1.w1], [a1.w1, a.w2]]    (closing: psi = a.w0, omega = a.w2, g)
// Definiteness is judged against rounding: beside every entry of H the same pass sums the magnitudes of its terms
// (q_k = |Psi| |b_k| in step 3, |a2|.q0, |a1|.q1, |a|.q2 in step 4); an entry counts only above its floor
// F = 3 M 2^-53 times that sum (M = max(Mx, My): three chained sums of at most M terms), and det only above
// Fxx |Hyy| + Fyy |Hxx| + 2 Fxy |Hxy|.  The Hessian of a field without curvature (psi = x + y) is the rounding of its own
// sums, two orders below the floor, with signs that follow the summation order: it is indefinite by this rule in any order;
// the Hessians of real vortices stand seven orders above it.
// Every reduction runs in a fixed order -- per thread in increasing index, xor shuffles inside a wave, the four waves in
// order from LDS, as fv_post_kernel reduces --: a job's result is bit-identical whatever else is in the launch.
// tests/vortex_refine_numpy.py states the same algorithm in NumPy with derived rounding bounds.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ldc_hip.h"

namespace {

constexpr int kRefThreads = 256, kRefWaves = 4, kRefRed = 8;
constexpr int kRefLaunchMax = 36;          // jobs of one launch

struct RefineLaunch {
  ldc_refine_job jobs[kRefLaunchMax];
};
static_assert(sizeof(RefineLaunch) <= 3600, "kernel arguments");
static_assert(LDC_REFINE_OUT_LEN == 4 * 8, "eight doubles per extremum");
static_assert(LDC_REFINE_MAX_M <= 2 * kRefThreads, "a thread takes at most two entries of a vector");

struct RefineLds {
  double a[3][LDC_REFINE_MAX_M], b[3][LDC_REFINE_MAX_M], w[3][LDC_REFINE_MAX_M], q[3][LDC_REFINE_MAX_M];
  double red[kRefWaves * kRefRed];
};

// sums of K values over the work-group, every thread gets the same totals; fixed order
template <int K>
__device__ inline void block_sum(double (&v)[K], double* red) {
  static_assert(K <= kRefRed, "reduction slot");
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_xor(v[k], off);
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) red[w * kRefRed + k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double s = 0.0;
#pragma unroll 1
    for (int q = 0; q < kRefWaves; ++q) s += red[q * kRefRed + k];
    v[k] = s;
  }
  __syncthreads();          // (the next sum writes red again)
}

// the Lagrange basis values of both axes at (zx, zy) into a[0..Mx), b[0..My)
__device__ inline void refine_basis(const ldc_refine_job& J, double zx, double zy, RefineLds& s) {
  const int t = threadIdx.x;
  double v[4] = {0.0, 0.0, 0.0, 0.0};      // sum of w_i / (z - x_i), 1 + the node z sits on; the same for y
  for (int i = t; i < J.Mx; i += kRefThreads) {
    const double d = zx - J.x[i];
    if (d == 0.0) { v[1] += (double)(i + 1); s.a[0][i] = 0.0; }
    else { const double q = J.wx[i] / d; v[0] += q; s.a[0][i] = q; }
  }
  for (int j = t; j < J.My; j += kRefThreads) {
    const double d = zy - J.y[j];
    if (d == 0.0) { v[3] += (double)(j + 1); s.b[0][j] = 0.0; }
    else { const double q = J.wy[j] / d; v[2] += q; s.b[0][j] = q; }
  }
  block_sum(v, s.red);
  const int hx = (int)v[1] - 1, hy = (int)v[3] - 1;
  for (int i = t; i < J.Mx; i += kRefThreads) s.a[0][i] = hx >= 0 ? (i == hx ? 1.0 : 0.0) : s.a[0][i] / v[0];
  for (int j = t; j < J.My; j += kRefThreads) s.b[0][j] = hy >= 0 ? (j == hy ? 1.0 : 0.0) : s.b[0][j] / v[2];
  __syncthreads();
}

// dst = src D (a row vector times the matrix): thread j takes column j
__device__ inline void refine_vecmat(const double* src, const double* D, int M, int LDD, double* dst) {
  for (int j = threadIdx.x; j < M; j += kRefThreads) {
    double acc = 0.0;
    for (int i = 0; i < M; ++i) acc += src[i] * D[(size_t)i * LDD + j];
    dst[j] = acc;
  }
}

// FINAL = false: out = gx, gy, Hxx, Hxy, Hyy at z and the sums of the magnitudes of the terms of Hxx, Hxy, Hyy.
// FINAL = true: out = gx, gy, psi, omega at z (the rest 0).
template <bool FINAL>
__device__ inline void refine_eval(const ldc_refine_job& J, double zx, double zy, RefineLds& s, double (&out)[8]) {
  const int Mx = J.Mx, My = J.My;
  refine_basis(J, zx, zy, s);
  refine_vecmat(s.a[0], J.Dx, Mx, J.LDD, s.a[1]);
  refine_vecmat(s.b[0], J.Dy, My, J.LDD, s.b[1]);
  __syncthreads();
  if (!FINAL) {
    refine_vecmat(s.a[1], J.Dx, Mx, J.LDD, s.a[2]);
    refine_vecmat(s.b[1], J.Dy, My, J.LDD, s.b[2]);
    __syncthreads();
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = wave; i < Mx; i += kRefWaves) {
    const double* row = J.Psi + (size_t)i * J.LD;
    const double* row2 = FINAL ? J.W + (size_t)i * J.LD : row;
    const double* b2 = FINAL ? s.b[0] : s.b[2];
    double r0 = 0.0, r1 = 0.0, r2 = 0.0, q0 = 0.0, q1 = 0.0, q2 = 0.0;
    for (int j = lane; j < My; j += 64) {
      const double p = row[j];
      const double t0 = p * s.b[0][j], t1 = p * s.b[1][j], t2 = row2[j] * b2[j];
      r0 += t0; r1 += t1; r2 += t2;
      if (!FINAL) { q0 += fabs(t0); q1 += fabs(t1); q2 += fabs(t2); }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      r0 += __shfl_xor(r0, off);
      r1 += __shfl_xor(r1, off);
      r2 += __shfl_xor(r2, off);
      if (!FINAL) { q0 += __shfl_xor(q0, off); q1 += __shfl_xor(q1, off); q2 += __shfl_xor(q2, off); }
    }
    if (lane == 0) {
      s.w[0][i] = r0; s.w[1][i] = r1; s.w[2][i] = r2;
      if (!FINAL) { s.q[0][i] = q0; s.q[1][i] = q1; s.q[2][i] = q2; }
    }
  }
  __syncthreads();
  double v[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < Mx; i += kRefThreads) {
    v[0] += s.a[1][i] * s.w[0][i];
    v[1] += s.a[0][i] * s.w[1][i];
    if (FINAL) {
      v[2] += s.a[0][i] * s.w[0][i];
      v[3] += s.a[0][i] * s.w[2][i];
    } else {
      v[2] += s.a[2][i] * s.w[0][i];
      v[3] += s.a[1][i] * s.w[1][i];
      v[4] += s.a[0][i] * s.w[2][i];
      v[5] += fabs(s.a[2][i]) * s.q[0][i];
      v[6] += fabs(s.a[1][i]) * s.q[1][i];
      v[7] += fabs(s.a[0][i]) * s.q[2][i];
    }
  }
  block_sum(v, s.red);
#pragma unroll
  for (int k = 0; k < 8; ++k) out[k] = v[k];
}

__device__ inline bool refine_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }      // (false for NaN)

__global__ __launch_bounds__(kRefThreads) void vortex_refine_kernel(const RefineLaunch L) {
  __shared__ RefineLds s;
  const ldc_refine_job& J = L.jobs[blockIdx.y];
  const int e = blockIdx.x;                // 0 primary minimum; 1, 2, 3 the BR, BL, TL maxima
  const bool is_min = e == 0;
  const int Mx = J.Mx, My = J.My;
  double* out = J.out + 8 * e;
  const int q = J.idx[e == 0 ? 0 : e + 1];
  const int i0 = q < 0 ? -1 : q / J.LD, j0 = q < 0 ? -1 : q % J.LD;
  const bool on_grid = i0 >= 0 && i0 < Mx && j0 < My;
  const double pn = on_grid ? J.Psi[(size_t)i0 * J.LD + j0] : 0.0;
  if (!on_grid || (!is_min && !(pn > 0.0))) {          // no grid candidate: zeros, as the host writes without a refinement
    if (threadIdx.x < 8) out[threadIdx.x] = threadIdx.x == 0 ? 1.0 : 0.0;
    return;
  }
  const double wn = J.W[(size_t)i0 * J.LD + j0], xn = J.x[i0], yn = J.y[j0];
  const int im = i0 > 0 ? i0 - 1 : 0, ip = i0 < Mx - 1 ? i0 + 1 : Mx - 1;
  const int jm = j0 > 0 ? j0 - 1 : 0, jp = j0 < My - 1 ? j0 + 1 : My - 1;
  const double xlo = fmin(J.x[im], J.x[ip]), xhi = fmax(J.x[im], J.x[ip]);
  const double ylo = fmin(J.y[jm], J.y[jp]), yhi = fmax(J.y[jm], J.y[jp]);
  const double tolx = 1e-13 * fabs(J.x[Mx - 1] - J.x[0]), toly = 1e-13 * fabs(J.y[My - 1] - J.y[0]);

  const double floor_rel = 3.0 * (double)(Mx > My ? Mx : My) * 0x1p-53;
  double zx = xn, zy = yn, r[8];
  int status = 4, steps = 0;
  for (int it = 0; it < LDC_REFINE_MAX_STEPS; ++it) {
    refine_eval<false>(J, zx, zy, s, r);
    const double gx = r[0], gy = r[1], hxx = r[2], hxy = r[3], hyy = r[4];
    if (!(refine_finite(gx) && refine_finite(gy) && refine_finite(hxx) && refine_finite(hxy) && refine_finite(hyy))) {
      status = 6;
      break;
    }
    const double fxx = floor_rel * r[5], fxy = floor_rel * r[6], fyy = floor_rel * r[7];
    const double det = hxx * hyy - hxy * hxy, fdet = fxx * fabs(hyy) + fyy * fabs(hxx) + 2.0 * fxy * fabs(hxy);
    const double sxx = is_min ? hxx : -hxx, syy = is_min ? hyy : -hyy;
    if (!(sxx > fxx && syy > fyy && det > fdet)) { status = 2; break; }
    const double tx = zx - (hyy * gx - hxy * gy) / det, ty = zy - (hxx * gy - hxy * gx) / det;
    const double nx = fmin(fmax(tx, xlo), xhi), ny = fmin(fmax(ty, ylo), yhi);
    const bool clipped = nx != tx || ny != ty;
    const double sx = nx - zx, sy = ny - zy;
    zx = nx; zy = ny; steps = it + 1;
    if (fabs(sx) <= tolx && fabs(sy) <= toly) { status = clipped ? 3 : 0; break; }
  }
  refine_eval<true>(J, zx, zy, s, r);
  const double gnorm = sqrt(r[0] * r[0] + r[1] * r[1]), psi = r[2], om = r[3];
  if (status == 0) {
    if (!(refine_finite(zx) && refine_finite(zy) && refine_finite(psi) && refine_finite(om) && refine_finite(gnorm))) status = 6;
    else if (is_min ? !(psi <= pn) : !(psi >= pn)) status = 5;
    else if (e == 1 && !(zx > 0.5 && zy < 0.5)) status = 5;
    else if (e == 2 && !(zx < 0.5 && zy < 0.5)) status = 5;
    else if (e == 3 && !(zx < 0.5 && zy > 0.5)) status = 5;
  }
  if (threadIdx.x == 0) {
    const bool ok = status == 0;
    out[0] = (double)status;
    out[1] = ok ? zx : xn;
    out[2] = ok ? zy : yn;
    out[3] = ok ? psi : pn;
    out[4] = ok ? om : wn;
    out[5] = (double)steps;
    out[6] = gnorm;
    out[7] = 0.0;
  }
}

}  // namespace

extern "C" {

int ldc_vortex_refine(const struct ldc_refine_job* jobs, int n, void* stream) {
  if (!jobs || n < 1) return LDC_E_ARG;
  for (int q = 0; q < n; ++q) {
    const ldc_refine_job& j = jobs[q];
    if (!j.Psi || !j.W || !j.x || !j.y || !j.wx || !j.wy || !j.Dx || !j.Dy || !j.idx || !j.out) return LDC_E_ARG;
    if (j.Mx < 3 || j.My < 3 || j.Mx > LDC_REFINE_MAX_M || j.My > LDC_REFINE_MAX_M) return LDC_E_ARG;
    if (j.LD < j.My || j.LDD < (j.Mx > j.My ? j.Mx : j.My)) return LDC_E_ARG;
  }
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) return LDC_E_NODEVICE;
  for (int lo = 0; lo < n; lo += kRefLaunchMax) {
    RefineLaunch L;
    const int b = n - lo < kRefLaunchMax ? n - lo : kRefLaunchMax;
    for (int q = 0; q < kRefLaunchMax; ++q) L.jobs[q] = jobs[lo + (q < b ? q : 0)];
    hipLaunchKernelGGL(vortex_refine_kernel, dim3(4, b), dim3(kRefThreads), 0, reinterpret_cast<hipStream_t>(stream), L);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  return 0;
}

}  // extern "C"
