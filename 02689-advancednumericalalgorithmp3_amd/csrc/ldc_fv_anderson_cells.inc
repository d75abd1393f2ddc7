// ldc_fv_anderson_cells.inc -- the arithmetic of the Anderson mixing of the finite-volume SIMPLE iteration
// (include/ldc_fv.h), written once for every mapping of a trial onto the card.  Included by ldc_fv_anderson.hip (one
// trial per work-group of 512 threads) and by ldc_fv_wide.hip ahead of ldc_fv_wide_anderson.inc (a chip or shared
// trial, three launches); everything is a device function in the anonymous namespace, so each unit compiles its own
// copy and neither code object depends on the other.  tests/fv_anderson_numpy.py restates the algorithm.
//
// The fixed-point map is x -> g = SIMPLE(x) on [u | v | p | mdot], L = 3n + faces entries;
// hist = [ x | g_prev | f_prev | dG[depth] | dF[depth] ], L doubles each.
//
// What is here: the constants, the view of hist (FvAaHist), entry e of the state (fv_state_at), push for one entry
// (fv_anderson_push_entry), one entry into a row block of A = dF^T dF and b = dF^T f with the sums of a wave
// (fv_anderson_acc_*), (A + lambda I) gamma = b by Cholesky (fv_anderson_solve) and mix for one entry
// (fv_anderson_mix_entry).
// What a mapping supplies: the loops over the entries, when an iteration pushes and mixes (astate, the gate), the sums
// over the waves of a work-group and beyond it, which triangle of A goes where, and the barriers or launch boundaries.
#ifndef LDC_FV_ANDERSON_CELLS_INC
#define LDC_FV_ANDERSON_CELLS_INC

#include <math.h>

#include "ldc_fv_common.inc"

namespace {

constexpr int kFvAaDepth = LDC_FV_ANDERSON_MAX_DEPTH;
constexpr int kFvAaRows = 4;                             // rows of A per pass over the columns
constexpr int kFvAaSums = kFvAaRows * (kFvAaDepth + 1);  // per pass: 4 x (16 entries of A, 1 of b)
constexpr double kFvAaLambda = 1e-12;
static_assert(kFvAaDepth % kFvAaRows == 0, "row blocks");

// the trial's vectors of L = 3n + faces doubles inside hist
struct FvAaHist {
  long long L;
  double *x, *gp, *fp, *dG, *dF;
  __device__ __forceinline__ FvAaHist(double* h, long long L_, int depth)
      : L(L_), x(h), gp(h + L_), fp(h + 2 * L_), dG(h + 3 * L_), dF(h + (3 + depth) * L_) {}
};

// entry e of [u | v | p | mdot]
__device__ __forceinline__ double* fv_state_at(const FvDesc& d, int n, int e) {
  return e < n ? d.u + e : (e < 2 * n ? d.v + (e - n) : (e < 3 * n ? d.p + (e - 2 * n) : d.mdot + (e - 3 * n)));
}

// push, entry e: f = g - x; the new columns dG = g - g_prev, dF = f - f_prev into the ring slot (dGs, dFs); g_prev = g,
// f_prev = f; keep_g (the iteration is not mixed): x = g at once
__device__ __forceinline__ void fv_anderson_push_entry(const FvDesc& d, const FvAaHist& H, int n, int e, bool has_f,
                                                       bool push, double* dGs, double* dFs, bool keep_g) {
  const double g = *fv_state_at(d, n, e);
  if (has_f) {
    const double f = g - H.x[e];
    if (push) {
      dGs[e] = g - H.gp[e];
      dFs[e] = f - H.fp[e];
    }
    H.gp[e] = g;
    H.fp[e] = f;
  }
  if (keep_g) H.x[e] = g;
}

// rows i0 .. i0 + 3 of A[i][k] = dF_i . dF_k (columns 0 .. 15) and of b[i] = dF_i . f (column 16) over m valid columns:
// the sums of a thread
__device__ __forceinline__ void fv_anderson_acc_clear(double (&acc)[kFvAaRows][kFvAaDepth + 1]) {
#pragma unroll
  for (int r = 0; r < kFvAaRows; ++r)
#pragma unroll
    for (int k = 0; k <= kFvAaDepth; ++k) acc[r][k] = 0.0;
}

__device__ __forceinline__ void fv_anderson_acc_entry(const FvAaHist& H, int m, int i0, int e,
                                                      double (&acc)[kFvAaRows][kFvAaDepth + 1]) {
  double c[kFvAaDepth + 1];
#pragma unroll
  for (int k = 0; k < kFvAaDepth; ++k) c[k] = k < m ? H.dF[k * H.L + e] : 0.0;
  c[kFvAaDepth] = H.fp[e];
#pragma unroll
  for (int r = 0; r < kFvAaRows; ++r) {
    const double rv = i0 + r < m ? H.dF[(i0 + r) * H.L + e] : 0.0;
#pragma unroll
    for (int k = 0; k <= kFvAaDepth; ++k) acc[r][k] = fma(rv, c[k], acc[r][k]);
  }
}

// the sums of the calling wave by xor shuffles, into part[wave][kFvAaSums]
__device__ __forceinline__ void fv_anderson_acc_wave(const double (&acc)[kFvAaRows][kFvAaDepth + 1],
                                                     double (*part)[kFvAaSums]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int r = 0; r < kFvAaRows; ++r) {
#pragma unroll
    for (int k = 0; k <= kFvAaDepth; ++k) {
      double s = acc[r][k];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
      if (lane == 0) part[w][r * (kFvAaDepth + 1) + k] = s;
    }
  }
}

// (A + lambda I) gamma = b by Cholesky on the lower triangle of A, one thread; false: a pivot that is not > 0 or a gamma
// that is not finite
__device__ __forceinline__ bool fv_anderson_solve(int m, double (*A)[kFvAaDepth + 1], const double* b, double* gamma) {
  double tr = 0.0;
  for (int i = 0; i < m; ++i) tr += A[i][i];
  const double lam = kFvAaLambda * tr / m;
  for (int i = 0; i < m; ++i) A[i][i] += lam;
  for (int i = 0; i < m; ++i) {                            // the lower triangle becomes R^T
    for (int k = 0; k <= i; ++k) {
      double s = A[i][k];
      for (int q = 0; q < k; ++q) s -= A[i][q] * A[k][q];
      if (k == i) {
        if (!(s > 0.0)) return false;
        A[i][i] = sqrt(s);
      } else {
        A[i][k] = s / A[k][k];
      }
    }
  }
  for (int i = 0; i < m; ++i) {
    double s = b[i];
    for (int q = 0; q < i; ++q) s -= A[i][q] * gamma[q];
    gamma[i] = s / A[i][i];
  }
  for (int i = m - 1; i >= 0; --i) {
    double s = gamma[i];
    for (int q = i + 1; q < m; ++q) s -= A[q][i] * gamma[q];
    gamma[i] = s / A[i][i];
  }
  for (int i = 0; i < m; ++i)
    if (!(fabs(gamma[i]) <= 1.7976931348623157e308)) return false;
  return true;
}

// mix, entry e: x_next = g - sum_i gamma_i dG_i (slot order) into the state and x; the pinned cell's p is written as
// 0.0.  The fallback leaves the state (it is g) and keeps g as x.
__device__ __forceinline__ void fv_anderson_mix_entry(const FvDesc& d, const FvAaHist& H, int n, int e, int m, bool fell,
                                                      const double* gamma) {
  double xn = H.gp[e];
  if (!fell) {
    for (int k = 0; k < m; ++k) xn -= gamma[k] * H.dG[k * H.L + e];
    if (e == 2 * n) xn = 0.0;
    *fv_state_at(d, n, e) = xn;
  }
  H.x[e] = xn;
}

}  // namespace

#endif  // LDC_FV_ANDERSON_CELLS_INC
