// ldc_fv_post_cells.inc -- the arithmetic of the finite-volume post-processing (streamfunction and vortex metrics,
// include/ldc_fv.h), written once for every mapping of a trial onto the card.  Included by ldc_fv_post.hip (one trial per
// work-group of 512 threads) and by ldc_fv_wide.hip (a chip or shared trial, one launch per phase); everything is a
// device function in the anonymous namespace, so each unit compiles its own copy and neither code object depends on the
// other.
//
// Reference: base.py:569-760 (streamfunction and vortex extrema), as solvers/fv/solver.py restates them on the host.
//
// What is here: one cell of omega (fv_post_cell_vorticity), one 16 x 16 tile of a GEMM of the sine fast diagonalisation
// (fv_post_gemm_tile), the five extremum candidates -- FvBest, one cell of their scan (fv_post_cell_extrema) and their
// merge over a work-group (fv_post_best_merge) -- and the result block from the winners (fv_post_result).
// What a mapping supplies: the cell loop and the tile loop (which cells and tiles a thread or wave takes), the barriers
// or launch boundaries between the phases, the LDS of the merge, and, where a phase is more than one work-group, the
// slots its candidates and not-finite flags go through.
#ifndef LDC_FV_POST_CELLS_INC
#define LDC_FV_POST_CELLS_INC

#include <limits.h>

#include "ldc_fv_common.inc"

namespace {

// omega at cell c with ghost cells (-f at the walls, 2 lid - u at the lid), psi = 0 on the boundary ring; true if the
// value is not finite
__device__ __forceinline__ bool fv_post_cell_vorticity(int c, int nx, int ny, double dx, double dy, double lid,
                                                       const double* u, const double* v, double* omega, double* psi) {
  const int i = c % nx, j = c / nx;
  const double vE = i < nx - 1 ? v[c + 1] : -v[c], vW = i > 0 ? v[c - 1] : -v[c];
  const double uN = j < ny - 1 ? u[c + nx] : 2 * lid - u[c], uS = j > 0 ? u[c - nx] : -u[c];
  const double wc = (vE - vW) / (2 * dx) - (uN - uS) / (2 * dy);
  omega[c] = wc;
  if (i == 0 || i == nx - 1 || j == 0 || j == ny - 1) psi[c] = 0.0;
  return !(fabs(wc) <= 1.7976931348623157e308);
}

// Tile t (16 x 16, row-major over the tiles) of C[r*ldc + c] = sum_k A(r, k) B(k, c) (M x N), A(r, k) = A[r*sar + k*sak],
// B(k, c) = B[k*sbk + c*sbc], by the calling wave: fv_gemm_tile of the solve kernel (operands from L2, zero fill at the
// edges, ONE accumulator over k in steps of 4) with a leading dimension for C and the Dirichlet epilogue.
// SCALE: C[a][b] /= cx*lamx[b] + cy*lamy[a]; every mode is kept.
template <bool SCALE>
__device__ __forceinline__ void fv_post_gemm_tile(int t, const double* A, int sar, int sak, const double* B, int sbk,
                                                  int sbc, double* Cm, int ldc, int M, int N, int K, const double* lamx,
                                                  const double* lamy, double cx, double cy) {
  const int lane = threadIdx.x & 63;
  const int tn = (N + 15) >> 4;
  const int r0 = (t / tn) * 16, c0 = (t % tn) * 16;
  const int ar = r0 + (lane & 15), bc = c0 + (lane & 15), kq = lane >> 4;
  v4d acc = {0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < K; k0 += 4) {
    const int k = k0 + kq;
    const double a = (ar < M && k < K) ? A[ar * sar + k * sak] : 0.0;
    const double b = (bc < N && k < K) ? B[k * sbk + bc * sbc] : 0.0;
    acc = MFMA_F64(a, b, acc);
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int row = r0 + (lane >> 4) + 4 * q, col = c0 + (lane & 15);
    if (row < M && col < N) {
      double val = acc[q];
      if (SCALE) val = val / (cx * lamx[col] + cy * lamy[row]);
      Cm[row * ldc + col] = val;
    }
  }
}

// an extremum candidate: the largest key, among equal keys the lowest cell index
struct FvBest {
  double key;
  int idx;
  __device__ __forceinline__ void scan(double k, int c) { if (k > key) { key = k; idx = c; } }     // increasing c
  __device__ __forceinline__ void merge(double k, int c) { if (k > key || (k == key && c < idx)) { key = k; idx = c; } }
};
constexpr int kFvPostBest = 5;               // -psi, |omega|, psi in BR, BL, TL
constexpr int kFvPostNone = INT_MAX;         // the cell of an empty candidate
enum { FVP_PSI_MIN, FVP_OMEGA_MAX, FVP_BR, FVP_BL, FVP_TL };

__device__ __forceinline__ void fv_post_best_clear(FvBest (&best)[kFvPostBest]) {
#pragma unroll
  for (int q = 0; q < kFvPostBest; ++q) { best[q].key = -HUGE_VAL; best[q].idx = kFvPostNone; }
}

// cell c into the five candidates of a thread that takes its cells in increasing c (strict comparisons); true if psi is
// not finite there
__device__ __forceinline__ bool fv_post_cell_extrema(int c, int nx, const double* psi, const double* omega, int ix_lt,
                                                     int ix_gt, int jy_lt, int jy_gt, FvBest (&best)[kFvPostBest]) {
  const int i = c % nx, j = c / nx;
  const double ps = psi[c], om = omega[c];
  best[FVP_PSI_MIN].scan(-ps, c);
  best[FVP_OMEGA_MAX].scan(fabs(om), c);
  const bool left = i < ix_lt, right = i >= ix_gt, low = j < jy_lt, high = j >= jy_gt;
  if (right && low) best[FVP_BR].scan(ps, c);
  if (left && low) best[FVP_BL].scan(ps, c);
  if (left && high) best[FVP_TL].scan(ps, c);
  return !(fabs(ps) <= 1.7976931348623157e308);
}

// the five candidates of all threads of a work-group of WAVES waves merged in a fixed order: xor shuffles inside a wave,
// then the waves in order from LDS; every thread gets the same winners
template <int WAVES>
__device__ __forceinline__ void fv_post_best_merge(FvBest (&best)[kFvPostBest], double (*lkey)[kFvPostBest],
                                                   int (*lidx)[kFvPostBest]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < kFvPostBest; ++q) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double k = __shfl_xor(best[q].key, off);
      const int c = __shfl_xor(best[q].idx, off);
      best[q].merge(k, c);
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < kFvPostBest; ++q) { lkey[w][q] = best[q].key; lidx[w][q] = best[q].idx; }
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < kFvPostBest; ++q) {
    best[q].key = lkey[0][q]; best[q].idx = lidx[0][q];
    for (int v = 1; v < WAVES; ++v) best[q].merge(lkey[v][q], lidx[v][q]);
  }
}

// the result block LDC_FV_POST_* of a trial of n cells from the winners, by ONE thread
__device__ __forceinline__ void fv_post_result(int n, const double* psi, const double* omega,
                                               const FvBest (&best)[kFvPostBest], int any_bad, double* r) {
  const int cmin = best[FVP_PSI_MIN].idx, cmax = best[FVP_OMEGA_MAX].idx;
  const bool ok = cmin < n && cmax < n;        // (a NaN field leaves a candidate empty; the flag below says so)
  r[LDC_FV_POST_PSI_MIN] = ok ? psi[cmin] : 0.0;
  r[LDC_FV_POST_OMEGA_CENTER] = ok ? omega[cmin] : 0.0;
  r[LDC_FV_POST_OMEGA_MAX] = ok ? omega[cmax] : 0.0;
  r[LDC_FV_POST_PSI_MIN_CELL] = ok ? cmin : -1;
  r[LDC_FV_POST_OMEGA_MAX_CELL] = ok ? cmax : -1;
  for (int q = 0; q < 3; ++q) {                // BR, BL, TL; an empty region: value -inf, cell -1
    const FvBest& b = best[FVP_BR + q];
    r[LDC_FV_POST_PSI_BR + q] = b.key;
    r[LDC_FV_POST_PSI_BR_CELL + q] = b.idx < n ? b.idx : -1;
  }
  r[LDC_FV_POST_NONFINITE] = (any_bad || !ok) ? 1.0 : 0.0;
  for (int q = LDC_FV_POST_NONFINITE + 1; q < LDC_FV_POST_RESULT_LEN; ++q) r[q] = 0.0;
}

}  // namespace

#endif  // LDC_FV_POST_CELLS_INC
