// ldc_fv_post.hip -- streamfunction and vortex metrics of finite-volume trials on the device (include/ldc_fv.h,
// ldc_fv_post_enqueue).  A translation unit of its own, linked into libldc_hip.so beside ldc_kernels.hip: its kernels
// live in their own code object, so the code object of the solve kernels is the same with and without this file.
//
// Reference: base.py:569-760 (streamfunction and vortex extrema), as solvers/fv/solver.py restates them on the host.
//
// Mapping: ONE work-group of 512 threads post-processes ONE trial; a launch of B trials is B independent work-groups
// (no flags, no spins, nobody waits for anybody).  fv_post_kernel reads the trial's descriptor and its post block
// (both in the slot in the tail of the trial's work buffer) and runs four phases, each ending on the barrier the next
// one needs:
//   1. fv_post_vorticity   omega at every cell by ghost cells (the arithmetic of fv_flux_vorticity), the psi ring = 0
//   2. fv_post_psi         psi on the interior cells: the 5-point Dirichlet problem solved exactly by fast
//                          diagonalisation with the analytic sine eigenvectors, four GEMMs on v_mfma_f64_16x16x4_f64
//   3. fv_post_extrema     argmin psi, argmax |omega|, argmax psi inside BR, BL, TL: ties to the lowest cell index
//   4. the result block    LDC_FV_POST_* of ldc_fv.h
// The interior is mx x my = (nx - 2) x (ny - 2); with T = tridiag(-1, 2, -1), cx = 1 / dx^2, cy = 1 / dy^2 the host's
// system is (cx Tx + cy Ty) psi = omega, and T = S diag(lam) S^T with S the sine vectors, so
//   psi = Sy ((Sy^T F Sx) / (cy lamy[a] + cx lamx[b])) Sx^T,   F = omega on the interior.
// Scratch: the trial's work vectors FV_W1 and FV_W2 (work vectors carry nothing between launches of the solve kernel,
// and the trial is not in flight while it is post-processed).
//
// The post blocks reach the device through fv_post_stage_kernel: the structs travel as kernel arguments and one thread
// per trial writes them behind the descriptor.  Stream-ordered, no host synchronisation, no library-owned staging.
//
// The arithmetic is NOT written here: one cell of omega, one GEMM tile, the candidates with their scan and merge and the
// result block are the functions of ldc_fv_post_cells.inc, which ldc_fv_wide.hip calls too (fv_wide_post_*: the same
// chain for a chip or shared trial, one launch per phase).  What this unit adds is the mapping: the post block and its
// staging, the loops of a work-group of 512 threads over cells and tiles, and the barriers between the phases.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ldc_hip.h"
#include "ldc_fv_common.inc"
#include "ldc_fv_post_cells.inc"

namespace {

typedef const __attribute__((address_space(4))) char* kernarg_ptr;

// the post block on the device, at byte kFvPostOffset of the descriptor slot
struct FvPost {
  const double *Sx, *lamx, *Sy, *lamy;
  double *psi, *omega, *result;
  int ix_lt, ix_gt, jy_lt, jy_gt;
};
constexpr int kFvPostOffset = 256;
static_assert(sizeof(FvDesc) <= kFvPostOffset, "the post block sits behind the descriptor");
static_assert(kFvPostOffset + sizeof(FvPost) <= LDC_FV_DESC_DOUBLES * sizeof(double), "descriptor slot");

__host__ __device__ inline FvPost* fv_post_slot(const FvDesc* d) {
  return reinterpret_cast<FvPost*>(reinterpret_cast<char*>(const_cast<FvDesc*>(d)) + kFvPostOffset);
}

constexpr int kFvStageMax = 40;              // post blocks per staging launch: 40 x (8 + 72) bytes of arguments
struct FvPostStage {
  const FvDesc* d[kFvStageMax];
  FvPost p[kFvStageMax];
};
static_assert(sizeof(FvPostStage) <= 3600, "kernel arguments");

__global__ __launch_bounds__(64) void fv_post_stage_kernel(FvPostStage S, int n) {
  const int q = threadIdx.x;
  if (q < n) *fv_post_slot(S.d[q]) = S.p[q];
}

struct FvPostLaunch {
  const FvDesc* d[LDC_FV_LAUNCH_MAX];
};

// one GEMM of the fast diagonalisation: one wave per 16 x 16 tile, round-robin
template <bool SCALE>
__device__ void fv_post_gemm(const double* A, int sar, int sak, const double* B, int sbk, int sbc, double* Cm, int ldc,
                             int M, int N, int K, const double* lamx, const double* lamy, double cx, double cy) {
  const int w = threadIdx.x >> 6;
  const int tiles = ((M + 15) >> 4) * ((N + 15) >> 4);
  for (int t = w; t < tiles; t += kFvWaves)
    fv_post_gemm_tile<SCALE>(t, A, sar, sak, B, sbk, sbc, Cm, ldc, M, N, K, lamx, lamy, cx, cy);
}

// ---- 1. omega at every cell, psi = 0 on the boundary ring; true if this thread saw a value that is not finite
__device__ __forceinline__ bool fv_post_vorticity(const FvDesc& d, const FvPost& P) {
  const int nx = d.nx, ny = d.ny, n = nx * ny;
  const double dx = d.dx, dy = d.dy, lid = d.lid;
  const double *u = d.u, *v = d.v;
  bool bad = false;
  for (int c = threadIdx.x; c < n; c += kFvThreads)
    bad |= fv_post_cell_vorticity(c, nx, ny, dx, dy, lid, u, v, P.omega, P.psi);
  __syncthreads();
  return bad;
}

// ---- 2. psi on the interior: W1 = Sy^T F, W2 = W1 Sx / Lambda, W1 = Sy W2, psi = W1 Sx^T
__device__ __forceinline__ void fv_post_psi(const FvDesc& d, const FvPost& P) {
  const int nx = d.nx, mx = d.nx - 2, my = d.ny - 2, n = d.nx * d.ny;
  const double cx = 1.0 / (d.dx * d.dx), cy = 1.0 / (d.dy * d.dy);
  double *W1 = d.work + FV_W1 * n, *W2 = d.work + FV_W2 * n;
  const double* F = P.omega + nx + 1;
  fv_post_gemm<false>(P.Sy, 1, my, F, nx, 1, W1, mx, my, mx, my, nullptr, nullptr, 0, 0);
  __syncthreads();
  fv_post_gemm<true>(W1, mx, 1, P.Sx, mx, 1, W2, mx, my, mx, mx, P.lamx, P.lamy, cx, cy);
  __syncthreads();
  fv_post_gemm<false>(P.Sy, my, 1, W2, mx, 1, W1, mx, my, mx, my, nullptr, nullptr, 0, 0);
  __syncthreads();
  fv_post_gemm<false>(W1, mx, 1, P.Sx, 1, mx, P.psi + nx + 1, nx, my, mx, mx, nullptr, nullptr, 0, 0);
  __syncthreads();
}

// ---- 3. the five extrema over the work-group, in a fixed order; every thread gets the same winners
__device__ __forceinline__ bool fv_post_extrema(const FvDesc& d, const FvPost& P, FvBest (&best)[kFvPostBest],
                                                double (*lkey)[kFvPostBest], int (*lidx)[kFvPostBest]) {
  const int nx = d.nx, n = d.nx * d.ny;
  bool bad = false;
  fv_post_best_clear(best);
  for (int c = threadIdx.x; c < n; c += kFvThreads)
    bad |= fv_post_cell_extrema(c, nx, P.psi, P.omega, P.ix_lt, P.ix_gt, P.jy_lt, P.jy_gt, best);
  fv_post_best_merge<kFvWaves>(best, lkey, lidx);
  return bad;
}

__global__ __launch_bounds__(kFvThreads) void fv_post_kernel(FvPostLaunch) {
  __shared__ double lkey[kFvWaves][kFvPostBest];
  __shared__ int lidx[kFvWaves][kFvPostBest];
  // (the descriptor pointer straight from the kernarg segment, as fv_kernel reads it)
  typedef const FvDesc* FvDescPtr;
  const FvDesc& d = **(const __attribute__((address_space(4))) FvDescPtr*)((kernarg_ptr)__builtin_amdgcn_kernarg_segment_ptr() +
                                                                           __builtin_offsetof(FvPostLaunch, d) + blockIdx.x * sizeof(FvDescPtr));
  const FvPost P = *fv_post_slot(&d);        // (by value: nothing writes the block while the kernel runs)
  bool bad = fv_post_vorticity(d, P);
  fv_post_psi(d, P);
  FvBest best[kFvPostBest];
  bad |= fv_post_extrema(d, P, best, lkey, lidx);
  const int any_bad = __syncthreads_or(bad ? 1 : 0);
  if (threadIdx.x == 0) fv_post_result(d.nx * d.ny, P.psi, P.omega, best, any_bad, P.result);
}

}  // namespace

extern "C" {

int ldc_fv_post_enqueue(ldc_fv* const* hs, const struct ldc_fv_post* posts, int n, void* stream) {
  if (!hs || !posts || n < 1) return LDC_E_ARG;
  for (int q = 0; q < n; ++q) {
    if (!hs[q]) return LDC_E_STATE;
    const struct ldc_fv_post& p = posts[q];
    const void* req[] = {p.Sx, p.lamx, p.Sy, p.lamy, p.psi, p.omega, p.result};
    for (const void* x : req) if (!x) return LDC_E_ARG;
    if (p.ix_lt < 0 || p.ix_gt < 0 || p.jy_lt < 0 || p.jy_gt < 0) return LDC_E_ARG;
  }
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) return LDC_E_NODEVICE;
  for (int q = 0; q < n; ++q) if (hs[q]->device != dev) return LDC_E_STATE;
  for (int lo = 0; lo < n; lo += kFvStageMax) {
    FvPostStage S;
    const int b = n - lo < kFvStageMax ? n - lo : kFvStageMax;
    for (int q = 0; q < kFvStageMax; ++q) {
      const int t = lo + (q < b ? q : 0);
      const struct ldc_fv_post& p = posts[t];
      S.d[q] = hs[t]->dev;
      S.p[q] = FvPost{p.Sx, p.lamx, p.Sy, p.lamy, p.psi, p.omega, p.result, p.ix_lt, p.ix_gt, p.jy_lt, p.jy_gt};
    }
    hipLaunchKernelGGL(fv_post_stage_kernel, dim3(1), dim3(64), 0, as_stream(stream), S, b);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  for (int lo = 0; lo < n; lo += LDC_FV_LAUNCH_MAX) {
    FvPostLaunch L;
    const int b = n - lo < LDC_FV_LAUNCH_MAX ? n - lo : LDC_FV_LAUNCH_MAX;
    for (int q = 0; q < LDC_FV_LAUNCH_MAX; ++q) L.d[q] = q < b ? hs[lo + q]->dev : nullptr;
    hipLaunchKernelGGL(fv_post_kernel, dim3(b), dim3(kFvThreads), 0, as_stream(stream), L);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  return 0;
}

}  // extern "C"
