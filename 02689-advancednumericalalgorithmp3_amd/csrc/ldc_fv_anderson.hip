// ldc_fv_anderson.hip -- Anderson acceleration of the finite-volume SIMPLE iteration (include/ldc_fv.h,
// ldc_fv_anderson_enqueue).  A translation unit of its own, linked into libldc_hip.so beside ldc_kernels.hip,
// ldc_fv_post.hip and ldc_fv_prolong.hip: the code object of the solve kernels is the same with and without this file,
// and the solve kernel is reached through the exported ldc_fv_batch_enqueue only.
//
// The outer iteration is the fixed-point map x -> g = SIMPLE(x) on [u | v | p | mdot].  An accelerated chunk of k
// iterations is k launches of ONE iteration, each followed by fv_anderson_kernel, all enqueued on the caller's stream.
//
// Mapping: ONE work-group of 512 threads per trial; a launch of B trials is B independent work-groups (no flags, no
// spins, nobody waits for anybody).  For its trial the kernel runs
//   1. fv_anderson_push    f = g - x, the new columns dG = g - g_prev, dF = f - f_prev into the ring, g_prev, f_prev
//   2. fv_anderson_gram    A = dF^T dF, b = dF^T f over u, v, p, four rows of A per pass over the columns
//   3. fv_anderson_solve   A + lambda I = R^T R and gamma by one thread, in LDS; a bad pivot or gamma: the fallback
//   4. fv_anderson_mix     x_next = g - sum_i gamma_i dG_i into the state and into x; p[0] = 0.0
// hist = [ x | g_prev | f_prev | dG[depth] | dF[depth] ], L doubles each.  The kernel is memory-bound: phase 2 reads the
// m columns ceil(m / 4) times (the Gram matrix is recomputed in full, nothing but hist and astate lives between
// launches), the others read or write each column they touch once.
//
// Sums run in a fixed order: per thread in increasing index, xor shuffles inside a wave, the eight waves in order from
// LDS (as fv_post_kernel reduces).  So a trial's result does not depend on what else is in the launch.
//
// The arithmetic is NOT written here: the constants, the view of hist, push and mix for one entry, one entry into a row
// block of the Gram sums and the Cholesky solve are the functions of ldc_fv_anderson_cells.inc, which the chip mapping
// calls too (ldc_fv_wide_anderson.inc).  What this unit adds is the mapping: the launch arguments, the record-row
// shuffle, the gate and astate, the loops of a work-group of 512 threads, the sums over its eight waves and the barriers.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ldc_hip.h"
#include "ldc_fv_common.inc"
#include "ldc_fv_anderson_cells.inc"

namespace {

typedef const __attribute__((address_space(4))) char* kernarg_ptr;

struct FvAndersonLaunch {                                  // 32 bytes per trial
  const FvDesc* d[LDC_FV_ANDERSON_LAUNCH_MAX];
  double* hist[LDC_FV_ANDERSON_LAUNCH_MAX];
  long long* astate[LDC_FV_ANDERSON_LAUNCH_MAX];
  int depth[LDC_FV_ANDERSON_LAUNCH_MAX], start[LDC_FV_ANDERSON_LAUNCH_MAX];
};
struct FvAndersonTrial {
  const FvDesc* d;
  double* hist;
  long long* astate;
  int depth, start;
};
// member `field` of trial blockIdx.x straight from the kernarg segment, as fv_kernel reads its descriptor pointer:
// indexing the by-value arrays with blockIdx.x would make the compiler materialise them in registers
#define FV_AA_ARG(type, field)                                                                          \
  (*(const __attribute__((address_space(4))) type*)((kernarg_ptr)__builtin_amdgcn_kernarg_segment_ptr() + \
                                                    __builtin_offsetof(FvAndersonLaunch, field) + blockIdx.x * sizeof(type)))
static_assert(sizeof(FvAndersonLaunch) + 2 * sizeof(int) <= 3600, "kernel arguments");

// Every launch of ONE iteration writes rec row 0, so row 0 of the enqueue waits in the last bytes of the descriptor
// slot (behind the post block of ldc_fv_post.hip, which ends at byte 328) until the trial's last iteration of the enqueue
constexpr int kFvAaKeepOffset = (LDC_FV_DESC_DOUBLES - LDC_FV_REC_LEN) * sizeof(double);
static_assert(kFvAaKeepOffset >= 384 && sizeof(FvDesc) <= 256, "the kept row sits behind the descriptor and the post block");

// the record row of iteration j of the enqueue into its place: the launch wrote it to row 0.  `last`: no launch of this
// enqueue writes row 0 after this one, so row 0 gets the row of iteration 0 back.  Thread t moves entry t of each row.
__device__ __forceinline__ void fv_anderson_record(const FvDesc& d, int j, bool last) {
  if (threadIdx.x >= LDC_FV_REC_LEN) return;
  double* keep = reinterpret_cast<double*>(reinterpret_cast<char*>(const_cast<FvDesc*>(&d)) + kFvAaKeepOffset);
  const double r = d.rec[threadIdx.x];
  if (j == 0) {
    if (!last) keep[threadIdx.x] = r;
  } else {
    d.rec[(long long)j * LDC_FV_REC_LEN + threadIdx.x] = r;
    if (last) d.rec[threadIdx.x] = keep[threadIdx.x];
  }
}

// ---- 1. f = g - x; the new columns into ring slot `slot` (push); g_prev = g, f_prev = f; without mixing x = g at once
__device__ __forceinline__ void fv_anderson_push(const FvDesc& d, const FvAaHist& H, int n, bool has_f, bool push,
                                                 int slot, bool keep_g) {
  const int L = (int)H.L;
  double *dGs = H.dG + slot * H.L, *dFs = H.dF + slot * H.L;
  for (int e = threadIdx.x; e < L; e += kFvThreads) fv_anderson_push_entry(d, H, n, e, has_f, push, dGs, dFs, keep_g);
  __syncthreads();
}

// ---- 2. A[i][k] = dF_i . dF_k, b[i] = dF_i . f over the first n3 entries, rows i0 .. i0 + 3 per pass
__device__ __forceinline__ void fv_anderson_gram(const FvAaHist& H, int n3, int m, double (*part)[kFvAaSums],
                                                 double (*A)[kFvAaDepth + 1], double* b) {
  for (int i0 = 0; i0 < m; i0 += kFvAaRows) {
    double acc[kFvAaRows][kFvAaDepth + 1];
    fv_anderson_acc_clear(acc);
    for (int e = threadIdx.x; e < n3; e += kFvThreads) fv_anderson_acc_entry(H, m, i0, e, acc);
    fv_anderson_acc_wave(acc, part);
    __syncthreads();
    if (threadIdx.x < kFvAaSums) {
      double s = part[0][threadIdx.x];
      for (int v = 1; v < kFvWaves; ++v) s += part[v][threadIdx.x];
      const int i = i0 + threadIdx.x / (kFvAaDepth + 1), k = threadIdx.x % (kFvAaDepth + 1);
      if (i < m) {
        if (k < kFvAaDepth) A[i][k] = s;
        else b[i] = s;
      }
    }
    __syncthreads();
  }
}

// ---- 3. is fv_anderson_solve of ldc_fv_anderson_cells.inc, which thread 0 calls on A, b and gamma in LDS
// ---- 4. x_next into the state and x, every entry
__device__ __forceinline__ void fv_anderson_mix(const FvDesc& d, const FvAaHist& H, int n, int m, bool fell,
                                                const double* gamma) {
  const int L = (int)H.L;
  for (int e = threadIdx.x; e < L; e += kFvThreads) fv_anderson_mix_entry(d, H, n, e, m, fell, gamma);
}

__global__ __launch_bounds__(kFvThreads) void fv_anderson_kernel(FvAndersonLaunch, int j, int n_iters) {
  __shared__ double part[kFvWaves][kFvAaSums];
  __shared__ double A[kFvAaDepth][kFvAaDepth + 1];
  __shared__ double b[kFvAaDepth], gamma[kFvAaDepth];
  __shared__ int fell_s;
  typedef const FvDesc* FvDescPtr;
  typedef double* FvHistPtr;
  typedef long long* FvWordPtr;
  const FvAndersonTrial T = {FV_AA_ARG(FvDescPtr, d), FV_AA_ARG(FvHistPtr, hist), FV_AA_ARG(FvWordPtr, astate),
                             FV_AA_ARG(int, depth), FV_AA_ARG(int, start)};
  const FvDesc& d = *T.d;
  const long long it = d.ctrl[1], seen = T.astate[2];
  if (it == seen) return;                                  // the SIMPLE launch did nothing: latched, NaN or capped
  long long ncol = T.astate[0], pos = T.astate[1];
  const long long fallbacks = T.astate[3];
  const bool stopped = d.ctrl[0] != 0 || d.ctrl[2] != 0;
  fv_anderson_record(d, j, stopped || j == n_iters - 1);
  __syncthreads();                                         // (every thread has read astate: thread 0 may write it)
  if (stopped || T.depth == 0) {
    if (threadIdx.x == 0) T.astate[2] = it;
    return;
  }
  const int n = d.nx * d.ny, depth = T.depth;
  const FvAaHist H(T.hist, 3LL * n + LDC_FV_FACES(d.nx, d.ny), depth);
  if (ncol < 0 || ncol > depth || pos < 0 || pos >= depth) { ncol = 0; pos = 0; }        // (words nobody zeroed)
  const bool has_f = seen >= 1, push = seen >= 2;          // x is known from the 2nd iteration on, g_prev from the 3rd
  const int slot = (int)pos;
  const int m = push ? (ncol < depth ? (int)ncol + 1 : depth) : (int)ncol;
  const bool mix = has_f && it >= T.start && m > 0;
  fv_anderson_push(d, H, n, has_f, push, slot, !mix);
  bool fell = false;
  if (mix) {
    fv_anderson_gram(H, 3 * n, m, part, A, b);
    if (threadIdx.x == 0) fell_s = fv_anderson_solve(m, A, b, gamma) ? 0 : 1;
    __syncthreads();
    fell = fell_s != 0;
    fv_anderson_mix(d, H, n, m, fell, gamma);
  }
  if (threadIdx.x == 0) {
    T.astate[0] = fell ? 0 : m;
    T.astate[1] = fell ? 0 : (push ? (slot + 1) % depth : slot);
    T.astate[2] = it;
    T.astate[3] = fallbacks + (fell ? 1 : 0);
  }
}

}  // namespace

extern "C" {

int ldc_fv_anderson_enqueue(ldc_fv* const* hs, const struct ldc_fv_anderson* acc, int n, int n_iters, void* stream) {
  if (!hs || !acc || n < 1 || n_iters < 1) return LDC_E_ARG;
  for (int q = 0; q < n; ++q) {
    if (!hs[q]) return LDC_E_STATE;
    const struct ldc_fv_anderson& a = acc[q];
    if (a.depth < 0 || a.depth > LDC_FV_ANDERSON_MAX_DEPTH || a.start < 1 || !a.astate) return LDC_E_ARG;
    if (n_iters > hs[q]->rec_cap) return LDC_E_ARG;
    if (a.depth > 0 && (!a.hist || a.hist_len < LDC_FV_ANDERSON_HIST_LEN(hs[q]->nx, hs[q]->ny, a.depth))) return LDC_E_ARG;
  }
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) return LDC_E_NODEVICE;
  for (int q = 0; q < n; ++q) if (hs[q]->device != dev) return LDC_E_STATE;
  for (int j = 0; j < n_iters; ++j) {
    const int rc = ldc_fv_batch_enqueue(hs, n, 1, stream);
    if (rc != 0) return rc;
    for (int lo = 0; lo < n; lo += LDC_FV_ANDERSON_LAUNCH_MAX) {
      FvAndersonLaunch L;
      const int b = n - lo < LDC_FV_ANDERSON_LAUNCH_MAX ? n - lo : LDC_FV_ANDERSON_LAUNCH_MAX;
      for (int q = 0; q < LDC_FV_ANDERSON_LAUNCH_MAX; ++q) {
        const struct ldc_fv_anderson* a = q < b ? &acc[lo + q] : nullptr;
        L.d[q] = a ? hs[lo + q]->dev : nullptr;
        L.hist[q] = a ? a->hist : nullptr;
        L.astate[q] = a ? reinterpret_cast<long long*>(a->astate) : nullptr;
        L.depth[q] = a ? a->depth : 0;
        L.start[q] = a ? a->start : 1;
      }
      hipLaunchKernelGGL(fv_anderson_kernel, dim3(b), dim3(kFvThreads), 0, as_stream(stream), L, j, n_iters);
      const hipError_t e = hipGetLastError();
      if (e != hipSuccess) return (int)e;
    }
  }
  return 0;
}

}  // extern "C"
