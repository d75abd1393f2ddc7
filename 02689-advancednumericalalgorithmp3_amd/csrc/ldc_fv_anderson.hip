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

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ldc_hip.h"
#include "ldc_fv_common.inc"

namespace {

typedef const __attribute__((address_space(4))) char* kernarg_ptr;

constexpr int kFvAaDepth = LDC_FV_ANDERSON_MAX_DEPTH;
constexpr int kFvAaRows = 4;                             // rows of A per pass of phase 2
constexpr int kFvAaSums = kFvAaRows * (kFvAaDepth + 1);  // per pass: 4 x (16 entries of A, 1 of b)
constexpr double kFvAaLambda = 1e-12;
static_assert(kFvAaDepth % kFvAaRows == 0, "row blocks");

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

// ---- 1. f = g - x; the new columns into ring slot `slot` (push); g_prev = g, f_prev = f; without mixing x = g at once
__device__ __forceinline__ void fv_anderson_push(const FvDesc& d, const FvAaHist& H, int n, bool has_f, bool push,
                                                 int slot, bool keep_g) {
  const int L = (int)H.L;
  double *dGs = H.dG + slot * H.L, *dFs = H.dF + slot * H.L;
  for (int e = threadIdx.x; e < L; e += kFvThreads) {
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
  __syncthreads();
}

// ---- 2. A[i][k] = dF_i . dF_k, b[i] = dF_i . f over the first n3 entries, rows i0 .. i0 + 3 per pass
__device__ __forceinline__ void fv_anderson_gram(const FvAaHist& H, int n3, int m, double (*part)[kFvAaSums],
                                                 double (*A)[kFvAaDepth + 1], double* b) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int i0 = 0; i0 < m; i0 += kFvAaRows) {
    double acc[kFvAaRows][kFvAaDepth + 1];
#pragma unroll
    for (int r = 0; r < kFvAaRows; ++r)
#pragma unroll
      for (int k = 0; k <= kFvAaDepth; ++k) acc[r][k] = 0.0;
    for (int e = threadIdx.x; e < n3; e += kFvThreads) {
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

// ---- 3. (A + lambda I) gamma = b by Cholesky, one thread; false: a pivot that is not > 0 or a gamma that is not finite
//         (wide_mix_solve of ldc_fv_wide_anderson.inc is a copy: a change to one goes into the other)
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

// ---- 4. x_next = g - sum_i gamma_i dG_i (slot order) into the state and x; the pinned cell's p is written as 0.0.
//         The fallback leaves the state (it is g) and keeps g as x.
__device__ __forceinline__ void fv_anderson_mix(const FvDesc& d, const FvAaHist& H, int n, int m, bool fell,
                                                const double* gamma) {
  const int L = (int)H.L;
  for (int e = threadIdx.x; e < L; e += kFvThreads) {
    double xn = H.gp[e];
    if (!fell) {
      for (int k = 0; k < m; ++k) xn -= gamma[k] * H.dG[k * H.L + e];
      if (e == 2 * n) xn = 0.0;
      *fv_state_at(d, n, e) = xn;
    }
    H.x[e] = xn;
  }
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

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

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
