// ldc_fv_stretched_sep.hip -- the SIMPLE iteration of a one-CU trial on a wall-clustered tensor grid with the consistent
// pressure equation, its CG preconditioned by a separable, scaled operator (include/ldc_fv.h, "The separable scaled
// preconditioner"; ldc_fv_set_preconditioner).
//
// A translation unit of its own, as ldc_fv_stretched.hip is and for the same reason: a trial that does not ask for this
// preconditioner runs fv_stretched_kernel, whose code object stays what it was.  Every phase but the CG loop is that
// kernel's (ldc_fv_stretched_phases.inc, ldc_fv_cu_phases.inc); so are the mapping (ONE work-group of 512 threads per trial,
// cells tid, tid + 512, ...), the reductions, the record and the latch.
//
// The preconditioner.  sg_pcg models A, whose face weights carry D = V / a_P, by Hy (x) Kx + Ky (x) Hx: D left out.  On a
// stretched mesh D varies with V by a factor of 30 ... 250.  Here D is modelled by a product a_i b_j (fitted on the host to
// the D of pure diffusion, once per mesh), which keeps the operator separable,
//     L_s = My (x) Kx^a + Ky^b (x) Mx,   Kx^a: weights rho a_f / d,   Mx = diag(hx a)   (y likewise with b),
// so L_s+ is the four GEMMs of sg_fastdiag with the generalised eigenpairs of (Kx^a, Mx) and (Ky^b, My); what the product
// misses of the actual D is taken by a diagonal scaling (Concus and Golub): s_c = sqrt(a_i b_j / D_c) per solve, and
//     z = s . L_s+ (s . r).
// Per axis one device table [a (n) | lam (n) | Q (n x n, row-major, column k the k-th vector)]; the two pointers live at byte
// 344 of the descriptor slot (FvPrecondBlk).
//
// The loop is sg_pcg's with three pointwise factors and no sweep or barrier more: s is written in the loop that sets r = b,
// s . r in the loops that write r, and s . z' is formed in the loops that read z' = L_s+ (s . r).  s and s . r live in the
// work vectors 15 and 17 (FV_VU, FV_PHU), which BiCGSTAB leaves dead during the pressure solve.
//
// Control flow is uniform (every stop decision is taken from totals that fv_reduce hands identically to every thread), every
// loop is bounded (n_iters, max_lin_iters, max_iters), sums run in the fixed order: no atomics, no flags, no waits, and a
// trial's result does not depend on what else is in the launch.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ldc_hip.h"
#include "ldc_fv_common.inc"
#include "ldc_fv_cells.inc"
#include "ldc_fv_pressure_cells.inc"

namespace {

typedef const __attribute__((address_space(4))) char* kernarg_ptr;

#include "ldc_fv_cu_phases.inc"
#include "ldc_fv_stretched_phases.inc"

// s and s . r: dead vectors of BiCGSTAB, clear of PCG_MS .. PCG_Q (9 .. 14, 16) and of FV_C ... (23 ...)
constexpr FvVec SEP_S = FV_VU, SEP_SR = FV_PHU;
static_assert(SEP_S == 15 && SEP_SR == 17 && SEP_S != PCG_Q && SEP_S > PCG_P && SEP_SR > PCG_Q && SEP_SR < FV_C,
              "the scaling vectors are clear of the CG vectors");

// the tables of both axes
struct SepCtx {
  const double *ax, *lamx, *Qx, *ay, *lamy, *Qy;
  __device__ __forceinline__ SepCtx(const FvCtx& x, const FvPrecondBlk& b)
      : ax(b.px), lamx(b.px + x.nx), Qx(b.px + 2 * x.nx), ay(b.py), lamy(b.py + x.ny), Qy(b.py + 2 * x.ny) {}
};

// out = L_s+ rhs: sg_fastdiag with the eigenpairs of the fitted operator
__device__ __forceinline__ void sep_fastdiag(const FvCtx& x, const SepCtx& t, const double* rhs, double* out) {
  const int nx = x.nx, ny = x.ny;
  fv_gemm<false>(t.Qy, 1, ny, rhs, nx, 1, x.vec(FV_W1), ny, nx, ny, nullptr, nullptr, 0, 0);
  __syncthreads();
  fv_gemm<true>(x.vec(FV_W1), nx, 1, t.Qx, nx, 1, x.vec(FV_W2), ny, nx, nx, t.lamx, t.lamy, 1.0, 1.0);
  __syncthreads();
  fv_gemm<false>(t.Qy, ny, 1, x.vec(FV_W2), nx, 1, x.vec(FV_W1), ny, nx, ny, nullptr, nullptr, 0, 0);
  __syncthreads();
  fv_gemm<false>(x.vec(FV_W1), nx, 1, t.Qx, 1, nx, out, ny, nx, nx, nullptr, nullptr, 0, 0);
  __syncthreads();
}

// sg_pcg with z = s . L_s+ (s . r): PCG_Z holds z' = L_s+ (s . r), every reader multiplies by s
__device__ __forceinline__ void sep_pcg(const SgCtx& s, const SepCtx& t, const FvCuPcg& P, FvRed& red, double b00,
                                        SgPcgRun& st) {
  const FvCtx& x = s.x;
  const int nx = x.nx, n = x.n, tid = threadIdx.x;
  double bb[1] = {0.0};
  for (int c = tid; c < n; c += kFvThreads) {
    const int i = c % nx, j = c / nx;
    const double b = c == 0 ? b00 : x.vec(FV_C)[c];
    const double sc = sqrt((t.ax[i] * t.ay[j]) / s.D(c, i, j));
    x.vec(PCG_R)[c] = b;
    x.vec(SEP_S)[c] = sc;
    x.vec(SEP_SR)[c] = sc * b;
    x.vec(FV_Y)[c] = 0.0;
    bb[0] += b * b;
  }
  red.sum(bb);
  double rr = bb[0], rz_prev = 0.0;
  bool act = bb[0] != 0.0;
  int its = 0;
  for (int it = 0; it < P.max_iters && act; ++it) {
    if (sqrt(rr) <= P.tol * sqrt(bb[0])) { act = false; break; }
    sep_fastdiag(x, t, x.vec(SEP_SR), x.vec(PCG_Z));
    double rz[1] = {0.0};
    for (int c = tid; c < n; c += kFvThreads) rz[0] += x.vec(SEP_SR)[c] * x.vec(PCG_Z)[c];
    red.sum(rz);
    const double beta = it > 0 ? rz[0] / rz_prev : 0.0;
    rz_prev = rz[0];
    for (int c = tid; c < n; c += kFvThreads) {
      double* p = x.vec(PCG_P);
      const double z = x.vec(SEP_S)[c] * x.vec(PCG_Z)[c];
      p[c] = it > 0 ? fma(beta, p[c], z) : z;
    }
    __syncthreads();
    double pq[1] = {0.0};
    for (int c = tid; c < n; c += kFvThreads) {
      const double* p = x.vec(PCG_P);
      const double y = sg_row(s, c, c % nx, c / nx, p);
      x.vec(PCG_Q)[c] = y;
      pq[0] += p[c] * y;
    }
    red.sum(pq);
    const double alpha = rz[0] / pq[0];
    double r2[1] = {0.0};
    for (int c = tid; c < n; c += kFvThreads) {
      double* r = x.vec(PCG_R);
      x.vec(FV_Y)[c] += alpha * x.vec(PCG_P)[c];
      const double rn = r[c] - alpha * x.vec(PCG_Q)[c];
      r[c] = rn;
      x.vec(SEP_SR)[c] = x.vec(SEP_S)[c] * rn;
      r2[0] += rn * rn;
    }
    red.sum(r2);
    rr = r2[0];
    its = it + 1;
  }
  if (act && sqrt(rr) <= P.tol * sqrt(bb[0])) act = false;
  st.iters += its; st.solves += 1; st.caps += act ? 1 : 0; st.last = its;
  __syncthreads();
}

__global__ __launch_bounds__(kFvThreads) void fv_stretched_sep_kernel(FvLaunch L) {
  __shared__ double lds[2][kFvWaves * kFvRed];
  // (the descriptor pointer from the kernarg segment: fv_kernel says why)
  typedef const FvDesc* FvDescPtr;
  const FvDesc& d = **(const __attribute__((address_space(4))) FvDescPtr*)((kernarg_ptr)__builtin_amdgcn_kernarg_segment_ptr() +
                                                                           __builtin_offsetof(FvLaunch, d) + blockIdx.x * sizeof(FvDescPtr));
  const FvCuPcg& P = *reinterpret_cast<const FvCuPcg*>(reinterpret_cast<const char*>(&d) + kFvCuPcgOffset);
  const FvGridBlk& G = *reinterpret_cast<const FvGridBlk*>(reinterpret_cast<const char*>(&d) + kFvGridOffset);
  const FvPrecondBlk& B = *reinterpret_cast<const FvPrecondBlk*>(reinterpret_cast<const char*>(&d) + kFvPrecondOffset);
  const FvCtx x(d);
  const SgCtx s(x, G);
  const SepCtx t(x, B);
  FvRed red = {lds, 0};
  FvRun run = {d.ctrl[0], d.ctrl[1], 0, 0, 0, d.ctrl[2] != 0};
  SgPcgRun st = {0, 0, 0, 0};
  for (int k = 0; k < L.n_iters && !run.done && !run.nan_seen; ++k) {
    double b2[2];
    sg_assemble(s, red, b2);
    fv_bicgstab(x, red, b2, run);
    double b00;
    sg_faces<true>(s, red, b00);
    sep_pcg(s, t, P, red, b00, st);
    double part[kFvRed] = {0.0};
    sg_correct(s, part);
    sg_fluxvort<true>(s, part);
    sg_record(s, red, part, k, run);
  }
  if (threadIdx.x == 0) {
    d.ctrl[0] = run.done; d.ctrl[1] = run.iter; d.ctrl[2] = run.nan_seen ? 1 : 0;
    d.ctrl[3] += run.giveups; d.ctrl[4] += run.lin_iters; d.ctrl[5] += run.solves;
    P.stats[0] += st.iters; P.stats[1] += st.solves; P.stats[2] += st.caps;
    if (st.solves) P.stats[3] = st.last;
  }
}

}  // namespace

int ldc_fv_stretched_sep_launch(ldc_fv* const* hs, int n, int n_iters, void* stream) {
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) return LDC_E_NODEVICE;
  for (int lo = 0; lo < n; lo += LDC_FV_LAUNCH_MAX) {
    FvLaunch L;
    const int b = n - lo < LDC_FV_LAUNCH_MAX ? n - lo : LDC_FV_LAUNCH_MAX;
    for (int q = 0; q < b; ++q) {
      const ldc_fv* h = hs[lo + q];
      if (h->device != dev || h->grid_mode != LDC_FV_GRID_TABLES || h->pressure_mode != LDC_FV_PRESSURE_CONSISTENT ||
          h->precond_mode != LDC_FV_PRECOND_SEPARABLE)
        return LDC_E_STATE;
      L.d[q] = h->dev;
    }
    for (int q = b; q < LDC_FV_LAUNCH_MAX; ++q) L.d[q] = nullptr;
    L.n_iters = n_iters;
    hipLaunchKernelGGL(fv_stretched_sep_kernel, dim3(b), dim3(kFvThreads), 0, as_stream(stream), L);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  return 0;
}
