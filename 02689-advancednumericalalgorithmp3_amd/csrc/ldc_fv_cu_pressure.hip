// ldc_fv_cu_pressure.hip -- the SIMPLE iteration of a one-CU trial with the consistent pressure equation
// (include/ldc_fv.h, "The consistent pressure equation of a one-CU trial"; ldc_fv_set_pressure).
//
// A translation unit of its own: the one-CU kernel and the spectral kernels beside it in ldc_kernels.hip change with any
// function around them (ldc_fv_kernel.inc, ldc_fv_cells.inc, profiles/fv_wide.md), so fv_cu_pressure_kernel lives here and
// that code object stays what it was.
//
// Mapping: that of fv_kernel (ldc_fv_kernel.inc).  ONE work-group of 512 threads advances ONE trial for a whole chunk of
// iterations, cells tid, tid + 512, ..., every sum through fv_reduce / FvRed, the descriptor pointer read from the kernarg
// segment; a launch of B trials is B independent work-groups.  Per iteration:
//   1. fv_assemble, 2. fv_bicgstab          unchanged (ldc_fv_cu_phases.inc)
//   3. fv_cu_faces      fv_cell_faces on a context whose fluxes point at the dead work vectors PCG_MS: mdot* waits there,
//                       and mdot is not touched before the solve is over (wide_pcg_faces); the sum of rhs_p
//   4. fv_cu_pcg        conjugate gradients on A x = b from x = 0 with z = L+ r, the loop of the chip chain
//                       (ldc_fv_wide_pressure.inc) between barriers where that one has launch boundaries: b, |b|^2; then
//                       per iteration the stop test, four fv_gemm, r.z, p = z + beta p, q = A p and p.q, x += alpha p,
//                       r -= alpha q and |r|^2.  One copy of p: the barrier between its update and the product does what
//                       the chip chain's two alternating copies do.
//   5. fv_correct       unchanged (p' = x - x_0, u' = -D grad p')
//   6. fv_cu_fluxvort   mdot = mdot* - w_f (p'_N - p'_P), walls 0.0, the vorticity (wide_pcg_cell_fluxvort)
//   7. fv_record        unchanged
// The cell arithmetic of the operator is ldc_fv_pressure_cells.inc, shared with the chip chain.
//
// Control flow is uniform: every stop decision is taken from totals that fv_reduce hands identically to every thread, so
// every __syncthreads() is reached by the whole work-group; every loop is bounded (n_iters, max_lin_iters, max_iters; a
// NaN in |r|^2 fails the stop test, runs to the cap, and the record's NaN stops the trial).  Sums run per thread in
// increasing cell index, then wave shuffles, then the waves in order from LDS: no atomics, no flags, no waits, and a
// trial's result does not depend on what else is in the launch.  There is no budget: the loop ends inside the kernel.

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

// this launch's increments of the caller's statistics words (last: the last solve's count)
struct FvCuPcgRun {
  long long iters, solves, caps, last;
};

// ---- 3. fv_face_fluxes with mdot* left in the work vectors PCG_MS; b00 = minus the sum of rhs_p, entry 0 of b
__device__ __forceinline__ void fv_cu_faces(const FvCtx& x, FvRed& red, double& b00) {
  const int n = x.n, tid = threadIdx.x;
  FvCtx xs(x.d);
  xs.fx = x.vec(PCG_MS); xs.fy = xs.fx + x.ny * x.ldx;
  double csum[1] = {0.0};
  for (int c = tid; c < n; c += kFvThreads) {
    double rhs;
    fv_cell_faces(xs, c, rhs);
    csum[0] += rhs;
  }
  red.sum(csum);
  b00 = -csum[0];
}

// ---- 4. A x = b by preconditioned conjugate gradients (tests/fv_consistent_numpy.py::FVConsistentState.pcg)
__device__ __forceinline__ void fv_cu_pcg(const FvCtx& x, const FvCuPcg& P, FvRed& red, double b00, FvCuPcgRun& st) {
  const FvDesc& d = x.d;
  const int nx = x.nx, ny = x.ny, n = x.n, tid = threadIdx.x;
  const double ax = x.dy / x.dx, ay = x.dx / x.dy;
  double bb[1] = {0.0};
  for (int c = tid; c < n; c += kFvThreads) {
    const double b = c == 0 ? b00 : x.vec(FV_C)[c];
    x.vec(PCG_R)[c] = b;
    x.vec(FV_Y)[c] = 0.0;
    bb[0] += b * b;
  }
  red.sum(bb);
  double rr = bb[0], rz_prev = 0.0;
  bool act = bb[0] != 0.0;
  int its = 0;
  for (int it = 0; it < P.max_iters && act; ++it) {
    if (sqrt(rr) <= P.tol * sqrt(bb[0])) { act = false; break; }
    // z = L+ r: W1 = Qy^T R, W2 = W1 Qx / Lambda (zero mode dropped), W1 = Qy W2, Z = W1 Qx^T (wide_pcg_gemm_of)
    fv_gemm<false>(d.Qy, 1, ny, x.vec(PCG_R), nx, 1, x.vec(FV_W1), ny, nx, ny, nullptr, nullptr, 0, 0);
    __syncthreads();
    fv_gemm<true>(x.vec(FV_W1), nx, 1, d.Qx, nx, 1, x.vec(FV_W2), ny, nx, nx, d.lamx, d.lamy, ax, ay);
    __syncthreads();
    fv_gemm<false>(d.Qy, ny, 1, x.vec(FV_W2), nx, 1, x.vec(FV_W1), ny, nx, ny, nullptr, nullptr, 0, 0);
    __syncthreads();
    fv_gemm<false>(x.vec(FV_W1), nx, 1, d.Qx, 1, nx, x.vec(PCG_Z), ny, nx, nx, nullptr, nullptr, 0, 0);
    __syncthreads();
    double rz[1] = {0.0};
    for (int c = tid; c < n; c += kFvThreads) rz[0] += x.vec(PCG_R)[c] * x.vec(PCG_Z)[c];
    red.sum(rz);
    const double beta = it > 0 ? rz[0] / rz_prev : 0.0;
    rz_prev = rz[0];
    for (int c = tid; c < n; c += kFvThreads) {
      double* p = x.vec(PCG_P);
      p[c] = it > 0 ? fma(beta, p[c], x.vec(PCG_Z)[c]) : x.vec(PCG_Z)[c];
    }
    __syncthreads();
    double pq[1] = {0.0};
    for (int c = tid; c < n; c += kFvThreads) {
      const double* p = x.vec(PCG_P);
      const double pc = p[c];
      const double y = wide_pcg_row(x, c, c % nx, c / nx, pc, [&](int k) { return p[k]; });
      x.vec(PCG_Q)[c] = y;
      pq[0] += pc * y;
    }
    red.sum(pq);
    const double alpha = rz[0] / pq[0];
    double r2[1] = {0.0};
    for (int c = tid; c < n; c += kFvThreads) {
      double* r = x.vec(PCG_R);
      x.vec(FV_Y)[c] += alpha * x.vec(PCG_P)[c];
      const double rn = r[c] - alpha * x.vec(PCG_Q)[c];
      r[c] = rn;
      r2[0] += rn * rn;
    }
    red.sum(r2);
    rr = r2[0];
    its = it + 1;
  }
  if (act && sqrt(rr) <= P.tol * sqrt(bb[0])) act = false;      // (converged with the last iteration the cap allows)
  st.iters += its; st.solves += 1; st.caps += act ? 1 : 0; st.last = its;
  __syncthreads();
}

// ---- 6. mdot = mdot* - w_f (p'_N - p'_P) on the inner faces, exactly 0.0 on the walls; the vorticity
__device__ __forceinline__ void fv_cu_fluxvort(const FvCtx& x, double (&part)[kFvRed]) {
  const int n = x.n, tid = threadIdx.x;
  const double *pp = x.vec(FV_Y), *sx = x.vec(PCG_MS), *sy = x.vec(PCG_MS) + x.ny * x.ldx;
  for (int c = tid; c < n; c += kFvThreads) wide_pcg_cell_fluxvort(x, c, pp, sx, sy, part[8]);
  __syncthreads();
}

__global__ __launch_bounds__(kFvThreads) void fv_cu_pressure_kernel(FvLaunch L) {
  __shared__ double lds[2][kFvWaves * kFvRed];
  // (the descriptor pointer from the kernarg segment: fv_kernel says why)
  typedef const FvDesc* FvDescPtr;
  const FvDesc& d = **(const __attribute__((address_space(4))) FvDescPtr*)((kernarg_ptr)__builtin_amdgcn_kernarg_segment_ptr() +
                                                                           __builtin_offsetof(FvLaunch, d) + blockIdx.x * sizeof(FvDescPtr));
  const FvCuPcg& P = *reinterpret_cast<const FvCuPcg*>(reinterpret_cast<const char*>(&d) + kFvCuPcgOffset);
  const FvCtx x(d);
  const FvDebug dbg = {};                    // (phases 5 and 7 are the production instantiations: they read nothing of it)
  FvRed red = {lds, 0};
  FvRun run = {d.ctrl[0], d.ctrl[1], 0, 0, 0, d.ctrl[2] != 0};
  FvCuPcgRun st = {0, 0, 0, 0};
  for (int k = 0; k < L.n_iters && !run.done && !run.nan_seen; ++k) {
    double b2[2];
    fv_assemble(x, red, b2);
    fv_bicgstab(x, red, b2, run);
    double b00;
    fv_cu_faces(x, red, b00);
    fv_cu_pcg(x, P, red, b00, st);
    double part[kFvRed] = {0.0};           // the sums of the record row (fv_correct)
    fv_correct<false>(x, part, dbg);
    fv_cu_fluxvort(x, part);
    fv_record<false>(x, red, part, k, run, dbg);
  }
  if (threadIdx.x == 0) {
    d.ctrl[0] = run.done; d.ctrl[1] = run.iter; d.ctrl[2] = run.nan_seen ? 1 : 0;
    d.ctrl[3] += run.giveups; d.ctrl[4] += run.lin_iters; d.ctrl[5] += run.solves;
    P.stats[0] += st.iters; P.stats[1] += st.solves; P.stats[2] += st.caps;
    if (st.solves) P.stats[3] = st.last;
  }
}

}  // namespace

int ldc_fv_cu_pressure_launch(ldc_fv* const* hs, int n, int n_iters, void* stream) {
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) return LDC_E_NODEVICE;
  for (int lo = 0; lo < n; lo += LDC_FV_LAUNCH_MAX) {
    FvLaunch L;
    const int b = n - lo < LDC_FV_LAUNCH_MAX ? n - lo : LDC_FV_LAUNCH_MAX;
    for (int q = 0; q < b; ++q) {
      if (hs[lo + q]->device != dev || hs[lo + q]->pressure_mode != LDC_FV_PRESSURE_CONSISTENT) return LDC_E_STATE;
      L.d[q] = hs[lo + q]->dev;
    }
    for (int q = b; q < LDC_FV_LAUNCH_MAX; ++q) L.d[q] = nullptr;
    L.n_iters = n_iters;
    hipLaunchKernelGGL(fv_cu_pressure_kernel, dim3(b), dim3(kFvThreads), 0, as_stream(stream), L);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  return 0;
}
