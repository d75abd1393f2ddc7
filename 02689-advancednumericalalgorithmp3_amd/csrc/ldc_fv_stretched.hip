// ldc_fv_stretched.hip -- the SIMPLE iteration of a one-CU trial on a wall-clustered tensor grid, with either pressure
// equation (include/ldc_fv.h, "Stretched grids of a one-CU trial"; ldc_fv_set_grid).
//
// A translation unit of its own, as ldc_fv_cu_pressure.hip is and for the same reason: fv_kernel and fv_cu_pressure_kernel
// change with any function around them, so fv_stretched_kernel lives here and those code objects stay what they were.
// Nothing of ldc_fv_cells.inc, ldc_fv_pressure_cells.inc or ldc_fv_cu_phases.inc is touched; where a cell body is needed
// with the geometry read from tables, it is defined in ldc_fv_stretched_phases.inc (shared with ldc_fv_stretched_sep.hip) and
// names its twin.
//
// Mapping: that of fv_kernel (ldc_fv_kernel.inc).  ONE work-group of 512 threads advances ONE trial for a whole chunk of
// iterations, cells tid, tid + 512, ..., every sum through fv_reduce / FvRed, the descriptor pointer read from the kernarg
// segment; a launch of B trials is B independent work-groups.  Per iteration:
//   1. sg_assemble      grad p, five diagonals, right-hand sides from the tables             (twin: fv_cell_assemble)
//   2. fv_bicgstab      unchanged (ldc_fv_cu_phases.inc): it reads the stored diagonals only
//   3. sg_faces         g-weighted Rhie-Chow face fluxes mdot*, rhs_p and its sum            (twin: fv_cell_faces)
//   4. reference:  the four fv_gemm of the fast diagonalisation with ax = ay = 1 and the generalised eigenpairs
//      consistent: sg_pcg, the loop of fv_cu_pcg with sg_row for A p                         (twin: wide_pcg_row)
//   5. sg_correct       p' = y - y_0, u' = -D grad p', the record sums weighted by V         (twin: fv_correct)
//   6. reference:  mdot += rho interp(u', v') |S|, walls rho u'_P |S| (FV-Q4)                (twin: fv_cell_flux_vorticity)
//      consistent: mdot = mdot* - w_f (p'_N - p'_P), walls 0.0                               (twin: wide_pcg_cell_fluxvort)
//      both: omega by the Gauss rule (f_e - f_w) / h with the walls' own values
//   7. sg_record        div mdot, |grad omega|^2 V, the record row (fv_rec_rel, fv_rec_row) and the latch
// Geometry: per axis one device table [h (n) | d (n + 1) | g (n + 1)]: cell widths; per face k = 0 .. n the distance between
// the centres it separates (walls: h / 2) and the weight of the cell behind it, phi_f = g phi_N + (1 - g) phi_P (walls: not
// read).  The two pointers live at byte 328 of the descriptor slot (FvGridBlk); FvDesc is what it was.
//
// Control flow is uniform (CONSISTENT is a template parameter; every stop decision is taken from totals that fv_reduce hands
// identically to every thread), every loop is bounded (n_iters, max_lin_iters, max_iters), sums run per thread in increasing
// cell index, then wave shuffles, then the waves in order from LDS: no atomics, no flags, no waits, and a trial's result does
// not depend on what else is in the launch.

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

// twin of fv_cu_pcg (ldc_fv_cu_pressure.hip), statement for statement; the preconditioner and the row are this unit's
__device__ __forceinline__ void sg_pcg(const SgCtx& s, const FvCuPcg& P, FvRed& red, double b00, SgPcgRun& st) {
  const FvCtx& x = s.x;
  const int nx = x.nx, n = x.n, tid = threadIdx.x;
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
    sg_fastdiag(x, x.vec(PCG_R), x.vec(PCG_Z));
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

template <bool CONSISTENT>
__global__ __launch_bounds__(kFvThreads) void fv_stretched_kernel(FvLaunch L) {
  __shared__ double lds[2][kFvWaves * kFvRed];
  // (the descriptor pointer from the kernarg segment: fv_kernel says why)
  typedef const FvDesc* FvDescPtr;
  const FvDesc& d = **(const __attribute__((address_space(4))) FvDescPtr*)((kernarg_ptr)__builtin_amdgcn_kernarg_segment_ptr() +
                                                                           __builtin_offsetof(FvLaunch, d) + blockIdx.x * sizeof(FvDescPtr));
  const FvCuPcg& P = *reinterpret_cast<const FvCuPcg*>(reinterpret_cast<const char*>(&d) + kFvCuPcgOffset);
  const FvGridBlk& G = *reinterpret_cast<const FvGridBlk*>(reinterpret_cast<const char*>(&d) + kFvGridOffset);
  const FvCtx x(d);
  const SgCtx s(x, G);
  FvRed red = {lds, 0};
  FvRun run = {d.ctrl[0], d.ctrl[1], 0, 0, 0, d.ctrl[2] != 0};
  SgPcgRun st = {0, 0, 0, 0};
  for (int k = 0; k < L.n_iters && !run.done && !run.nan_seen; ++k) {
    double b2[2];
    sg_assemble(s, red, b2);
    fv_bicgstab(x, red, b2, run);
    double b00;
    sg_faces<CONSISTENT>(s, red, b00);
    if (CONSISTENT) sg_pcg(s, P, red, b00, st);
    else sg_fastdiag(x, x.vec(FV_C), x.vec(FV_Y));
    double part[kFvRed] = {0.0};
    sg_correct(s, part);
    sg_fluxvort<CONSISTENT>(s, part);
    sg_record(s, red, part, k, run);
  }
  if (threadIdx.x == 0) {
    d.ctrl[0] = run.done; d.ctrl[1] = run.iter; d.ctrl[2] = run.nan_seen ? 1 : 0;
    d.ctrl[3] += run.giveups; d.ctrl[4] += run.lin_iters; d.ctrl[5] += run.solves;
    if (CONSISTENT) {
      P.stats[0] += st.iters; P.stats[1] += st.solves; P.stats[2] += st.caps;
      if (st.solves) P.stats[3] = st.last;
    }
  }
}

}  // namespace

int ldc_fv_stretched_launch(ldc_fv* const* hs, int n, int n_iters, int consistent, void* stream) {
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) return LDC_E_NODEVICE;
  const int mode = consistent ? LDC_FV_PRESSURE_CONSISTENT : LDC_FV_PRESSURE_REFERENCE;
  for (int lo = 0; lo < n; lo += LDC_FV_LAUNCH_MAX) {
    FvLaunch L;
    const int b = n - lo < LDC_FV_LAUNCH_MAX ? n - lo : LDC_FV_LAUNCH_MAX;
    for (int q = 0; q < b; ++q) {
      const ldc_fv* h = hs[lo + q];
      if (h->device != dev || h->grid_mode != LDC_FV_GRID_TABLES || h->pressure_mode != mode) return LDC_E_STATE;
      L.d[q] = h->dev;
    }
    for (int q = b; q < LDC_FV_LAUNCH_MAX; ++q) L.d[q] = nullptr;
    L.n_iters = n_iters;
    if (consistent) hipLaunchKernelGGL(fv_stretched_kernel<true>, dim3(b), dim3(kFvThreads), 0, as_stream(stream), L);
    else hipLaunchKernelGGL(fv_stretched_kernel<false>, dim3(b), dim3(kFvThreads), 0, as_stream(stream), L);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  return 0;
}
