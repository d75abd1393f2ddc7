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
//   4. fv_pcg           conjugate gradients on A x = b from x = 0 with z = L+ r.  The loop, the four-GEMM solve
//                       (fv_fastdiag) and the kernel frame are ldc_fv_cu_solve.inc, shared with the stretched-grid
//                       kernels; this unit contributes FvCuPolicy: the Laplacian's eigenpairs with dy/dx, dx/dy and the
//                       row of A on the uniform grid (wide_pcg_row).
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
#include "ldc_fv_cu_solve.inc"

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

// ---- 4. what fv_pcg (ldc_fv_cu_solve.inc) takes from this unit: z = L+ r with the Laplacian's eigenpairs of the
//         descriptor, and the row of A on the uniform grid (wide_pcg_row, ldc_fv_pressure_cells.inc).  ax = dy / dx and
//         ay = dx / dy are formed once per solve, where the policy is made
struct FvCuPolicy {
  const FvCtx& x;
  const double ax, ay;
  __device__ __forceinline__ void start(int, double) const {}
  __device__ __forceinline__ void precondition() const {
    const FvDesc& d = x.d;
    fv_fastdiag(x, d.Qx, d.lamx, d.Qy, d.lamy, ax, ay, x.vec(PCG_R), x.vec(PCG_Z));
  }
  __device__ __forceinline__ const double* src() const { return x.vec(PCG_R); }
  __device__ __forceinline__ double z(int c) const { return x.vec(PCG_Z)[c]; }
  __device__ __forceinline__ double row(int c, int i, int j, double pc, const double* p) const {
    return wide_pcg_row(x, c, i, j, pc, [&](int k) { return p[k]; });
  }
  __device__ __forceinline__ void residual(int, double) const {}
};

// ---- 6. mdot = mdot* - w_f (p'_N - p'_P) on the inner faces, exactly 0.0 on the walls; the vorticity
__device__ __forceinline__ void fv_cu_fluxvort(const FvCtx& x, double (&part)[kFvRed]) {
  const int n = x.n, tid = threadIdx.x;
  const double *pp = x.vec(FV_Y), *sx = x.vec(PCG_MS), *sy = x.vec(PCG_MS) + x.ny * x.ldx;
  for (int c = tid; c < n; c += kFvThreads) wide_pcg_cell_fluxvort(x, c, pp, sx, sy, part[8]);
  __syncthreads();
}

__global__ __launch_bounds__(kFvThreads) void fv_cu_pressure_kernel(FvLaunch L) {
  __shared__ double lds[2][kFvWaves * kFvRed];
  const FvDesc& d = fv_block_desc();
  const FvCuPcg& P = fv_slot_block<FvCuPcg>(d, kFvCuPcgOffset);
  const FvCtx x(d);
  const FvDebug dbg = {};                    // (phases 5 and 7 are the production instantiations: they read nothing of it)
  FvRed red = {lds, 0};
  FvRun run = {d.ctrl[0], d.ctrl[1], 0, 0, 0, d.ctrl[2] != 0};
  FvPcgRun st = {0, 0, 0, 0};
  for (int k = 0; k < L.n_iters && !run.done && !run.nan_seen; ++k) {
    double b2[2];
    fv_assemble(x, red, b2);
    fv_bicgstab(x, red, b2, run);
    double b00;
    fv_cu_faces(x, red, b00);
    fv_pcg(x, FvCuPolicy{x, x.dy / x.dx, x.dx / x.dy}, P, red, b00, st);
    double part[kFvRed] = {0.0};           // the sums of the record row (fv_correct)
    fv_correct<false>(x, part, dbg);
    fv_cu_fluxvort(x, part);
    fv_record<false>(x, red, part, k, run, dbg);
  }
  if (threadIdx.x == 0) {
    fv_store_run(d, run);
    fv_store_stats(P, st);
  }
}

}  // namespace

int ldc_fv_cu_pressure_launch(ldc_fv* const* hs, int n, int n_iters, void* stream) {
  return fv_launch_chunks(fv_cu_pressure_kernel, hs, n, n_iters, stream,
                          [](const ldc_fv* h) { return h->pressure_mode == LDC_FV_PRESSURE_CONSISTENT; });
}
