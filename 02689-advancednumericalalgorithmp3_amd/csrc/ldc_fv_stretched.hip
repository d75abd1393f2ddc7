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
//   4. reference:  sg_fastdiag, the four fv_gemm of fv_fastdiag with ax = ay = 1 and the generalised eigenpairs
//      consistent: fv_pcg with SgPolicy: z = sg_fastdiag r, sg_row for A p                   (twin: wide_pcg_row)
//      (the loop, fv_fastdiag and the kernel frame are ldc_fv_cu_solve.inc, shared with ldc_fv_cu_pressure.hip)
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
#include "ldc_fv_cu_solve.inc"
#include "ldc_fv_stretched_phases.inc"

// what fv_pcg (ldc_fv_cu_solve.inc) takes from this unit: z = L+ r with the generalised eigenpairs (sg_fastdiag) and the
// row of A from the tables (sg_row)
struct SgPolicy {
  const SgCtx& s;
  __device__ __forceinline__ void start(int, double) const {}
  __device__ __forceinline__ void precondition() const { sg_fastdiag(s.x, s.x.vec(PCG_R), s.x.vec(PCG_Z)); }
  __device__ __forceinline__ const double* src() const { return s.x.vec(PCG_R); }
  __device__ __forceinline__ double z(int c) const { return s.x.vec(PCG_Z)[c]; }
  __device__ __forceinline__ double row(int c, int i, int j, double pc, const double* p) const {
    return sg_row(s, c, i, j, pc, p);
  }
  __device__ __forceinline__ void residual(int, double) const {}
};

template <bool CONSISTENT>
__global__ __launch_bounds__(kFvThreads) void fv_stretched_kernel(FvLaunch L) {
  __shared__ double lds[2][kFvWaves * kFvRed];
  const FvDesc& d = fv_block_desc();
  const FvCuPcg& P = fv_slot_block<FvCuPcg>(d, kFvCuPcgOffset);
  const FvCtx x(d);
  const SgCtx s(x, fv_slot_block<FvGridBlk>(d, kFvGridOffset));
  const SgPolicy pol = {s};
  FvRed red = {lds, 0};
  FvRun run = {d.ctrl[0], d.ctrl[1], 0, 0, 0, d.ctrl[2] != 0};
  FvPcgRun st = {0, 0, 0, 0};
  for (int k = 0; k < L.n_iters && !run.done && !run.nan_seen; ++k) {
    double b2[2];
    sg_assemble(s, red, b2);
    fv_bicgstab(x, red, b2, run);
    double b00;
    sg_faces<CONSISTENT>(s, red, b00);
    if (CONSISTENT) fv_pcg(x, pol, P, red, b00, st);
    else sg_fastdiag(x, x.vec(FV_C), x.vec(FV_Y));
    double part[kFvRed] = {0.0};
    sg_correct(s, part);
    sg_fluxvort<CONSISTENT>(s, part);
    sg_record(s, red, part, k, run);
  }
  if (threadIdx.x == 0) {
    fv_store_run(d, run);
    if (CONSISTENT) fv_store_stats(P, st);
  }
}

}  // namespace

int ldc_fv_stretched_launch(ldc_fv* const* hs, int n, int n_iters, int consistent, void* stream) {
  const int mode = consistent ? LDC_FV_PRESSURE_CONSISTENT : LDC_FV_PRESSURE_REFERENCE;
  return fv_launch_chunks(consistent ? fv_stretched_kernel<true> : fv_stretched_kernel<false>, hs, n, n_iters, stream,
                          [mode](const ldc_fv* h) {
                            return h->grid_mode == LDC_FV_GRID_TABLES && h->pressure_mode == mode;
                          });
}
