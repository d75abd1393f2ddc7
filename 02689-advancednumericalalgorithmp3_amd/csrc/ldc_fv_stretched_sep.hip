// ldc_fv_stretched_sep.hip -- the SIMPLE iteration of a one-CU trial on a wall-clustered tensor grid with the consistent
// pressure equation, its CG preconditioned by a separable, scaled operator (include/ldc_fv.h, "The separable scaled
// preconditioner"; ldc_fv_set_preconditioner).
//
// A translation unit of its own, as ldc_fv_stretched.hip is and for the same reason: a trial that does not ask for this
// preconditioner runs fv_stretched_kernel, whose code object stays what it was.  Every phase is that kernel's
// (ldc_fv_stretched_phases.inc, ldc_fv_cu_phases.inc); so are the CG loop and the kernel frame (fv_pcg,
// ldc_fv_cu_solve.inc), the mapping (ONE work-group of 512 threads per trial, cells tid, tid + 512, ...), the reductions,
// the record and the latch.  This unit contributes SepPolicy: the preconditioner below.
//
// The preconditioner.  That of fv_stretched_kernel models A, whose face weights carry D = V / a_P, by
// Hy (x) Kx + Ky (x) Hx: D left out.  On a stretched mesh D varies with V by a factor of 30 ... 250.  Here D is modelled by
// a product a_i b_j (fitted on the host to the D of pure diffusion, once per mesh), which keeps the operator separable,
//     L_s = My (x) Kx^a + Ky^b (x) Mx,   Kx^a: weights rho a_f / d,   Mx = diag(hx a)   (y likewise with b),
// so L_s+ is the four GEMMs of fv_fastdiag with the generalised eigenpairs of (Kx^a, Mx) and (Ky^b, My); what the product
// misses of the actual D is taken by a diagonal scaling (Concus and Golub): s_c = sqrt(a_i b_j / D_c) per solve, and
//     z = s . L_s+ (s . r).
// Per axis one device table [a (n) | lam (n) | Q (n x n, row-major, column k the k-th vector)]; the two pointers live at byte
// 344 of the descriptor slot (FvPrecondBlk).
//
// The loop takes three pointwise factors from the policy and no sweep or barrier more: s is written in the loop that sets
// r = b, s . r in the loops that write r, and s . z' is formed in the loop that reads z' = L_s+ (s . r).  s and s . r live
// in the work vectors 15 and 17 (FV_VU, FV_PHU), which BiCGSTAB leaves dead during the pressure solve.
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
#include "ldc_fv_cu_solve.inc"
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

// what fv_pcg (ldc_fv_cu_solve.inc) takes from this unit: z = s . L_s+ (s . r).  PCG_Z holds z' = L_s+ (s . r) by
// fv_fastdiag with the eigenpairs of the fitted operator; every reader of z' multiplies by s.  The row of A is sg_row.
struct SepPolicy {
  const SgCtx& s;
  const SepCtx& t;
  __device__ __forceinline__ void start(int c, double b) const {
    const FvCtx& x = s.x;
    const int i = c % x.nx, j = c / x.nx;
    const double sc = sg_sep_scale(s, t.ax, t.ay, c, i, j);
    x.vec(SEP_S)[c] = sc;
    x.vec(SEP_SR)[c] = sc * b;
  }
  __device__ __forceinline__ void precondition() const {
    fv_fastdiag(s.x, t.Qx, t.lamx, t.Qy, t.lamy, 1.0, 1.0, s.x.vec(SEP_SR), s.x.vec(PCG_Z));
  }
  __device__ __forceinline__ const double* src() const { return s.x.vec(SEP_SR); }
  __device__ __forceinline__ double z(int c) const { return s.x.vec(SEP_S)[c] * s.x.vec(PCG_Z)[c]; }
  __device__ __forceinline__ double row(int c, int i, int j, double pc, const double* p) const {
    return sg_row(s, c, i, j, pc, p);
  }
  __device__ __forceinline__ void residual(int c, double rn) const { s.x.vec(SEP_SR)[c] = s.x.vec(SEP_S)[c] * rn; }
};

__global__ __launch_bounds__(kFvThreads) void fv_stretched_sep_kernel(FvLaunch L) {
  __shared__ double lds[2][kFvWaves * kFvRed];
  const FvDesc& d = fv_block_desc();
  const FvCuPcg& P = fv_slot_block<FvCuPcg>(d, kFvCuPcgOffset);
  const FvCtx x(d);
  const SgCtx s(x, fv_slot_block<FvGridBlk>(d, kFvGridOffset));
  const SepCtx t(x, fv_slot_block<FvPrecondBlk>(d, kFvPrecondOffset));
  const SepPolicy pol = {s, t};
  FvRed red = {lds, 0};
  FvRun run = {d.ctrl[0], d.ctrl[1], 0, 0, 0, d.ctrl[2] != 0};
  FvPcgRun st = {0, 0, 0, 0};
  for (int k = 0; k < L.n_iters && !run.done && !run.nan_seen; ++k) {
    double b2[2];
    sg_assemble(s, red, b2);
    fv_bicgstab(x, red, b2, run);
    double b00;
    sg_faces<true>(s, red, b00);
    fv_pcg(x, pol, P, red, b00, st);
    double part[kFvRed] = {0.0};
    sg_correct(s, part);
    sg_fluxvort<true>(s, part);
    sg_record(s, red, part, k, run);
  }
  if (threadIdx.x == 0) {
    fv_store_run(d, run);
    fv_store_stats(P, st);
  }
}

}  // namespace

int ldc_fv_stretched_sep_launch(ldc_fv* const* hs, int n, int n_iters, void* stream) {
  return fv_launch_chunks(fv_stretched_sep_kernel, hs, n, n_iters, stream, [](const ldc_fv* h) {
    return h->grid_mode == LDC_FV_GRID_TABLES && h->pressure_mode == LDC_FV_PRESSURE_CONSISTENT &&
           h->precond_mode == LDC_FV_PRECOND_SEPARABLE;
  });
}
