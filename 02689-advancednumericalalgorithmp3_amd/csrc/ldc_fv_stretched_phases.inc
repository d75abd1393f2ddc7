// ldc_fv_stretched_phases.inc -- the phases of a SIMPLE iteration of a one-CU trial on a wall-clustered tensor grid that do
// not depend on how the pressure equation is preconditioned (include/ldc_fv.h, "Stretched grids of a one-CU trial"):
// sg_assemble, sg_faces, sg_fastdiag, sg_correct, sg_fluxvort and sg_record.  These are the mapping -- the cell loop of ONE
// work-group, its reductions and its barriers; the arithmetic of a cell (SgCtx, sg_grad, sg_cell_*, sg_wx, sg_wy, sg_row,
// sg_gauss) is ldc_fv_stretched_cells.inc, which the chip mapping (ldc_fv_wide.hip) includes too.
// Included INSIDE the anonymous namespace of its unit, behind ldc_fv_cu_phases.inc and ldc_fv_cu_solve.inc (fv_fastdiag,
// and fv_pcg, the CG loop that calls sg_row), by ldc_fv_stretched.hip (fv_stretched_kernel) and by
// ldc_fv_stretched_sep.hip (fv_stretched_sep_kernel, whose CG has another preconditioner).

#include "ldc_fv_stretched_cells.inc"

// ---- 1. twin of fv_assemble
__device__ __forceinline__ void sg_assemble(const SgCtx& s, FvRed& red, double (&b2)[2]) {
  const int n = s.x.n, tid = threadIdx.x;
  b2[0] = 0.0; b2[1] = 0.0;
  for (int c = tid; c < n; c += kFvThreads) sg_cell_assemble(s, c, b2);
  red.sum(b2);
}

// ---- 3. b00 = minus the sum of rhs_p: entry 0 of the pinned right-hand side
template <bool CONSISTENT>
__device__ __forceinline__ void sg_faces(const SgCtx& s, FvRed& red, double& b00) {
  const FvCtx& x = s.x;
  const int n = x.n, tid = threadIdx.x;
  double* fx = CONSISTENT ? x.vec(PCG_MS) : x.fx;
  double* fy = CONSISTENT ? x.vec(PCG_MS) + x.ny * x.ldx : x.fy;
  double csum[1] = {0.0};
  for (int c = tid; c < n; c += kFvThreads) {
    double rhs;
    sg_cell_faces(s, fx, fy, c, rhs);
    csum[0] += rhs;
  }
  red.sum(csum);
  b00 = -csum[0];
  if (!CONSISTENT) {
    if (tid == 0) x.vec(FV_C)[0] = b00;
    __syncthreads();
  }
}

// ---- 4. z = L+ r (or the exact solve of the reference mode): fv_fastdiag with ax = ay = 1 and the generalised eigenpairs
__device__ __forceinline__ void sg_fastdiag(const FvCtx& x, const double* rhs, double* out) {
  fv_fastdiag(x, x.d.Qx, x.d.lamx, x.d.Qy, x.d.lamy, 1.0, 1.0, rhs, out);
}

// ---- 5. twin of fv_correct<false>
__device__ __forceinline__ void sg_correct(const SgCtx& s, double (&part)[kFvRed]) {
  const FvCtx& x = s.x;
  const int n = x.n, tid = threadIdx.x;
  const double y0 = x.vec(FV_Y)[0];
  for (int c = tid; c < n; c += kFvThreads) sg_cell_correct(s, y0, c, part);
  __syncthreads();
}

// ---- 6. the corrected face fluxes of either mode, then omega = dv/dx - du/dy; part[8] += omega^2 V
template <bool CONSISTENT>
__device__ __forceinline__ void sg_fluxvort(const SgCtx& s, double (&part)[kFvRed]) {
  const int n = s.x.n, tid = threadIdx.x;
  for (int c = tid; c < n; c += kFvThreads) sg_cell_fluxvort<CONSISTENT>(s, c, part[8]);
  __syncthreads();
}

// ---- 7. twin of fv_record<false>: div mdot, |grad omega|^2 V; the sums of E, Z, P carry V already, so the row takes V = 1
__device__ __forceinline__ void sg_record(const SgCtx& s, FvRed& red, double (&part)[kFvRed], int k, FvRun& run) {
  const FvDesc& d = s.x.d;
  const int n = s.x.n, tid = threadIdx.x;
  for (int c = tid; c < n; c += kFvThreads) sg_cell_sums(s, c, part[7], part[9]);
  red.sum(part);
  const double rel = fv_rec_rel(part);
  if (tid == 0) fv_rec_row(d.rec + (long long)k * LDC_FV_REC_LEN, rel, part, 1.0);
  if (rel != rel) run.nan_seen = true;
  else if (run.iter >= d.warmup && rel < d.tol) run.done = 1;
  ++run.iter;
  __syncthreads();
}
