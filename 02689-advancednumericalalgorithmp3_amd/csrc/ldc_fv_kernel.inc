// ldc_fv_kernel.inc -- the finite-volume SIMPLE solver (include/ldc_fv.h), included at the end of ldc_kernels.hip.
//
// Mapping: ONE work-group of 512 threads (8 waves, two per SIMD) advances ONE trial for a whole chunk of iterations.
// A SIMPLE iteration is a sequence of cell sweeps (each thread takes cells tid, tid + 512, ...) separated by
// __syncthreads(); every scalar the iteration needs (BiCGSTAB dots, norms, the latch, E / Z / P) is a work-group
// reduction through LDS.  No work-group ever waits for another, so a batch launch is B independent work-groups:
// no flags, no spin limits, no co-residency.  512 threads rather than 1024: the iteration's live state takes ~175
// VGPRs, which two waves per SIMD allow; with four (1024 threads, 128 VGPRs) the kernel spilled ~400 registers to
// scratch.  The state of an N = 128 trial (32 vectors of 128 KB) stays L2-resident.
//
// The arithmetic of a cell, of a BiCGSTAB scalar step, of the record row and of a GEMM tile is in ldc_fv_cells.inc
// (fv_cell_*, fv_kry_*, fv_rec_*, fv_gemm_tile), shared with the chip mappings of ldc_fv_wide.hip.  What is here is this
// mapping: the loop over tid with stride 512, the barriers, the reductions (FvRed), the control words (FvRun), the debug
// copies and the host entry points.
//
// Structure: fv_kernel fetches the trial's descriptor, sets up the context the phases share (FvCtx) and calls, once
// per iteration and in this order,
//   1. fv_assemble             grad p, the five diagonals, the relaxed right-hand sides, the BiCGSTAB start
//   2. fv_bicgstab             the joint u / v BiCGSTAB, each update written once for component q = 0, 1
//   3. fv_face_fluxes          Rhie-Chow face fluxes mdot* and rhs_p
//   4. fv_pressure_correction  the four fv_gemm calls of the fast diagonalisation
//   5. fv_correct              u, v and p updated by u', v', p'
//   6. fv_flux_vorticity       mdot updated; the vorticity
//   7. fv_record               divergence, palinstrophy, the record row and the latch
// then writes the control words back.  Every phase ends on the barrier the next one needs.  The kernel is a template:
// fv_kernel<false> is the production kernel; fv_kernel<true>, launched by ldc_fv_step_debug alone, also copies out the
// intermediates FvDebug selects (if constexpr (DEBUG) in phases 3, 5 and 7).  Same arithmetic in both.
//
// Momentum: u and v share one matrix (the assembly depends on mdot and mu only), kept as five diagonals with aP
// unrelaxed; the relaxed diagonal is aP / alpha_uv.  Both systems run through ONE BiCGSTAB loop (Jacobi
// preconditioner, SciPy's iteration and stopping rule per component), so each iteration's reductions serve both.
// Pressure correction: the pinned Neumann Laplacian is solved exactly by fast diagonalisation, four GEMMs on fp64 MFMA
// (v_mfma_f64_16x16x4_f64) with the eigenvectors the host computed once.

// (kFvThreads, kFvWaves, FvVec, FvDesc, fv_desc_of and struct ldc_fv: ldc_fv_common.inc, shared with the other FV
// units; FvCtx, FvKrylov, fv_cell_*, fv_kry_*, fv_rec_* and fv_gemm_tile: ldc_fv_cells.inc, shared with ldc_fv_wide.hip;
// FvLaunch, fv_reduce, fv_gemm, FvRed, FvRun and the seven phases: ldc_fv_cu_phases.inc, included below, shared with
// ldc_fv_cu_pressure.hip -- the kernel of a handle in mode LDC_FV_PRESSURE_CONSISTENT, a unit of its own -- and with
// ldc_fv_stretched.hip, the kernel of a handle with geometry tables, ldc_fv_set_grid, and ldc_fv_stretched_sep.hip, the
// kernel of such a handle with the separable preconditioner, ldc_fv_set_preconditioner)

namespace {

#include "ldc_fv_cu_phases.inc"

// DEBUG = false: the production kernel, which reads nothing of dbg; DEBUG = true: ldc_fv_step_debug's, which also
// copies out the intermediates dbg selects
template <bool DEBUG>
__global__ __launch_bounds__(kFvThreads) void fv_kernel(FvLaunch L, FvDebug dbg) {
  __shared__ double lds[2][kFvWaves * kFvRed];
  // the descriptor pointer is read straight from the kernarg segment: indexing the by-value array with blockIdx.x
  // would make the compiler materialise all LDC_FV_LAUNCH_MAX pointers in registers
  typedef const FvDesc* FvDescPtr;
  const FvDesc& d = **(const __attribute__((address_space(4))) FvDescPtr*)((kernarg_ptr)__builtin_amdgcn_kernarg_segment_ptr() +
                                                                           __builtin_offsetof(FvLaunch, d) + blockIdx.x * sizeof(FvDescPtr));
  const FvCtx x(d);
  FvRed red = {lds, 0};
  FvRun run = {d.ctrl[0], d.ctrl[1], 0, 0, 0, d.ctrl[2] != 0};
  for (int k = 0; k < L.n_iters && !run.done && !run.nan_seen; ++k) {
    double b2[2];
    fv_assemble(x, red, b2);
    fv_bicgstab(x, red, b2, run);
    fv_face_fluxes<DEBUG>(x, red, dbg);
    fv_pressure_correction(x);
    double part[kFvRed] = {0.0};           // the sums of the record row (fv_correct)
    fv_correct<DEBUG>(x, part, dbg);
    fv_flux_vorticity(x, part);
    fv_record<DEBUG>(x, red, part, k, run, dbg);
  }
  if (threadIdx.x == 0) {
    d.ctrl[0] = run.done; d.ctrl[1] = run.iter; d.ctrl[2] = run.nan_seen ? 1 : 0;
    d.ctrl[3] += run.giveups; d.ctrl[4] += run.lin_iters; d.ctrl[5] += run.solves;
  }
}

// Explicit instantiations: the two kernels are emitted here, ahead of the spectral kernels' (implicit) template
// instantiations, where the kernel stood before it became a template.  Left implicit they are emitted last and every
// spectral kernel moves in the code object; with that placement tests/test_gpu_wide.py::
// test_wide_two_identical_runs_agree_bit_for_bit (tail layout) failed in 5 of 6 runs, with this one and with the
// non-template kernel in 0 of 6 (profiles/fv_perf.md).  The chip-wide kernel's instructions are the same in all three.
template __global__ void fv_kernel<false>(FvLaunch, FvDebug);
template __global__ void fv_kernel<true>(FvLaunch, FvDebug);

}  // namespace

namespace {

// debug: the instantiation that copies out what dbg selects (ldc_fv_step_debug); production launches ignore dbg
int fv_launch(ldc_fv* const* hs, int n, int n_iters, bool debug, const FvDebug& dbg, void* stream) {
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) return LDC_E_NODEVICE;
  for (int lo = 0; lo < n; lo += LDC_FV_LAUNCH_MAX) {
    FvLaunch L;
    const int b = n - lo < LDC_FV_LAUNCH_MAX ? n - lo : LDC_FV_LAUNCH_MAX;
    for (int q = 0; q < b; ++q) {
      if (hs[lo + q]->device != dev) return LDC_E_STATE;
      L.d[q] = hs[lo + q]->dev;
    }
    for (int q = b; q < LDC_FV_LAUNCH_MAX; ++q) L.d[q] = nullptr;
    L.n_iters = n_iters;
    hipLaunchKernelGGL(debug ? fv_kernel<true> : fv_kernel<false>, dim3(b), dim3(kFvThreads), 0, as_stream(stream), L, dbg);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  return 0;
}

// n_iters iterations of every handle, each by the kernel of its mode: the reference handles through fv_launch exactly as
// before, in list order; the consistent ones (ldc_fv_set_pressure) through the launch function of ldc_fv_cu_pressure.hip,
// in list order too; the handles with geometry tables (ldc_fv_set_grid) through that of ldc_fv_stretched.hip, one group per
// pressure mode; of these the consistent ones with the separable preconditioner (ldc_fv_set_preconditioner) through that of
// ldc_fv_stretched_sep.hip.  A mixed list is up to five launch groups; nothing waits for anything, so the order does not
// matter.
int fv_dispatch(ldc_fv* const* hs, int n, int n_iters, void* stream) {
  int count[5] = {0, 0, 0, 0, 0};
  const auto group = [](const ldc_fv* h) {
    const int g = (h->grid_mode == LDC_FV_GRID_TABLES ? 2 : 0) + (h->pressure_mode == LDC_FV_PRESSURE_CONSISTENT ? 1 : 0);
    return g == 3 && h->precond_mode == LDC_FV_PRECOND_SEPARABLE ? 4 : g;
  };
  for (int q = 0; q < n; ++q) ++count[group(hs[q])];
  const auto launch = [&](int g, ldc_fv* const* list, int m) {
    if (g == 0) return fv_launch(list, m, n_iters, false, FvDebug{}, stream);
    if (g == 1) return ldc_fv_cu_pressure_launch(list, m, n_iters, stream);
    if (g == 4) return ldc_fv_stretched_sep_launch(list, m, n_iters, stream);
    return ldc_fv_stretched_launch(list, m, n_iters, g == 3, stream);
  };
  for (int g = 0; g < 5; ++g) if (count[g] == n) return launch(g, hs, n);
  for (int g = 0; g < 5; ++g) {
    if (count[g] == 0) continue;
    std::vector<ldc_fv*> part;
    for (int q = 0; q < n; ++q) if (group(hs[q]) == g) part.push_back(hs[q]);
    const int rc = launch(g, part.data(), (int)part.size());
    if (rc != 0) return rc;
  }
  return 0;
}

}  // namespace

extern "C" {

int ldc_fv_version(void) { return LDC_FV_VERSION; }

int ldc_fv_create(const struct ldc_fv_problem* pr, ldc_fv** out) {
  if (!pr || !out) return LDC_E_ARG;
  *out = nullptr;
  FvDesc h;
  const int rc = fv_desc_of(pr, LDC_FV_MAX_N, &h);
  if (rc != 0) return rc;
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) return LDC_E_NODEVICE;
  FvDesc* slot = reinterpret_cast<FvDesc*>(pr->work + (int64_t)LDC_FV_NWORK * pr->nx * pr->ny);
  const hipError_t e = copy_now(slot, &h, sizeof(h), hipMemcpyHostToDevice);
  if (e != hipSuccess) return (int)e;
  ldc_fv* s = new (std::nothrow) ldc_fv;
  if (!s) return LDC_E_STATE;
  s->dev = slot; s->ctrl = h.ctrl; s->rec_cap = pr->rec_cap; s->device = dev;
  s->nx = pr->nx; s->ny = pr->ny; s->dx = pr->dx; s->dy = pr->dy;
  s->pressure_mode = LDC_FV_PRESSURE_REFERENCE;
  s->grid_mode = LDC_FV_GRID_UNIFORM;
  s->precond_mode = LDC_FV_PRECOND_LAPLACIAN;
  *out = s;
  return 0;
}

int ldc_fv_destroy(ldc_fv* h) {
  if (!h) return LDC_E_STATE;
  delete h;
  return 0;
}

int ldc_fv_enqueue(ldc_fv* h, int n_iters, void* stream) {
  if (!h) return LDC_E_STATE;
  if (n_iters < 1 || n_iters > h->rec_cap) return LDC_E_ARG;
  return fv_dispatch(&h, 1, n_iters, stream);
}

int ldc_fv_batch_enqueue(ldc_fv* const* hs, int n, int n_iters, void* stream) {
  if (!hs || n < 1 || n_iters < 1) return LDC_E_ARG;
  for (int q = 0; q < n; ++q) {
    if (!hs[q]) return LDC_E_STATE;
    if (n_iters > hs[q]->rec_cap) return LDC_E_ARG;
  }
  return fv_dispatch(hs, n, n_iters, stream);
}

int ldc_fv_set_pressure(ldc_fv* h, const struct ldc_fv_pressure* cfg, int64_t* stats, int64_t stats_len) {
  if (!h) return LDC_E_STATE;
  if (!cfg || cfg->mode == LDC_FV_PRESSURE_REFERENCE) {
    h->pressure_mode = LDC_FV_PRESSURE_REFERENCE;
    return 0;
  }
  if (cfg->mode != LDC_FV_PRESSURE_CONSISTENT || cfg->max_iters < 1 || !(cfg->tol > 0.0 && cfg->tol < 1.0)) return LDC_E_ARG;
  if (!stats || stats_len < LDC_FV_PRESSURE_STATS_LEN) return LDC_E_ARG;
  const FvCuPcg blk = {cfg->tol, cfg->max_iters, cfg->mode, reinterpret_cast<long long*>(stats)};
  const hipError_t e = copy_now(reinterpret_cast<char*>(h->dev) + kFvCuPcgOffset, &blk, sizeof(blk), hipMemcpyHostToDevice);
  if (e != hipSuccess) return (int)e;
  h->pressure_mode = LDC_FV_PRESSURE_CONSISTENT;
  return 0;
}

int ldc_fv_set_grid(ldc_fv* h, const struct ldc_fv_grid* grid) {
  if (!h) return LDC_E_STATE;
  if (!grid || grid->mode == LDC_FV_GRID_UNIFORM) {
    h->grid_mode = LDC_FV_GRID_UNIFORM;             // (precond_mode is not read without tables: fv_dispatch)
    return 0;
  }
  if (grid->mode != LDC_FV_GRID_TABLES || !grid->x_tables || !grid->y_tables) return LDC_E_ARG;
  if (grid->x_len < LDC_FV_GRID_TABLE_LEN(h->nx) || grid->y_len < LDC_FV_GRID_TABLE_LEN(h->ny)) return LDC_E_ARG;
  const FvGridBlk blk = {grid->x_tables, grid->y_tables};
  const hipError_t e = copy_now(reinterpret_cast<char*>(h->dev) + kFvGridOffset, &blk, sizeof(blk), hipMemcpyHostToDevice);
  if (e != hipSuccess) return (int)e;
  h->grid_mode = LDC_FV_GRID_TABLES;
  h->precond_mode = LDC_FV_PRECOND_LAPLACIAN;       // (preconditioner tables belong to the mesh they were fitted to)
  return 0;
}

int ldc_fv_set_preconditioner(ldc_fv* h, const struct ldc_fv_precond* cfg) {
  if (!h) return LDC_E_STATE;
  if (!cfg || cfg->mode == LDC_FV_PRECOND_LAPLACIAN) {
    h->precond_mode = LDC_FV_PRECOND_LAPLACIAN;
    return 0;
  }
  if (cfg->mode != LDC_FV_PRECOND_SEPARABLE || h->grid_mode != LDC_FV_GRID_TABLES) return LDC_E_ARG;
  if (!cfg->x_table || !cfg->y_table) return LDC_E_ARG;
  if (cfg->x_len < LDC_FV_PRECOND_TABLE_LEN(h->nx) || cfg->y_len < LDC_FV_PRECOND_TABLE_LEN(h->ny)) return LDC_E_ARG;
  const FvPrecondBlk blk = {cfg->x_table, cfg->y_table};
  const hipError_t e = copy_now(reinterpret_cast<char*>(h->dev) + kFvPrecondOffset, &blk, sizeof(blk), hipMemcpyHostToDevice);
  if (e != hipSuccess) return (int)e;
  h->precond_mode = LDC_FV_PRECOND_SEPARABLE;
  return 0;
}

int ldc_fv_status(ldc_fv* h) {
  if (!h) return LDC_E_STATE;
  long long flag = 0;
  const hipError_t e = copy_now(&flag, h->ctrl + 2, sizeof(flag), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return (int)e;
  return flag ? LDC_FV_E_NAN : 0;
}

int ldc_fv_step_debug(ldc_fv* h, int which, double* const* out, void* stream) {
  if (!h) return LDC_E_STATE;
  if (which < 0 || which >= (1 << LDC_FV_DBG_COUNT) || (which && !out)) return LDC_E_ARG;
  if (h->pressure_mode != LDC_FV_PRESSURE_REFERENCE) return LDC_E_ARG;      // (the debug kernel is the reference iteration)
  if (h->grid_mode != LDC_FV_GRID_UNIFORM) return LDC_E_ARG;                // (... on the uniform grid)
  FvDebug dbg = {};
  for (int k = 0; k < LDC_FV_DBG_COUNT; ++k) {
    if (!(which & (1 << k))) continue;
    if (!out[k]) return LDC_E_ARG;
    dbg.out[k] = out[k];
  }
  return fv_launch(&h, 1, 1, true, dbg, stream);
}

}  // extern "C"
