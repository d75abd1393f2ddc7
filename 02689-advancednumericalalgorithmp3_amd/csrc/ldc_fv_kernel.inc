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
// units; FvCtx, FvKrylov, fv_cell_*, fv_kry_*, fv_rec_* and fv_gemm_tile: ldc_fv_cells.inc, shared with ldc_fv_wide.hip)

namespace {

constexpr int kFvRed = 10;                  // most values one reduction carries

struct FvLaunch {
  const FvDesc* d[LDC_FV_LAUNCH_MAX];
  int n_iters;
};

struct FvDebug {
  double* out[LDC_FV_DBG_COUNT];
};

// sums of K values over the work-group; every thread gets the same totals (fixed order: bit-reproducible).
// (wide_block_sum of ldc_fv_wide.hip is the same sum for 4 waves with a trailing barrier and an unrolled last loop;
// the two are kept apart so that neither kernel's code depends on a parameter meant for the other.)
template <int K>
__device__ inline void fv_reduce(double (&a)[K], double* lds) {
  static_assert(K <= kFvRed, "reduction slot");
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) a[k] += __shfl_xor(a[k], off);
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) lds[w * kFvRed + k] = a[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double s = 0.0;
#pragma unroll 1
    for (int q = 0; q < kFvWaves; ++q) s += lds[q * kFvRed + k];
    a[k] = s;
  }
}

// C[r][c] = sum_k A(r, k) B(k, c) (M x N, row-major), A(r, k) = A[r*sar + k*sak], B(k, c) = B[k*sbk + c*sbc].
// One wave per 16 x 16 output tile (fv_gemm_tile; waves take tiles round-robin); SCALE: the fast-diagonalisation
// epilogue.
template <bool SCALE>
__device__ void fv_gemm(const double* A, int sar, int sak, const double* B, int sbk, int sbc, double* Cm, int M,
                        int N, int K, const double* lamx, const double* lamy, double ax, double ay) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int tn = (N + 15) >> 4, tiles = ((M + 15) >> 4) * tn;
  for (int t = w; t < tiles; t += kFvWaves) {
    const int r0 = (t / tn) * 16, c0 = (t % tn) * 16;
    fv_gemm_tile<SCALE, false>(A, sar, sak, B, sbk, sbc, Cm, M, N, K, r0, c0, lane, lamx, lamy, ax, ay, 0.0);
  }
}

static_assert(FV_AN == FV_AP + 4, "the five diagonals are adjacent (LDC_FV_DBG_DIAG)");

// the two LDS buffers the work-group reductions alternate between
struct FvRed {
  double (*lds)[kFvWaves * kFvRed];
  int rb;
  template <int K>
  __device__ __forceinline__ void sum(double (&a)[K]) { fv_reduce(a, lds[rb]); rb ^= 1; }
};

// the trial's control words while a launch runs (ctrl[0 .. 5] of ldc_fv.h; the three counters are this launch's
// increments)
struct FvRun {
  long long done, iter, giveups, lin_iters, solves;
  bool nan_seen;
};

// ---- 1. grad p, the momentum matrix (five diagonals), relaxed right-hand sides, BiCGSTAB start: b2 = |b_u|^2, |b_v|^2
__device__ __forceinline__ void fv_assemble(const FvCtx& x, FvRed& red, double (&b2)[2]) {
  const int n = x.n, tid = threadIdx.x;
  b2[0] = 0.0; b2[1] = 0.0;
  for (int c = tid; c < n; c += kFvThreads) fv_cell_assemble(x, c, b2);
  red.sum(b2);
}

// ---- 2. BiCGSTAB for u (q = 0) and v (q = 1) together (SciPy's loop: rtol * |b|, x0 = 0, non-convergence accepted);
//         the sums of both components share each reduction: s2[q], s3[3q .. 3q+2], s4[2q .. 2q+1]
__device__ __forceinline__ void fv_bicgstab(const FvCtx& x, FvRed& red, const double (&b2)[2], FvRun& run) {
  const FvDesc& d = x.d;
  const int nx = x.nx, n = x.n, tid = threadIdx.x;
  double* const w = x.w;
  const double inv_a = x.inv_a;
  FvKrylov s[2];
  for (int q = 0; q < 2; ++q) fv_kry_start(s[q], b2[q], d.lin_tol);
  for (int it = 0; it < d.maxit; ++it) {
    for (int q = 0; q < 2; ++q) fv_kry_head(s[q], it);
    if (!s[0].act && !s[1].act) break;
    for (int c = tid; c < n; c += kFvThreads) {
      const double dg = w[FV_AP * n + c] * inv_a;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        if (!s[q].act) continue;
        fv_cell_p(x, c, q, it, s[q], dg);
      }
    }
    __syncthreads();
    double s2[2] = {0, 0};
    for (int c = tid; c < n; c += kFvThreads) {
      const int i = c % nx, j = c / nx;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        if (!s[q].act) continue;
        fv_cell_v(x, c, i, j, q, s2[q]);
      }
    }
    red.sum(s2);
    for (int q = 0; q < 2; ++q) fv_kry_alpha(s[q], s2[q]);
    for (int c = tid; c < n; c += kFvThreads) {
      const double dg = w[FV_AP * n + c] * inv_a;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        if (!s[q].act || s[q].brk) continue;
        fv_cell_s(x, c, q, s[q], dg);
      }
    }
    __syncthreads();
    double s3[6] = {0, 0, 0, 0, 0, 0};
    for (int c = tid; c < n; c += kFvThreads) {
      const int i = c % nx, j = c / nx;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        if (!s[q].act || s[q].brk) continue;
        fv_cell_t(x, c, i, j, q, s3 + 3 * q);
      }
    }
    red.sum(s3);
    for (int q = 0; q < 2; ++q) fv_kry_omega(s[q], s3[3 * q], s3[3 * q + 1], s3[3 * q + 2], it);
    double s4[4] = {0, 0, 0, 0};
    for (int c = tid; c < n; c += kFvThreads) {
#pragma unroll
      for (int q = 0; q < 2; ++q) {             // (not a function of ldc_fv_cells.inc, which says why; wide_bicg_x of
        if (!s[q].act) continue;                // ldc_fv_wide.hip holds a copy: a change to one goes into the other)
        double *xs = x.vec(FV_XU, q), *ph = x.vec(FV_PHU, q);
        if (s[q].fin) xs[c] += s[q].alpha * ph[c];
        else {
          double *rs = x.vec(FV_RU, q);
          double xn = xs[c]; xn += s[q].alpha * ph[c]; xn += s[q].omega * x.vec(FV_SHU, q)[c]; xs[c] = xn;
          const double r = rs[c] - s[q].omega * x.vec(FV_TU, q)[c];
          rs[c] = r; s4[2 * q] += r * r; s4[2 * q + 1] += x.vec(FV_RTU, q)[c] * r;
        }
      }
    }
    red.sum(s4);
    for (int q = 0; q < 2; ++q) fv_kry_after_x(s[q], s4[2 * q], s4[2 * q + 1], it + 1);
  }
  for (int q = 0; q < 2; ++q) {
    if (s[q].act) ++run.giveups;             // still active after max_lin_iters: accepted (scipy_solver.py:45-49)
    run.lin_iters += s[q].its;
  }
  run.solves += 2;
  __syncthreads();
}

// ---- 3. Rhie-Chow face velocities, mdot*, rhs_p = -div mdot* (rhs_p[0] = 0), its cell-0 entry for the pinned solve
template <bool DEBUG>
__device__ __forceinline__ void fv_face_fluxes(const FvCtx& x, FvRed& red, const FvDebug& dbg) {
  const FvDesc& d = x.d;
  const int nx = x.nx, ny = x.ny, n = x.n, ldx = x.ldx, tid = threadIdx.x;
  double* const w = x.w;
  double csum[1] = {0.0};
  for (int c = tid; c < n; c += kFvThreads) {
    double rhs;
    fv_cell_faces(x, c, rhs);
    csum[0] += rhs;
    if constexpr (DEBUG) {
      if (dbg.out[LDC_FV_DBG_RHS_P]) dbg.out[LDC_FV_DBG_RHS_P][c] = rhs;
    }
  }
  red.sum(csum);
  if (tid == 0) x.vec(FV_C)[0] = -csum[0];
  if constexpr (DEBUG) {
    if (dbg.out[LDC_FV_DBG_MDOT_STAR] || dbg.out[LDC_FV_DBG_GRAD_P] || dbg.out[LDC_FV_DBG_DIAG] ||
        dbg.out[LDC_FV_DBG_B] || dbg.out[LDC_FV_DBG_USTAR] || dbg.out[LDC_FV_DBG_VSTAR]) {
      for (int c = tid; c < n; c += kFvThreads) {
        if (dbg.out[LDC_FV_DBG_GRAD_P]) { dbg.out[LDC_FV_DBG_GRAD_P][c] = x.vec(FV_GPX)[c]; dbg.out[LDC_FV_DBG_GRAD_P][n + c] = x.vec(FV_GPY)[c]; }
        if (dbg.out[LDC_FV_DBG_DIAG]) for (int q = 0; q < 5; ++q) dbg.out[LDC_FV_DBG_DIAG][q * n + c] = w[(FV_AP + q) * n + c];
        if (dbg.out[LDC_FV_DBG_B]) { dbg.out[LDC_FV_DBG_B][c] = w[FV_BU * n + c]; dbg.out[LDC_FV_DBG_B][n + c] = w[FV_BV * n + c]; }
        if (dbg.out[LDC_FV_DBG_USTAR]) dbg.out[LDC_FV_DBG_USTAR][c] = x.vec(FV_XU)[c];
        if (dbg.out[LDC_FV_DBG_VSTAR]) dbg.out[LDC_FV_DBG_VSTAR][c] = x.vec(FV_XV)[c];
      }
      __syncthreads();                      // (the face writes above are visible to the copy)
      if (dbg.out[LDC_FV_DBG_MDOT_STAR]) {
        const int nf = ny * ldx + (ny + 1) * nx;
        for (int f = tid; f < nf; f += kFvThreads) dbg.out[LDC_FV_DBG_MDOT_STAR][f] = d.mdot[f];
      }
    }
  }
  __syncthreads();
}

// ---- 4. pressure correction by fast diagonalisation: Y = Qy (Qy^T C Qx / Lambda) Qx^T (p' is Y minus its cell-0 value)
__device__ __forceinline__ void fv_pressure_correction(const FvCtx& x) {
  const FvDesc& d = x.d;
  const int nx = x.nx, ny = x.ny;
  const double ax = x.dy / x.dx, ay = x.dx / x.dy;
  fv_gemm<false>(d.Qy, 1, ny, x.vec(FV_C), nx, 1, x.vec(FV_W1), ny, nx, ny, nullptr, nullptr, 0, 0);     // W1 = Qy^T C
  __syncthreads();
  fv_gemm<true>(x.vec(FV_W1), nx, 1, d.Qx, nx, 1, x.vec(FV_W2), ny, nx, nx, d.lamx, d.lamy, ax, ay);     // W2 = W1 Qx / Lambda
  __syncthreads();
  fv_gemm<false>(d.Qy, ny, 1, x.vec(FV_W2), nx, 1, x.vec(FV_W1), ny, nx, ny, nullptr, nullptr, 0, 0);    // W1 = Qy W2
  __syncthreads();
  fv_gemm<false>(x.vec(FV_W1), nx, 1, d.Qx, 1, nx, x.vec(FV_Y), ny, nx, nx, nullptr, nullptr, 0, 0);     // Y = W1 Qx^T
  __syncthreads();
}

// ---- 5. u' = -D grad p', u = u* + u', p += alpha_p p' (grad of y - y_0 is grad y) ---------------------------------
//         The cell body is NOT a function of ldc_fv_cells.inc: with any function around it fv_kernel<true> changes
//         (profiles/fv_wide.md).  wide_correct in ldc_fv_wide.hip holds a copy: a change to one goes into the other.
//         part: this thread's sums for the record row, filled by phases 5 - 7 and reduced once in phase 7:
//         du^2, u_old^2, dv^2, v_old^2, u'^2, v'^2, u^2+v^2, div^2, w^2, |grad w|^2
template <bool DEBUG>
__device__ __forceinline__ void fv_correct(const FvCtx& x, double (&part)[kFvRed], const FvDebug& dbg) {
  const FvDesc& d = x.d;
  const int nx = x.nx, ny = x.ny, n = x.n, tid = threadIdx.x;
  const double y0 = x.vec(FV_Y)[0];
  for (int c = tid; c < n; c += kFvThreads) {
    const int i = c % nx, j = c / nx;
    double gx, gy;
    fv_grad(x.vec(FV_Y), c, i, j, nx, ny, x.dx, x.dy, gx, gy);
    const double D = x.V / (x.w[FV_AP * n + c] + 1e-14);
    const double upc = -D * gx, vpc = -D * gy;
    const double un = x.vec(FV_XU)[c] + upc, vn = x.vec(FV_XV)[c] + vpc, uo = d.u[c], vo = d.v[c];
    const double pp = x.vec(FV_Y)[c] - y0;
    d.p[c] += d.alpha_p * pp;
    d.u[c] = un; d.v[c] = vn; x.vec(FV_UP)[c] = upc; x.vec(FV_VP)[c] = vpc;
    part[0] += (un - uo) * (un - uo); part[1] += uo * uo;
    part[2] += (vn - vo) * (vn - vo); part[3] += vo * vo;
    part[4] += upc * upc; part[5] += vpc * vpc; part[6] += un * un + vn * vn;
    if constexpr (DEBUG) {
      if (dbg.out[LDC_FV_DBG_P_PRIME]) dbg.out[LDC_FV_DBG_P_PRIME][c] = pp;
      if (dbg.out[LDC_FV_DBG_U_PRIME]) dbg.out[LDC_FV_DBG_U_PRIME][c] = upc;
      if (dbg.out[LDC_FV_DBG_V_PRIME]) dbg.out[LDC_FV_DBG_V_PRIME][c] = vpc;
    }
  }
  __syncthreads();
}

// ---- 6. mdot += rho interp(u', v') . S (walls: rho u'_P |S|, FV-Q4); vorticity with ghost cells -------------------
__device__ __forceinline__ void fv_flux_vorticity(const FvCtx& x, double (&part)[kFvRed]) {
  const int n = x.n, tid = threadIdx.x;
  for (int c = tid; c < n; c += kFvThreads) fv_cell_flux_vorticity(x, c, part[8]);
  __syncthreads();
}

// ---- 7. |div mdot|, palinstrophy, record row k of this launch and the latch ---------------------------------------
template <bool DEBUG>
__device__ __forceinline__ void fv_record(const FvCtx& x, FvRed& red, double (&part)[kFvRed], int k, FvRun& run,
                                          const FvDebug& dbg) {
  const FvDesc& d = x.d;
  const int n = x.n, tid = threadIdx.x;
  for (int c = tid; c < n; c += kFvThreads) fv_cell_div_palinstrophy(x, c, part[7], part[9]);
  red.sum(part);
  if constexpr (DEBUG) {
    if (dbg.out[LDC_FV_DBG_MDOT]) {
      const int nf = x.ny * x.ldx + (x.ny + 1) * x.nx;
      for (int f = tid; f < nf; f += kFvThreads) dbg.out[LDC_FV_DBG_MDOT][f] = d.mdot[f];
    }
  }
  const double rel = fv_rec_rel(part);
  if (tid == 0) fv_rec_row(d.rec + (long long)k * LDC_FV_REC_LEN, rel, part, x.V);
  if (rel != rel) run.nan_seen = true;
  else if (run.iter >= d.warmup && rel < d.tol) run.done = 1;
  ++run.iter;
  __syncthreads();
}

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
  return fv_launch(&h, 1, n_iters, false, FvDebug{}, stream);
}

int ldc_fv_batch_enqueue(ldc_fv* const* hs, int n, int n_iters, void* stream) {
  if (!hs || n < 1 || n_iters < 1) return LDC_E_ARG;
  for (int q = 0; q < n; ++q) {
    if (!hs[q]) return LDC_E_STATE;
    if (n_iters > hs[q]->rec_cap) return LDC_E_ARG;
  }
  return fv_launch(hs, n, n_iters, false, FvDebug{}, stream);
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
  FvDebug dbg = {};
  for (int k = 0; k < LDC_FV_DBG_COUNT; ++k) {
    if (!(which & (1 << k))) continue;
    if (!out[k]) return LDC_E_ARG;
    dbg.out[k] = out[k];
  }
  return fv_launch(&h, 1, 1, true, dbg, stream);
}

}  // extern "C"
