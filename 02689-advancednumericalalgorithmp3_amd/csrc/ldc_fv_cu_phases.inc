// ldc_fv_cu_phases.inc -- the phases of a SIMPLE iteration on the one-CU mapping (one work-group of 512 threads per trial,
// cells tid, tid + 512, ...; include/ldc_fv.h): the launch arguments, the work-group reduction (fv_reduce, FvRed), the
// GEMM over the waves (fv_gemm), the control words (FvRun) and the seven phase loops fv_assemble ... fv_record.
// Included INSIDE the anonymous namespace of its unit, behind ldc_fv_cells.inc, by ldc_fv_kernel.inc (fv_kernel, at the
// spot where this text stood: the token stream of ldc_kernels.hip is what it was) and by ldc_fv_cu_pressure.hip
// (fv_cu_pressure_kernel, which replaces phases 3, 4 and 6).  The warning of ldc_fv_kernel.inc holds: fv_kernel changes
// with any function around these bodies, so nothing is added here for the other unit's sake.

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
