// ldc_fv_kernel.inc -- the finite-volume SIMPLE solver (include/ldc_fv.h), included at the end of ldc_kernels.hip.
//
// Reference: src/solvers/fv/solver.py:170-257 (one SIMPLE iteration), its assembly / discretisation helpers and
// base.py:202-330 (the loop), 359-450 (E, Z, P by ghost cells).  Quirks: DESIGN.md FV-Q1 ... FV-Q4.
//
// Mapping: ONE work-group of 512 threads (8 waves, two per SIMD) advances ONE trial for a whole chunk of iterations.
// A SIMPLE iteration is a sequence of cell sweeps (each thread takes cells tid, tid + 512, ...) separated by
// __syncthreads(); every scalar the iteration needs (BiCGSTAB dots, norms, the latch, E / Z / P) is a work-group
// reduction through LDS.  No work-group ever waits for another, so a batch launch is B independent work-groups:
// no flags, no spin limits, no co-residency.  512 threads rather than 1024: the iteration's live state takes ~175
// VGPRs, which two waves per SIMD allow; with four (1024 threads, 128 VGPRs) the kernel spilled ~400 registers to
// scratch.  The state of an N = 128 trial (32 vectors of 128 KB) stays L2-resident.
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

// (kFvThreads, kFvWaves, FvVec, FvDesc and struct ldc_fv: ldc_fv_common.inc, shared with ldc_fv_post.hip)

namespace {

constexpr int kFvRed = 10;                  // most values one reduction carries

struct FvLaunch {
  const FvDesc* d[LDC_FV_LAUNCH_MAX];
  int n_iters;
};

struct FvDebug {
  double* out[LDC_FV_DBG_COUNT];
};

// sums of K values over the work-group; every thread gets the same totals (fixed order: bit-reproducible)
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

__device__ inline double fv_muscl(double r) {
  return r > 0 ? fmax(0.0, fmin(fmin(2.0, 2.0 * r), 0.5 * (1 + r))) : 0.0;
}

// TVD deferred correction of a face with owner value fP (west / south cell), neighbour value fN and flux m (P -> N).
// FV-Q1: for m >= 0 the reference's compiled code leaves psi unassigned; the stored converged fields select
// psi = MUSCL(r) by the same formula as the m < 0 branch (profiles/fv_q1_table.md).
__device__ inline double fv_dc(double m, double fP, double fN) {
  double up, down, r;
  const double F_low = m * (m >= 0 ? fP : fN);
  if (m >= 0) {
    up = fP; down = fN;
    const double fW = 2 * fP - fN;
    r = (fN - fP) / (fP - fW + 1e-12);
  } else {
    up = fN; down = fP;
    const double fW = 2 * fN - fP;
    r = (fP - fN) / (fN - fW + 1e-12);
  }
  const double psi = fv_muscl(r);
  return m * (up + 0.5 * psi * (down - up)) - F_low;
}

// central-difference gradient with the reference's rules (structured_gradient.py): the pinned cell 0 has a zero
// gradient, its neighbours skip it, a wall cell averages the one-sided differences it has
__device__ inline void fv_grad(const double* f, int c, int i, int j, int nx, int ny, double dx, double dy,
                               double& gx, double& gy) {
  gx = 0.0; gy = 0.0;
  if (c == 0) return;
  const double fc = f[c];
  double sx = 0.0, sy = 0.0;
  int nxc = 0, nyc = 0;
  if (i > 0 && c - 1 != 0) { sx += (f[c - 1] - fc) / (-dx); ++nxc; }
  if (i < nx - 1) { sx += (f[c + 1] - fc) / dx; ++nxc; }
  if (j > 0 && c - nx != 0) { sy += (f[c - nx] - fc) / (-dy); ++nyc; }
  if (j < ny - 1) { sy += (f[c + nx] - fc) / dy; ++nyc; }
  gx = nxc > 0 ? sx / nxc : 0.0;
  gy = nyc > 0 ? sy / nyc : 0.0;
}

// y = (relaxed A) x at cell c: diag = aP / alpha_uv
__device__ inline double fv_matvec(const double* w, int n, const double* x, int c, int i, int j, int nx, int ny,
                                   double inv_a) {
  double y = (w[FV_AP * n + c] * inv_a) * x[c];
  if (i > 0) y += w[FV_AW * n + c] * x[c - 1];
  if (i < nx - 1) y += w[FV_AE * n + c] * x[c + 1];
  if (j > 0) y += w[FV_AS * n + c] * x[c - nx];
  if (j < ny - 1) y += w[FV_AN * n + c] * x[c + nx];
  return y;
}

// C[r][c] = sum_k A(r, k) B(k, c) (M x N, row-major), A(r, k) = A[r*sar + k*sak], B(k, c) = B[k*sbk + c*sbc].
// One wave per 16 x 16 output tile (waves take tiles round-robin), operands read from L2 with zero fill at the edges;
// SCALE: the fast-diagonalisation epilogue, C[a][b] /= ax*lamx[b] + ay*lamy[a], the (0, 0) zero mode dropped.
template <bool SCALE>
__device__ void fv_gemm(const double* A, int sar, int sak, const double* B, int sbk, int sbc, double* Cm, int M,
                        int N, int K, const double* lamx, const double* lamy, double ax, double ay) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int tn = (N + 15) >> 4, tiles = ((M + 15) >> 4) * tn;
  for (int t = w; t < tiles; t += kFvWaves) {
    const int r0 = (t / tn) * 16, c0 = (t % tn) * 16;
    const int ar = r0 + (lane & 15), bc = c0 + (lane & 15), kq = lane >> 4;
    v4d acc = {0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < K; k0 += 4) {
      const int k = k0 + kq;
      const double a = (ar < M && k < K) ? A[ar * sar + k * sak] : 0.0;
      const double b = (bc < N && k < K) ? B[k * sbk + bc * sbc] : 0.0;
      acc = MFMA_F64(a, b, acc);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int row = r0 + (lane >> 4) + 4 * q, col = c0 + (lane & 15);
      if (row < M && col < N) {
        double val = acc[q];
        if (SCALE) val = (row == 0 && col == 0) ? 0.0 : val * (1.0 / (ax * lamx[col] + ay * lamy[row]));
        Cm[row * N + col] = val;
      }
    }
  }
}

// the BiCGSTAB loop takes the v vector of a pair as vec(u vector, 1)
static_assert(FV_XV == FV_XU + 1 && FV_RV == FV_RU + 1 && FV_RTV == FV_RTU + 1 && FV_PV == FV_PU + 1, "u/v pairs");
static_assert(FV_VV == FV_VU + 1 && FV_PHV == FV_PHU + 1 && FV_SHV == FV_SHU + 1 && FV_TV == FV_TU + 1, "u/v pairs");
static_assert(FV_AN == FV_AP + 4, "the five diagonals are adjacent (LDC_FV_DBG_DIAG)");

// what the phases of an iteration share: the trial's geometry, coefficients and arrays
struct FvCtx {
  const FvDesc& d;
  int nx, ny, n, ldx;
  double dx, dy, V, rho;
  double Dx, Dy, Dbx, Dby;                  // diffusion coefficients of an inner face and of a wall face, per axis
  double inv_a, scale;                      // 1 / alpha_uv and (1 - alpha_uv) / alpha_uv
  bool tvd;
  double *w, *fx, *fy;                      // work vectors; +x and +y face fluxes inside d.mdot

  __device__ __forceinline__ explicit FvCtx(const FvDesc& d_)
      : d(d_), nx(d_.nx), ny(d_.ny), n(nx * ny), ldx(nx + 1), dx(d_.dx), dy(d_.dy), V(dx * dy), rho(d_.rho),
        Dx(d_.mu * dy / dx), Dy(d_.mu * dx / dy), Dbx(d_.mu * dy / (0.5 * dx)), Dby(d_.mu * dx / (0.5 * dy)),
        inv_a(1.0 / d_.alpha_uv), scale((1.0 - d_.alpha_uv) / d_.alpha_uv), tvd(d_.scheme == 1), w(d_.work),
        fx(d_.mdot), fy(d_.mdot + ny * ldx) {}

  // work vector k (k + q: the v vector of a u/v pair), recomputed at each use (held as pointers the 25 vectors
  // spill the register file)
  __device__ __forceinline__ double* vec(FvVec k, int q = 0) const { return w + (k + q) * n; }
};

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

// one component's BiCGSTAB scalars; beta, brk and fin belong to one iteration
struct FvKrylov {
  double atol, nr2, rh, rh_prev, alpha, omega, beta;
  bool act, brk, fin;
  int its;
};

// ---- 1. grad p, the momentum matrix (five diagonals), relaxed right-hand sides, BiCGSTAB start: b2 = |b_u|^2, |b_v|^2
__device__ __forceinline__ void fv_assemble(const FvCtx& x, FvRed& red, double (&b2)[2]) {
  const FvDesc& d = x.d;
  const int nx = x.nx, ny = x.ny, n = x.n, ldx = x.ldx, tid = threadIdx.x;
  double* const w = x.w;
  const double *fx = x.fx, *fy = x.fy;
  b2[0] = 0.0; b2[1] = 0.0;
  for (int c = tid; c < n; c += kFvThreads) {
    const int i = c % nx, j = c / nx;
    double gx, gy;
    fv_grad(d.p, c, i, j, nx, ny, x.dx, x.dy, gx, gy);
    x.vec(FV_GPX)[c] = gx; x.vec(FV_GPY)[c] = gy;
    double aP = 0.0, aW = 0.0, aE = 0.0, aS = 0.0, aN = 0.0, bu = 0.0, bv = 0.0;
    const double uc = d.u[c], vc = d.v[c];
    if (i > 0) {                 // west face: owner c-1, neighbour c
      const double m = fx[j * ldx + i];
      aP += x.Dx - fmin(m, 0.0); aW = -(fmax(m, 0.0) + x.Dx);
      if (x.tvd) { bu += fv_dc(m, d.u[c - 1], uc); bv += fv_dc(m, d.v[c - 1], vc); }
    } else {
      aP += x.Dbx + (-fx[j * ldx]);
    }
    if (i < nx - 1) {            // east face: owner c
      const double m = fx[j * ldx + i + 1];
      aP += fmax(m, 0.0) + x.Dx; aE = fmin(m, 0.0) - x.Dx;
      if (x.tvd) { bu -= fv_dc(m, uc, d.u[c + 1]); bv -= fv_dc(m, vc, d.v[c + 1]); }
    } else {
      aP += x.Dbx + fx[j * ldx + nx];
    }
    if (j > 0) {
      const double m = fy[j * nx + i];
      aP += x.Dy - fmin(m, 0.0); aS = -(fmax(m, 0.0) + x.Dy);
      if (x.tvd) { bu += fv_dc(m, d.u[c - nx], uc); bv += fv_dc(m, d.v[c - nx], vc); }
    } else {
      aP += x.Dby + (-fy[i]);
    }
    if (j < ny - 1) {
      const double m = fy[(j + 1) * nx + i];
      aP += fmax(m, 0.0) + x.Dy; aN = fmin(m, 0.0) - x.Dy;
      if (x.tvd) { bu -= fv_dc(m, uc, d.u[c + nx]); bv -= fv_dc(m, vc, d.v[c + nx]); }
    } else {
      const double mo = fy[ny * nx + i];
      aP += x.Dby + mo;
      bu += (x.Dby + mo) * d.ulid[i];
    }
    w[FV_AP * n + c] = aP; w[FV_AW * n + c] = aW; w[FV_AE * n + c] = aE;
    w[FV_AS * n + c] = aS; w[FV_AN * n + c] = aN;
    w[FV_BU * n + c] = bu; w[FV_BV * n + c] = bv;
    const double hu = (bu - gx * x.V) + x.scale * aP * uc;      // Patankar relaxation (helpers.py:6-25)
    const double hv = (bv - gy * x.V) + x.scale * aP * vc;
    x.vec(FV_XU)[c] = 0.0; x.vec(FV_XV)[c] = 0.0;
    x.vec(FV_RU)[c] = hu; x.vec(FV_RTU)[c] = hu; x.vec(FV_RV)[c] = hv; x.vec(FV_RTV)[c] = hv;
    b2[0] += hu * hu; b2[1] += hv * hv;
  }
  red.sum(b2);
}

// ---- 2. BiCGSTAB for u (q = 0) and v (q = 1) together (SciPy's loop: rtol * |b|, x0 = 0, non-convergence accepted);
//         the sums of both components share each reduction: s2[q], s3[3q .. 3q+2], s4[2q .. 2q+1]
__device__ __forceinline__ void fv_bicgstab(const FvCtx& x, FvRed& red, const double (&b2)[2], FvRun& run) {
  const FvDesc& d = x.d;
  const int nx = x.nx, ny = x.ny, n = x.n, tid = threadIdx.x;
  double* const w = x.w;
  const double inv_a = x.inv_a;
  const double rhotol = 2.220446049250313e-16 * 2.220446049250313e-16;
  FvKrylov s[2];
  for (int q = 0; q < 2; ++q) {
    const double bn = sqrt(b2[q]);
    s[q].nr2 = b2[q]; s[q].rh = b2[q]; s[q].rh_prev = 0; s[q].alpha = 0; s[q].omega = 0; s[q].its = 0;
    s[q].atol = d.lin_tol * bn;
    s[q].act = bn != 0.0;
  }
  for (int it = 0; it < d.maxit; ++it) {
    for (int q = 0; q < 2; ++q) {
      s[q].beta = 0;
      if (!s[q].act) continue;
      if (sqrt(s[q].nr2) < s[q].atol || fabs(s[q].rh) < rhotol || (it > 0 && fabs(s[q].omega) < rhotol)) {
        s[q].act = false; s[q].its = it; continue;
      }
      if (it > 0) s[q].beta = (s[q].rh / s[q].rh_prev) * (s[q].alpha / s[q].omega);
    }
    if (!s[0].act && !s[1].act) break;
    for (int c = tid; c < n; c += kFvThreads) {
      const double dg = w[FV_AP * n + c] * inv_a;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        if (!s[q].act) continue;
        double *p = x.vec(FV_PU, q), *r = x.vec(FV_RU, q);
        const double pp = it > 0 ? (p[c] - s[q].omega * x.vec(FV_VU, q)[c]) * s[q].beta + r[c] : r[c];
        p[c] = pp; x.vec(FV_PHU, q)[c] = pp / dg;
      }
    }
    __syncthreads();
    double s2[2] = {0, 0};
    for (int c = tid; c < n; c += kFvThreads) {
      const int i = c % nx, j = c / nx;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        if (!s[q].act) continue;
        const double y = fv_matvec(w, n, x.vec(FV_PHU, q), c, i, j, nx, ny, inv_a);
        x.vec(FV_VU, q)[c] = y; s2[q] += x.vec(FV_RTU, q)[c] * y;
      }
    }
    red.sum(s2);
    for (int q = 0; q < 2; ++q) {
      s[q].brk = false;
      if (!s[q].act) continue;
      if (s2[q] == 0.0) { s[q].brk = true; continue; }
      s[q].alpha = s[q].rh / s2[q];
    }
    for (int c = tid; c < n; c += kFvThreads) {
      const double dg = w[FV_AP * n + c] * inv_a;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        if (!s[q].act || s[q].brk) continue;
        double* r = x.vec(FV_RU, q);
        const double sv = r[c] - s[q].alpha * x.vec(FV_VU, q)[c];
        r[c] = sv; x.vec(FV_SHU, q)[c] = sv / dg;
      }
    }
    __syncthreads();
    double s3[6] = {0, 0, 0, 0, 0, 0};
    for (int c = tid; c < n; c += kFvThreads) {
      const int i = c % nx, j = c / nx;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        if (!s[q].act || s[q].brk) continue;
        const double t = fv_matvec(w, n, x.vec(FV_SHU, q), c, i, j, nx, ny, inv_a), sv = x.vec(FV_RU, q)[c];
        x.vec(FV_TU, q)[c] = t; s3[3 * q] += sv * sv; s3[3 * q + 1] += t * sv; s3[3 * q + 2] += t * t;
      }
    }
    red.sum(s3);
    for (int q = 0; q < 2; ++q) {
      s[q].fin = false;                      // fin: converged on |s|: x += alpha phat and stop
      if (!s[q].act) continue;
      if (s[q].brk) { s[q].act = false; s[q].its = it + 1; continue; }
      if (sqrt(s3[3 * q]) < s[q].atol) { s[q].fin = true; continue; }
      s[q].omega = s3[3 * q + 1] / s3[3 * q + 2];
    }
    double s4[4] = {0, 0, 0, 0};
    for (int c = tid; c < n; c += kFvThreads) {
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        if (!s[q].act) continue;
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
    for (int q = 0; q < 2; ++q) {
      if (!s[q].act) continue;
      if (s[q].fin) { s[q].act = false; s[q].its = it + 1; continue; }
      s[q].nr2 = s4[2 * q]; s[q].rh_prev = s[q].rh; s[q].rh = s4[2 * q + 1];
      s[q].its = it + 1;
    }
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
  double *fx = x.fx, *fy = x.fy;
  const double V = x.V;
  double csum[1] = {0.0};
  for (int c = tid; c < n; c += kFvThreads) {
    const int i = c % nx, j = c / nx;
    const double DP = V / (w[FV_AP * n + c] + 1e-14);
    double flux[4];                      // W, E, S, N in +x / +y
    for (int f = 0; f < 4; ++f) {
      const bool xdir = f < 2;
      const int o = f == 0 ? c - 1 : f == 1 ? c + 1 : f == 2 ? c - nx : c + nx;
      const bool wall = f == 0 ? i == 0 : f == 1 ? i == nx - 1 : f == 2 ? j == 0 : j == ny - 1;
      if (wall) { flux[f] = 0.0; continue; }     // boundary velocity has no normal component
      const int P = (f == 0 || f == 2) ? o : c, N = (f == 0 || f == 2) ? c : o;
      const double g = 0.5;
      const double* st = xdir ? x.vec(FV_XU) : x.vec(FV_XV);
      const double* gp = xdir ? x.vec(FV_GPX) : x.vec(FV_GPY);
      const double DPc = P == c ? DP : V / (w[FV_AP * n + P] + 1e-14);
      const double DNc = N == c ? DP : V / (w[FV_AP * n + N] + 1e-14);
      const double Uf = (1.0 - g) * st[P] + g * st[N];
      const double gbar = g * gp[N] + (1.0 - g) * gp[P];          // interpolate_to_face(grad_p)
      const double gin = (1.0 - g) * gp[P] + g * gp[N];           // rhie_chow.py's inline interpolation (FV-Q2)
      const double Df = g * DNc + (1.0 - g) * DPc;
      flux[f] = x.rho * ((Uf - Df * (gbar - gin)) * (xdir ? x.dy : x.dx));
    }
    if (i == 0) fx[j * ldx] = flux[0];
    fx[j * ldx + i + 1] = flux[1];
    if (j == 0) fy[i] = flux[2];
    fy[(j + 1) * nx + i] = flux[3];
    const double rhs = c == 0 ? 0.0 : -((flux[1] - flux[0]) + (flux[3] - flux[2]));
    x.vec(FV_C)[c] = rhs;
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
  const FvDesc& d = x.d;
  const int nx = x.nx, ny = x.ny, n = x.n, ldx = x.ldx, tid = threadIdx.x;
  double *fx = x.fx, *fy = x.fy;
  const double dx = x.dx, dy = x.dy, rho = x.rho;
  for (int c = tid; c < n; c += kFvThreads) {
    const int i = c % nx, j = c / nx;
    const double *up = x.vec(FV_UP), *vp = x.vec(FV_VP);
    const double ue = i < nx - 1 ? 0.5 * up[c + 1] + (1.0 - 0.5) * up[c] : up[c];
    const double vn = j < ny - 1 ? 0.5 * vp[c + nx] + (1.0 - 0.5) * vp[c] : vp[c];
    if (i == 0) fx[j * ldx] += rho * (up[c] * dy);
    fx[j * ldx + i + 1] += rho * (ue * dy);
    if (j == 0) fy[i] += rho * (vp[c] * dx);
    fy[(j + 1) * nx + i] += rho * (vn * dx);
    const double vE = i < nx - 1 ? d.v[c + 1] : -d.v[c], vW = i > 0 ? d.v[c - 1] : -d.v[c];
    const double uN = j < ny - 1 ? d.u[c + nx] : 2 * d.lid - d.u[c], uS = j > 0 ? d.u[c - nx] : -d.u[c];
    const double wc = (vE - vW) / (2 * dx) - (uN - uS) / (2 * dy);
    x.vec(FV_OMEGA)[c] = wc;
    part[8] += wc * wc;
  }
  __syncthreads();
}

// ---- 7. |div mdot|, palinstrophy, record row k of this launch and the latch ---------------------------------------
template <bool DEBUG>
__device__ __forceinline__ void fv_record(const FvCtx& x, FvRed& red, double (&part)[kFvRed], int k, FvRun& run,
                                          const FvDebug& dbg) {
  const FvDesc& d = x.d;
  const int nx = x.nx, ny = x.ny, n = x.n, ldx = x.ldx, tid = threadIdx.x;
  const double *fx = x.fx, *fy = x.fy;
  const double dx = x.dx, dy = x.dy, V = x.V;
  for (int c = tid; c < n; c += kFvThreads) {
    const int i = c % nx, j = c / nx;
    const double* om = x.vec(FV_OMEGA);
    const double dv = (fx[j * ldx + i + 1] - fx[j * ldx + i]) + (fy[(j + 1) * nx + i] - fy[j * nx + i]);
    part[7] += dv * dv;
    const double wc = om[c];
    const double wE = i < nx - 1 ? om[c + 1] : -wc, wW = i > 0 ? om[c - 1] : -wc;
    const double wN = j < ny - 1 ? om[c + nx] : -wc, wS = j > 0 ? om[c - nx] : -wc;
    const double gx = (wE - wW) / (2 * dx), gy = (wN - wS) / (2 * dy);
    part[9] += gx * gx + gy * gy;
  }
  red.sum(part);
  if constexpr (DEBUG) {
    if (dbg.out[LDC_FV_DBG_MDOT]) {
      const int nf = ny * ldx + (ny + 1) * nx;
      for (int f = tid; f < nf; f += kFvThreads) dbg.out[LDC_FV_DBG_MDOT][f] = d.mdot[f];
    }
  }
  const double chu = sqrt(part[0]) / (sqrt(part[1]) + 1e-12), chv = sqrt(part[2]) / (sqrt(part[3]) + 1e-12);
  const double rel = chu > chv ? chu : chv;
  if (tid == 0) {
    double* row = d.rec + (long long)k * LDC_FV_REC_LEN;
    row[0] = rel; row[1] = sqrt(part[4]); row[2] = sqrt(part[5]); row[3] = sqrt(part[7]);
    row[4] = 0.5 * (part[6] * V); row[5] = 0.5 * (part[8] * V); row[6] = 0.5 * (part[9] * V); row[7] = 0.0;
  }
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
  if (pr->nx < LDC_FV_MIN_N || pr->nx > LDC_FV_MAX_N || pr->ny < LDC_FV_MIN_N || pr->ny > LDC_FV_MAX_N) return LDC_E_ARG;
  if (pr->scheme != 0 && pr->scheme != 1) return LDC_E_ARG;
  if (pr->rec_cap < 1 || pr->warmup < 0 || pr->max_lin_iters < 1) return LDC_E_ARG;
  if (!(pr->dx > 0) || !(pr->dy > 0) || !(pr->rho > 0) || !(pr->mu > 0)) return LDC_E_ARG;
  if (!(pr->alpha_uv > 0 && pr->alpha_uv <= 1) || !(pr->alpha_p > 0 && pr->alpha_p <= 1)) return LDC_E_ARG;
  if (!(pr->lin_tol > 0) || !(pr->tol >= 0)) return LDC_E_ARG;
  const void* req[] = {pr->ulid, pr->Qx, pr->lamx, pr->Qy, pr->lamy, pr->u, pr->v, pr->p, pr->mdot, pr->work,
                       pr->rec, pr->ctrl};
  for (const void* q : req) if (!q) return LDC_E_ARG;
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) return LDC_E_NODEVICE;
  FvDesc h;
  h.nx = pr->nx; h.ny = pr->ny; h.scheme = pr->scheme; h.rec_cap = pr->rec_cap; h.warmup = pr->warmup;
  h.maxit = pr->max_lin_iters;
  h.dx = pr->dx; h.dy = pr->dy; h.rho = pr->rho; h.mu = pr->mu; h.alpha_uv = pr->alpha_uv; h.alpha_p = pr->alpha_p;
  h.lin_tol = pr->lin_tol; h.tol = pr->tol; h.lid = pr->lid_velocity;
  h.ulid = pr->ulid; h.Qx = pr->Qx; h.lamx = pr->lamx; h.Qy = pr->Qy; h.lamy = pr->lamy;
  h.u = pr->u; h.v = pr->v; h.p = pr->p; h.mdot = pr->mdot; h.work = pr->work; h.rec = pr->rec;
  h.ctrl = reinterpret_cast<long long*>(pr->ctrl);
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
