// ldc_fv_cells.inc -- the arithmetic of one finite-volume SIMPLE iteration (include/ldc_fv.h), written once for every
// mapping of a trial onto the card.  Included by ldc_kernels.hip ahead of ldc_fv_kernel.inc (one trial per CU) and by
// ldc_fv_wide.hip (mapping="chip" and "shared"); everything is a device function in the anonymous namespace, so each
// unit compiles its own copy and neither code object depends on the other.
//
// Reference: src/solvers/fv/solver.py:170-257 (one SIMPLE iteration), its assembly / discretisation helpers and
// base.py:202-330 (the loop), 359-450 (E, Z, P by ghost cells).  Quirks: DESIGN.md FV-Q1 ... FV-Q4.
//
// What is here: the context of a trial (FvCtx), one function per cell body of a sweep (fv_cell_*: cell c of the trial,
// adding to the caller's partial sums; two bodies are missing and say so where they would stand), the scalar steps of
// BiCGSTAB for one component (fv_kry_*), the record row from the ten sums (fv_rec_*) and one 16 x 16 tile of the
// fast-diagonalisation GEMM (fv_gemm_tile).
// What a mapping supplies: the cell loop (which cells a thread takes), the reduction of the partial sums, the barriers
// or launch boundaries between the sweeps, and a place for the Krylov scalars between them.
#ifndef LDC_FV_CELLS_INC
#define LDC_FV_CELLS_INC

#include "ldc_fv_common.inc"

namespace {

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

// the BiCGSTAB sweeps take the v vector of a pair as vec(u vector, 1)
static_assert(FV_XV == FV_XU + 1 && FV_RV == FV_RU + 1 && FV_RTV == FV_RTU + 1 && FV_PV == FV_PU + 1, "u/v pairs");
static_assert(FV_VV == FV_VU + 1 && FV_PHV == FV_PHU + 1 && FV_SHV == FV_SHU + 1 && FV_TV == FV_TU + 1, "u/v pairs");

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

// one component's BiCGSTAB scalars; beta, brk and fin belong to one iteration
struct FvKrylov {
  double atol, nr2, rh, rh_prev, alpha, omega, beta;
  bool act, brk, fin;
  int its;
};

// ---- 1. assembly: grad p, the momentum matrix (five diagonals), the relaxed right-hand sides, x = 0 and r = rtilde = b;
//         b2 += |b_u|^2, |b_v|^2
__device__ __forceinline__ void fv_cell_assemble(const FvCtx& x, int c, double (&b2)[2]) {
  const FvDesc& d = x.d;
  const int nx = x.nx, ny = x.ny, n = x.n, ldx = x.ldx;
  double* const w = x.w;
  const double *fx = x.fx, *fy = x.fy;
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

// ---- 2. the joint u (q = 0) / v (q = 1) BiCGSTAB (SciPy's loop: rtol * |b|, x0 = 0, non-convergence accepted).
// The scalar steps, one component per call, in the order of an iteration:
// the start from |b|^2
__device__ __forceinline__ void fv_kry_start(FvKrylov& s, double b2, double lin_tol) {
  const double bn = sqrt(b2);
  s.nr2 = b2; s.rh = b2; s.rh_prev = 0; s.alpha = 0; s.omega = 0; s.beta = 0; s.its = 0;
  s.atol = lin_tol * bn;
  s.act = bn != 0.0; s.brk = false; s.fin = false;
}

// the test at the head of iteration `it`: converged or broken down -> finished with `it` iterations; else beta
__device__ __forceinline__ void fv_kry_head(FvKrylov& s, int it) {
  const double rhotol = 2.220446049250313e-16 * 2.220446049250313e-16;
  s.beta = 0;
  if (!s.act) return;
  if (sqrt(s.nr2) < s.atol || fabs(s.rh) < rhotol || (it > 0 && fabs(s.omega) < rhotol)) {
    s.act = false; s.its = it; return;
  }
  if (it > 0) s.beta = (s.rh / s.rh_prev) * (s.alpha / s.omega);
}

// alpha from s2 = rtilde . v (brk: the breakdown rtilde . v = 0)
__device__ __forceinline__ void fv_kry_alpha(FvKrylov& s, double s2) {
  s.brk = false;
  if (!s.act) return;
  if (s2 == 0.0) { s.brk = true; return; }
  s.alpha = s.rh / s2;
}

// omega from s.s, t.s, t.t of iteration `it` (fin: converged on |s|: x += alpha phat and stop)
__device__ __forceinline__ void fv_kry_omega(FvKrylov& s, double ss, double ts, double tt, int it) {
  s.fin = false;
  if (!s.act) return;
  if (s.brk) { s.act = false; s.its = it + 1; return; }
  if (sqrt(ss) < s.atol) { s.fin = true; return; }
  s.omega = ts / tt;
}

// after the x sweep of the iteration that makes `its` in all: rr = r . r, rtr = rtilde . r
__device__ __forceinline__ void fv_kry_after_x(FvKrylov& s, double rr, double rtr, int its) {
  if (!s.act) return;
  if (s.fin) { s.act = false; s.its = its; return; }
  s.nr2 = rr; s.rh_prev = s.rh; s.rh = rtr;
  s.its = its;
}

// The cell sweeps of iteration `it`, for component q of cell c; the caller skips a component that is not active (s
// and t: or has broken down).  dg: the relaxed diagonal of the cell, aP / alpha_uv; i, j: the cell's column and row.
// p = r + beta (p - omega v) and phat = p / diag
__device__ __forceinline__ void fv_cell_p(const FvCtx& x, int c, int q, int it, const FvKrylov s, double dg) {
  double *p = x.vec(FV_PU, q), *r = x.vec(FV_RU, q);
  const double pp = it > 0 ? (p[c] - s.omega * x.vec(FV_VU, q)[c]) * s.beta + r[c] : r[c];
  p[c] = pp; x.vec(FV_PHU, q)[c] = pp / dg;
}

// v = A phat; s2 += rtilde . v
__device__ __forceinline__ void fv_cell_v(const FvCtx& x, int c, int i, int j, int q, double& s2) {
  const double y = fv_matvec(x.w, x.n, x.vec(FV_PHU, q), c, i, j, x.nx, x.ny, x.inv_a);
  x.vec(FV_VU, q)[c] = y; s2 += x.vec(FV_RTU, q)[c] * y;
}

// s = r - alpha v (into r) and shat = s / diag
__device__ __forceinline__ void fv_cell_s(const FvCtx& x, int c, int q, const FvKrylov s, double dg) {
  double* r = x.vec(FV_RU, q);
  const double sv = r[c] - s.alpha * x.vec(FV_VU, q)[c];
  r[c] = sv; x.vec(FV_SHU, q)[c] = sv / dg;
}

// t = A shat; s3[0 .. 2] += s.s, t.s, t.t
__device__ __forceinline__ void fv_cell_t(const FvCtx& x, int c, int i, int j, int q, double* s3) {
  const double t = fv_matvec(x.w, x.n, x.vec(FV_SHU, q), c, i, j, x.nx, x.ny, x.inv_a), sv = x.vec(FV_RU, q)[c];
  x.vec(FV_TU, q)[c] = t; s3[0] += sv * sv; s3[1] += t * sv; s3[2] += t * t;
}

// x += alpha phat + omega shat and r = s - omega t (fin: x += alpha phat alone) is NOT here: fv_bicgstab of
// ldc_fv_kernel.inc and wide_bicg_x of ldc_fv_wide.hip each hold that cell body, because the one-CU kernel changes with
// any function around it (profiles/fv_wide.md).  A change to one of them goes into the other.

// ---- 3. Rhie-Chow face velocities and mdot* on the faces of cell c; rhs = rhs_p[c] = -div mdot* (rhs_p[0] = 0, the
//         caller's to sum: minus the total is the cell-0 entry of the pinned solve)
__device__ __forceinline__ void fv_cell_faces(const FvCtx& x, int c, double& rhs) {
  const int nx = x.nx, ny = x.ny, n = x.n, ldx = x.ldx;
  double* const w = x.w;
  double *fx = x.fx, *fy = x.fy;
  const double V = x.V;
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
  rhs = c == 0 ? 0.0 : -((flux[1] - flux[0]) + (flux[3] - flux[2]));
  x.vec(FV_C)[c] = rhs;
}

// ---- 4. the 16 x 16 tile at (r0, c0) of C[r][c] = sum_k A(r, k) B(k, c) (M x N, row-major), A(r, k) = A[r*sar + k*sak],
//         B(k, c) = B[k*sbk + c*sbc], by one wave (`lane` of it) on fp64 MFMA; operands read from L2 with zero fill at
//         the edges.  FIRST: entry (0, 0) of B is b00 and not what memory holds.  SCALE: the fast-diagonalisation
//         epilogue, C[a][b] /= ax*lamx[b] + ay*lamy[a], the (0, 0) zero mode dropped.
template <bool SCALE, bool FIRST>
__device__ __forceinline__ void fv_gemm_tile(const double* A, int sar, int sak, const double* B, int sbk, int sbc,
                                             double* Cm, int M, int N, int K, int r0, int c0, int lane,
                                             const double* lamx, const double* lamy, double ax, double ay, double b00) {
  const int ar = r0 + (lane & 15), bc = c0 + (lane & 15), kq = lane >> 4;
  v4d acc = {0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < K; k0 += 4) {
    const int k = k0 + kq;
    const double a = (ar < M && k < K) ? A[ar * sar + k * sak] : 0.0;
    double b = (bc < N && k < K) ? B[k * sbk + bc * sbc] : 0.0;
    if (FIRST && k == 0 && bc == 0) b = b00;
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

// ---- 5. the correction of u, v and p by u', v', p' is NOT here: ldc_fv_kernel.inc (fv_correct) and ldc_fv_wide.hip
//         (wide_correct) each hold the cell body, because the one-CU debug kernel changes with any function around it
//         (profiles/fv_wide.md).  A change to one of them goes into the other.

// ---- 6. mdot += rho interp(u', v') . S (walls: rho u'_P |S|, FV-Q4); the vorticity with ghost cells; w2 += omega^2
__device__ __forceinline__ void fv_cell_flux_vorticity(const FvCtx& x, int c, double& w2) {
  const FvDesc& d = x.d;
  const int nx = x.nx, ny = x.ny, ldx = x.ldx;
  double *fx = x.fx, *fy = x.fy;
  const double dx = x.dx, dy = x.dy, rho = x.rho;
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
  w2 += wc * wc;
}

// ---- 7. div2 += (div mdot)^2, gw2 += |grad omega|^2 (ghost cells); the record row from the ten sums
__device__ __forceinline__ void fv_cell_div_palinstrophy(const FvCtx& x, int c, double& div2, double& gw2) {
  const int nx = x.nx, ny = x.ny, ldx = x.ldx;
  const double *fx = x.fx, *fy = x.fy;
  const double dx = x.dx, dy = x.dy;
  const int i = c % nx, j = c / nx;
  const double* om = x.vec(FV_OMEGA);
  const double dv = (fx[j * ldx + i + 1] - fx[j * ldx + i]) + (fy[(j + 1) * nx + i] - fy[j * nx + i]);
  div2 += dv * dv;
  const double wc = om[c];
  const double wE = i < nx - 1 ? om[c + 1] : -wc, wW = i > 0 ? om[c - 1] : -wc;
  const double wN = j < ny - 1 ? om[c + nx] : -wc, wS = j > 0 ? om[c - nx] : -wc;
  const double gx = (wE - wW) / (2 * dx), gy = (wN - wS) / (2 * dy);
  gw2 += gx * gx + gy * gy;
}

// part: the totals of du^2, u_old^2, dv^2, v_old^2, u'^2, v'^2, u^2+v^2, div^2, w^2, |grad w|^2 over the trial.
// The relative change of the iteration (what the latch tests) ...
__device__ __forceinline__ double fv_rec_rel(const double (&part)[10]) {
  const double chu = sqrt(part[0]) / (sqrt(part[1]) + 1e-12), chv = sqrt(part[2]) / (sqrt(part[3]) + 1e-12);
  return chu > chv ? chu : chv;
}

// ... and the record row (LDC_FV_REC_LEN entries; V: a cell's volume)
__device__ __forceinline__ void fv_rec_row(double* row, double rel, const double (&part)[10], double V) {
  row[0] = rel; row[1] = sqrt(part[4]); row[2] = sqrt(part[5]); row[3] = sqrt(part[7]);
  row[4] = 0.5 * (part[6] * V); row[5] = 0.5 * (part[8] * V); row[6] = 0.5 * (part[9] * V); row[7] = 0.0;
}

}  // namespace

#endif  // LDC_FV_CELLS_INC
