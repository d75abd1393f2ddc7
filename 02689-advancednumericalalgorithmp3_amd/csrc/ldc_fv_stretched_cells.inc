// ldc_fv_stretched_cells.inc -- the per-cell arithmetic of a SIMPLE iteration on a wall-clustered tensor grid (include/ldc_fv.h,
// "Stretched grids of a one-CU trial" and "Stretched grids of a chip trial"), written once for every mapping: the context
// with the tables of both axes (SgCtx), the gradient (sg_grad), one function per cell body of a sweep (sg_cell_*), the face
// weights and the row of the consistent operator (sg_wx, sg_wy, sg_row) and the Gauss rule (sg_gauss).  Each names its twin
// on the uniform grid.
// Included INSIDE the anonymous namespace of its unit, behind ldc_fv_cells.inc and ldc_fv_pressure_cells.inc: by
// ldc_fv_stretched.hip and ldc_fv_stretched_sep.hip through ldc_fv_stretched_phases.inc (one work-group per trial: the loops,
// the reductions and the barriers are there) and by ldc_fv_wide.hip through ldc_fv_wide_stretched.inc (one launch per phase
// over the whole chip).  Each unit compiles its own copy and no code object depends on another's.
// What a mapping supplies: the cell loop, the reduction of the partial sums, the barriers or launch boundaries.

// the trial's context with the tables of both axes
struct SgCtx {
  const FvCtx& x;
  const double *hx, *dxf, *gxf, *hy, *dyf, *gyf;
  __device__ __forceinline__ SgCtx(const FvCtx& x_, const FvGridBlk& g)
      : x(x_), hx(g.ax), dxf(g.ax + x_.nx), gxf(g.ax + 2 * x_.nx + 1), hy(g.ay), dyf(g.ay + x_.ny),
        gyf(g.ay + 2 * x_.ny + 1) {}
  __device__ __forceinline__ double V(int i, int j) const { return hx[i] * hy[j]; }
  __device__ __forceinline__ double D(int c, int i, int j) const { return V(i, j) / (x.w[FV_AP * x.n + c] + 1e-14); }
};

// twin of fv_grad (ldc_fv_cells.inc): the distances of the faces instead of dx, dy
__device__ __forceinline__ void sg_grad(const SgCtx& s, const double* f, int c, int i, int j, double& gx, double& gy) {
  const int nx = s.x.nx, ny = s.x.ny;
  gx = 0.0; gy = 0.0;
  if (c == 0) return;
  const double fc = f[c];
  double sx = 0.0, sy = 0.0;
  int nxc = 0, nyc = 0;
  if (i > 0 && c - 1 != 0) { sx += (f[c - 1] - fc) / (-s.dxf[i]); ++nxc; }
  if (i < nx - 1) { sx += (f[c + 1] - fc) / s.dxf[i + 1]; ++nxc; }
  if (j > 0 && c - nx != 0) { sy += (f[c - nx] - fc) / (-s.dyf[j]); ++nyc; }
  if (j < ny - 1) { sy += (f[c + nx] - fc) / s.dyf[j + 1]; ++nyc; }
  gx = nxc > 0 ? sx / nxc : 0.0;
  gy = nyc > 0 ? sy / nyc : 0.0;
}

// ---- 1. twin of fv_cell_assemble: the diffusion coefficient of a face is mu |S| / d, the walls' d being h / 2
__device__ __forceinline__ void sg_cell_assemble(const SgCtx& s, int c, double (&b2)[2]) {
  const FvCtx& x = s.x;
  const FvDesc& d = x.d;
  const int nx = x.nx, ny = x.ny, n = x.n, ldx = x.ldx;
  double* const w = x.w;
  const double *fx = x.fx, *fy = x.fy;
  const int i = c % nx, j = c / nx;
  const double hx = s.hx[i], hy = s.hy[j], V = hx * hy, mu = d.mu;
  double gx, gy;
  sg_grad(s, d.p, c, i, j, gx, gy);
  x.vec(FV_GPX)[c] = gx; x.vec(FV_GPY)[c] = gy;
  double aP = 0.0, aW = 0.0, aE = 0.0, aS = 0.0, aN = 0.0, bu = 0.0, bv = 0.0;
  const double uc = d.u[c], vc = d.v[c];
  const double DW = mu * hy / s.dxf[i], DE = mu * hy / s.dxf[i + 1], DS = mu * hx / s.dyf[j], DN = mu * hx / s.dyf[j + 1];
  if (i > 0) {
    const double m = fx[j * ldx + i];
    aP += DW - fmin(m, 0.0); aW = -(fmax(m, 0.0) + DW);
    if (x.tvd) { bu += fv_dc(m, d.u[c - 1], uc); bv += fv_dc(m, d.v[c - 1], vc); }
  } else {
    aP += DW + (-fx[j * ldx]);
  }
  if (i < nx - 1) {
    const double m = fx[j * ldx + i + 1];
    aP += fmax(m, 0.0) + DE; aE = fmin(m, 0.0) - DE;
    if (x.tvd) { bu -= fv_dc(m, uc, d.u[c + 1]); bv -= fv_dc(m, vc, d.v[c + 1]); }
  } else {
    aP += DE + fx[j * ldx + nx];
  }
  if (j > 0) {
    const double m = fy[j * nx + i];
    aP += DS - fmin(m, 0.0); aS = -(fmax(m, 0.0) + DS);
    if (x.tvd) { bu += fv_dc(m, d.u[c - nx], uc); bv += fv_dc(m, d.v[c - nx], vc); }
  } else {
    aP += DS + (-fy[i]);
  }
  if (j < ny - 1) {
    const double m = fy[(j + 1) * nx + i];
    aP += fmax(m, 0.0) + DN; aN = fmin(m, 0.0) - DN;
    if (x.tvd) { bu -= fv_dc(m, uc, d.u[c + nx]); bv -= fv_dc(m, vc, d.v[c + nx]); }
  } else {
    const double mo = fy[ny * nx + i];
    aP += DN + mo;
    bu += (DN + mo) * d.ulid[i];
  }
  w[FV_AP * n + c] = aP; w[FV_AW * n + c] = aW; w[FV_AE * n + c] = aE;
  w[FV_AS * n + c] = aS; w[FV_AN * n + c] = aN;
  w[FV_BU * n + c] = bu; w[FV_BV * n + c] = bv;
  const double hu = (bu - gx * V) + x.scale * aP * uc;
  const double hv = (bv - gy * V) + x.scale * aP * vc;
  x.vec(FV_XU)[c] = 0.0; x.vec(FV_XV)[c] = 0.0;
  x.vec(FV_RU)[c] = hu; x.vec(FV_RTU)[c] = hu; x.vec(FV_RV)[c] = hv; x.vec(FV_RTV)[c] = hv;
  b2[0] += hu * hu; b2[1] += hv * hv;
}

// ---- 3. twin of fv_cell_faces: g from the tables, D with each cell's own volume, |S| = hy_j or hx_i.
//         fx, fy: where mdot* goes (mdot itself, or the dead work vectors PCG_MS of the consistent mode)
__device__ __forceinline__ void sg_cell_faces(const SgCtx& s, double* fx, double* fy, int c, double& rhs) {
  const FvCtx& x = s.x;
  const int nx = x.nx, ny = x.ny, ldx = x.ldx;
  const int i = c % nx, j = c / nx;
  const double DP = s.D(c, i, j);
  double flux[4];                      // W, E, S, N in +x / +y
  for (int f = 0; f < 4; ++f) {
    const bool xdir = f < 2;
    const int o = f == 0 ? c - 1 : f == 1 ? c + 1 : f == 2 ? c - nx : c + nx;
    const bool wall = f == 0 ? i == 0 : f == 1 ? i == nx - 1 : f == 2 ? j == 0 : j == ny - 1;
    if (wall) { flux[f] = 0.0; continue; }
    const int P = (f == 0 || f == 2) ? o : c, N = (f == 0 || f == 2) ? c : o;
    const double g = f == 0 ? s.gxf[i] : f == 1 ? s.gxf[i + 1] : f == 2 ? s.gyf[j] : s.gyf[j + 1];
    const int io = f == 0 ? i - 1 : f == 1 ? i + 1 : i, jo = f == 2 ? j - 1 : f == 3 ? j + 1 : j;
    const double Do = s.D(o, io, jo);
    const double* st = xdir ? x.vec(FV_XU) : x.vec(FV_XV);
    const double* gp = xdir ? x.vec(FV_GPX) : x.vec(FV_GPY);
    const double DPc = P == c ? DP : Do, DNc = N == c ? DP : Do;
    const double Uf = (1.0 - g) * st[P] + g * st[N];
    const double gbar = g * gp[N] + (1.0 - g) * gp[P];
    const double gin = (1.0 - g) * gp[P] + g * gp[N];
    const double Df = g * DNc + (1.0 - g) * DPc;
    flux[f] = x.rho * ((Uf - Df * (gbar - gin)) * (xdir ? s.hy[j] : s.hx[i]));
  }
  if (i == 0) fx[j * ldx] = flux[0];
  fx[j * ldx + i + 1] = flux[1];
  if (j == 0) fy[i] = flux[2];
  fy[(j + 1) * nx + i] = flux[3];
  rhs = c == 0 ? 0.0 : -((flux[1] - flux[0]) + (flux[3] - flux[2]));
  x.vec(FV_C)[c] = rhs;
}

// the weight of the inner x face k (between cells i = k - 1 and k of row j) / the inner y face k of column i;
// twin of wide_pcg_w: w_f = rho (g D_N + (1 - g) D_P) |S| / d
__device__ __forceinline__ double sg_wx(const SgCtx& s, int j, int k, double DP, double DN) {
  const double g = s.gxf[k];
  return (s.x.rho * (g * DN + (1.0 - g) * DP)) * (s.hy[j] / s.dxf[k]);
}
__device__ __forceinline__ double sg_wy(const SgCtx& s, int i, int k, double DP, double DN) {
  const double g = s.gyf[k];
  return (s.x.rho * (g * DN + (1.0 - g) * DP)) * (s.hx[i] / s.dyf[k]);
}

// twin of wide_pcg_row: (A p)_c; pv(k): the value of p at cell k, pc = pv(c)
template <class PV>
__device__ __forceinline__ double sg_row(const SgCtx& s, int c, int i, int j, double pc, PV pv) {
  const int nx = s.x.nx, ny = s.x.ny;
  const double Dc = s.D(c, i, j);
  double y = 0.0;
  if (i > 0) y += sg_wx(s, j, i, s.D(c - 1, i - 1, j), Dc) * (pc - pv(c - 1));
  if (i < nx - 1) y += sg_wx(s, j, i + 1, Dc, s.D(c + 1, i + 1, j)) * (pc - pv(c + 1));
  if (j > 0) y += sg_wy(s, i, j, s.D(c - nx, i, j - 1), Dc) * (pc - pv(c - nx));
  if (j < ny - 1) y += sg_wy(s, i, j + 1, Dc, s.D(c + nx, i, j + 1)) * (pc - pv(c + nx));
  return y;
}
// (the same with p stored: the CG loop of a one-CU trial)
__device__ __forceinline__ double sg_row(const SgCtx& s, int c, int i, int j, double pc, const double* p) {
  return sg_row(s, c, i, j, pc, [p](int k) { return p[k]; });
}

// the diagonal scaling of the separable preconditioner (Concus and Golub) at cell c: s_c = sqrt(a_i b_j / D_c), a and b the
// fitted factors of the two axes (the heads of the tables of ldc_fv_set_preconditioner / ldc_fv_wide_set_preconditioner).
// One definition for SepPolicy::start (ldc_fv_stretched_sep.hip) and wide_sep_init (ldc_fv_wide_separable.inc)
__device__ __forceinline__ double sg_sep_scale(const SgCtx& s, const double* a, const double* b, int c, int i, int j) {
  return sqrt((a[i] * b[j]) / s.D(c, i, j));
}

// ---- 5. twin of the cell body of fv_correct<false>: the gradient and D of this grid; u^2 + v^2 weighted by the cell's
//         volume.  y0 = y[0]; part: the record sums 0 .. 6
template <int K>
__device__ __forceinline__ void sg_cell_correct(const SgCtx& s, double y0, int c, double (&part)[K]) {
  static_assert(K >= 7, "record sums 0 .. 6");
  const FvCtx& x = s.x;
  const FvDesc& d = x.d;
  const int i = c % x.nx, j = c / x.nx;
  double gx, gy;
  sg_grad(s, x.vec(FV_Y), c, i, j, gx, gy);
  const double D = s.D(c, i, j);
  const double upc = -D * gx, vpc = -D * gy;
  const double un = x.vec(FV_XU)[c] + upc, vn = x.vec(FV_XV)[c] + vpc, uo = d.u[c], vo = d.v[c];
  const double pp = x.vec(FV_Y)[c] - y0;
  d.p[c] += d.alpha_p * pp;
  d.u[c] = un; d.v[c] = vn; x.vec(FV_UP)[c] = upc; x.vec(FV_VP)[c] = vpc;
  part[0] += (un - uo) * (un - uo); part[1] += uo * uo;
  part[2] += (vn - vo) * (vn - vo); part[3] += vo * vo;
  part[4] += upc * upc; part[5] += vpc * vpc; part[6] += (un * un + vn * vn) * s.V(i, j);
}

// d f / dx and d f / dy at cell c by the Gauss rule: (f_e - f_w) / hx_i with g-weighted face values; a wall face takes the
// wall's own value: 0, or lid[i] on the lid when lid is not null
__device__ __forceinline__ void sg_gauss(const SgCtx& s, const double* f, const double* lid, int c, int i, int j,
                                         double& gx, double& gy) {
  const int nx = s.x.nx, ny = s.x.ny;
  const double fc = f[c];
  const double gw = s.gxf[i], ge = s.gxf[i + 1], gs = s.gyf[j], gn = s.gyf[j + 1];
  const double fw = i > 0 ? gw * fc + (1.0 - gw) * f[c - 1] : 0.0;
  const double fe = i < nx - 1 ? ge * f[c + 1] + (1.0 - ge) * fc : 0.0;
  const double fs = j > 0 ? gs * fc + (1.0 - gs) * f[c - nx] : 0.0;
  const double fn = j < ny - 1 ? gn * f[c + nx] + (1.0 - gn) * fc : (lid ? lid[i] : 0.0);
  gx = (fe - fw) / s.hx[i];
  gy = (fn - fs) / s.hy[j];
}

// ---- 6. the corrected face fluxes of either mode at cell c, then omega = dv/dx - du/dy; w2 += omega^2 V (record sum 8)
template <bool CONSISTENT>
__device__ __forceinline__ void sg_cell_fluxvort(const SgCtx& s, int c, double& w2) {
  const FvCtx& x = s.x;
  const FvDesc& d = x.d;
  const int nx = x.nx, ny = x.ny, ldx = x.ldx;
  double *fx = x.fx, *fy = x.fy;
  const int i = c % nx, j = c / nx;
  if (CONSISTENT) {                    // twin of wide_pcg_cell_fluxvort
    const double *pp = x.vec(FV_Y), *sx = x.vec(PCG_MS), *sy = x.vec(PCG_MS) + ny * ldx;
    const double Dc = s.D(c, i, j);
    if (i == 0) fx[j * ldx] = 0.0;
    fx[j * ldx + i + 1] =
        i < nx - 1 ? sx[j * ldx + i + 1] - sg_wx(s, j, i + 1, Dc, s.D(c + 1, i + 1, j)) * (pp[c + 1] - pp[c]) : 0.0;
    if (j == 0) fy[i] = 0.0;
    fy[(j + 1) * nx + i] =
        j < ny - 1 ? sy[(j + 1) * nx + i] - sg_wy(s, i, j + 1, Dc, s.D(c + nx, i, j + 1)) * (pp[c + nx] - pp[c]) : 0.0;
  } else {                             // twin of the first half of fv_cell_flux_vorticity (FV-Q4 kept)
    const double *up = x.vec(FV_UP), *vp = x.vec(FV_VP);
    const double ge = s.gxf[i + 1], gn = s.gyf[j + 1], hx = s.hx[i], hy = s.hy[j], rho = x.rho;
    const double ue = i < nx - 1 ? ge * up[c + 1] + (1.0 - ge) * up[c] : up[c];
    const double vn = j < ny - 1 ? gn * vp[c + nx] + (1.0 - gn) * vp[c] : vp[c];
    if (i == 0) fx[j * ldx] += rho * (up[c] * hy);
    fx[j * ldx + i + 1] += rho * (ue * hy);
    if (j == 0) fy[i] += rho * (vp[c] * hx);
    fy[(j + 1) * nx + i] += rho * (vn * hx);
  }
  double dvdx, dudy, unused;
  sg_gauss(s, d.v, nullptr, c, i, j, dvdx, unused);
  sg_gauss(s, d.u, d.ulid, c, i, j, unused, dudy);
  const double wc = dvdx - dudy;
  x.vec(FV_OMEGA)[c] = wc;
  w2 += (wc * wc) * s.V(i, j);
}

// ---- 7. twin of fv_cell_div_palinstrophy: div2 += (div mdot)^2, pal += |grad omega|^2 V (record sums 7 and 9).  The sums
//         of E, Z and P carry V already, so the record row takes V = 1
__device__ __forceinline__ void sg_cell_sums(const SgCtx& s, int c, double& div2, double& pal) {
  const FvCtx& x = s.x;
  const int nx = x.nx, ldx = x.ldx;
  const double *fx = x.fx, *fy = x.fy;
  const int i = c % nx, j = c / nx;
  const double dv = (fx[j * ldx + i + 1] - fx[j * ldx + i]) + (fy[(j + 1) * nx + i] - fy[j * nx + i]);
  div2 += dv * dv;
  double gx, gy;
  sg_gauss(s, x.vec(FV_OMEGA), nullptr, c, i, j, gx, gy);
  pal += (gx * gx + gy * gy) * s.V(i, j);
}
