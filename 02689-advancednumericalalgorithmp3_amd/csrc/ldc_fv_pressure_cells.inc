// ldc_fv_pressure_cells.inc -- the per-cell arithmetic of the consistent pressure equation (include/ldc_fv.h), written once
// for every mapping: the work vectors of the solve, D and the face weight w_f, the row of A p and the corrected face
// fluxes with the vorticity.  Included by ldc_fv_wide.hip (ahead of ldc_fv_wide_pressure.inc: the chip and shared chain)
// and by ldc_fv_cu_pressure.hip (one work-group per trial); everything is a device function in the anonymous namespace,
// so each unit compiles its own copy and neither code object depends on the other.
//
//   (A x)_P = sum over the inner faces f of P of w_f (x_P - x_N),   w_f = rho (D_P / 2 + D_N / 2) |S_f| / d_f,
//   D_c = V / (a_P + 1e-14) from the unrelaxed diagonal, |S| / d = dy / dx on x faces and dx / dy on y faces.
// What a mapping supplies: the cell loop, the reductions, the barriers or launch boundaries, the CG scalars.
#ifndef LDC_FV_PRESSURE_CELLS_INC
#define LDC_FV_PRESSURE_CELLS_INC

#include "ldc_fv_cells.inc"

namespace {

// work vectors of the solve (all dead after the momentum solves): mdot* (3 n >= faces), r, z, p (the chip chain: two
// alternating copies), q; x is FV_Y
constexpr FvVec PCG_MS = FV_RU, PCG_R = FV_RTV, PCG_Z = FV_PU, PCG_P = FV_PV, PCG_Q = FV_VV;
static_assert(PCG_R == PCG_MS + 3 && PCG_Z == PCG_R + 1 && PCG_P == PCG_Z + 1 && PCG_Q == PCG_P + 2 && PCG_Q < FV_C,
              "the vectors of the pressure solve");
static_assert(3 * LDC_FV_MIN_N * LDC_FV_MIN_N >= LDC_FV_FACES(LDC_FV_MIN_N, LDC_FV_MIN_N), "mdot* in three work vectors");

__device__ __forceinline__ double wide_pcg_D(const FvCtx& x, int c) { return x.V / (x.w[FV_AP * x.n + c] + 1e-14); }

// the weight of an inner face between owner P (west / south) and neighbour N
__device__ __forceinline__ double wide_pcg_w(const FvCtx& x, double DP, double DN, bool xdir) {
  return (x.rho * (0.5 * DP + 0.5 * DN)) * (xdir ? x.dy / x.dx : x.dx / x.dy);
}

// (A p)_c of cell c = (i, j); pv(k): the value of p at cell k, pc = pv(c)
template <class PV>
__device__ __forceinline__ double wide_pcg_row(const FvCtx& x, int c, int i, int j, double pc, PV pv) {
  const int nx = x.nx, ny = x.ny;
  const double Dc = wide_pcg_D(x, c);
  double y = 0.0;
  if (i > 0) y += wide_pcg_w(x, wide_pcg_D(x, c - 1), Dc, true) * (pc - pv(c - 1));
  if (i < nx - 1) y += wide_pcg_w(x, Dc, wide_pcg_D(x, c + 1), true) * (pc - pv(c + 1));
  if (j > 0) y += wide_pcg_w(x, wide_pcg_D(x, c - nx), Dc, false) * (pc - pv(c - nx));
  if (j < ny - 1) y += wide_pcg_w(x, Dc, wide_pcg_D(x, c + nx), false) * (pc - pv(c + nx));
  return y;
}

// mdot = mdot* - w_f (p'_N - p'_P) on the east and north faces of cell c (and 0.0 on its wall faces), mdot* = [sx | sy]
// in the layout of mdot, pp = p' + const; then the vorticity with ghost cells, w2 += omega^2.  (The vorticity is a copy of
// the second half of fv_cell_flux_vorticity, ldc_fv_cells.inc, 6.: a change to one goes into the other.)
__device__ __forceinline__ void wide_pcg_cell_fluxvort(const FvCtx& x, int c, const double* pp, const double* sx,
                                                       const double* sy, double& w2) {
  const FvDesc& d = x.d;
  const int nx = x.nx, ny = x.ny, ldx = x.ldx;
  const double dx = x.dx, dy = x.dy;
  double *fx = x.fx, *fy = x.fy;
  const int i = c % nx, j = c / nx;
  const double Dc = wide_pcg_D(x, c);
  if (i == 0) fx[j * ldx] = 0.0;
  fx[j * ldx + i + 1] =
      i < nx - 1 ? sx[j * ldx + i + 1] - wide_pcg_w(x, Dc, wide_pcg_D(x, c + 1), true) * (pp[c + 1] - pp[c]) : 0.0;
  if (j == 0) fy[i] = 0.0;
  fy[(j + 1) * nx + i] =
      j < ny - 1 ? sy[(j + 1) * nx + i] - wide_pcg_w(x, Dc, wide_pcg_D(x, c + nx), false) * (pp[c + nx] - pp[c]) : 0.0;
  const double vE = i < nx - 1 ? d.v[c + 1] : -d.v[c], vW = i > 0 ? d.v[c - 1] : -d.v[c];
  const double uN = j < ny - 1 ? d.u[c + nx] : 2 * d.lid - d.u[c], uS = j > 0 ? d.u[c - nx] : -d.u[c];
  const double wc = (vE - vW) / (2 * dx) - (uN - uS) / (2 * dy);
  x.vec(FV_OMEGA)[c] = wc;
  w2 += wc * wc;
}

}  // namespace

#endif  // LDC_FV_PRESSURE_CELLS_INC
