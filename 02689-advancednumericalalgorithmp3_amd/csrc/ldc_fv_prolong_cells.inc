// ldc_fv_prolong_cells.inc -- the arithmetic of the coarse-to-fine transfer of a finite-volume state (include/ldc_fv.h),
// written once for every mapping of a trial onto the card.  Included by ldc_fv_prolong.hip (one pair per work-group of
// 512 threads) and by ldc_fv_wide.hip (a pair of chip or shared trials, two launches); everything is in the anonymous
// namespace, so each unit compiles its own copy and neither code object depends on the other.
//
// The arithmetic is the one tests/fv_prolong_numpy.py states, and it rounds like it only with contraction OFF: this file
// sets no pragma of its own.  Each unit includes it BEHIND its `#pragma STDC FP_CONTRACT OFF`, which in ldc_fv_wide.hip
// stands at the start of the prolongation section, behind the SIMPLE chain, whose multiply-adds stay fused.
//
// What is here: one axis of the extended coarse grid (FvAxis), the extended coarse field at a node and its bilinear
// interpolant (fv_prolong_node, fv_prolong_at), the interpolated p at fine cell 0 (fv_prolong_p0), one fine cell of
// u, v, p (fv_prolong_cell), one x-face and one y-face of mdot (fv_prolong_xface, fv_prolong_yface), and the host's
// test that two trials cover one domain (fv_same_domain).
// What a mapping supplies: the loops over cells and faces, and the barrier or launch boundary between them.  It passes
// by value what its loop has hoisted (nx, ny, the axes, p0, fx, fy): a descriptor that lives in global memory would be
// read again after every store.
#ifndef LDC_FV_PROLONG_CELLS_INC
#define LDC_FV_PROLONG_CELLS_INC

#include <math.h>

#include "ldc_fv_common.inc"

namespace {

// one axis of the extended coarse grid: nodes e_0 = 0, e_k = (k - 1/2) h (k = 1..n), e_{n+1} = n h
struct FvAxis {
  int n;
  double h;
  __device__ __forceinline__ double node(int k) const { return k == 0 ? 0.0 : (k == n + 1 ? n * h : (k - 0.5) * h); }
  // the left node of x (the largest node <= x, at most n: the last interval) and the weight inside its interval
  __device__ __forceinline__ void locate(double x, int& k, double& t) const {
    k = (int)(x / h + 0.5);
    k = k < 0 ? 0 : (k > n ? n : k);
    while (k < n && node(k + 1) <= x) ++k;           // (the guess is off by one at most: rounding at a node)
    while (k > 0 && node(k) > x) --k;
    const double e0 = node(k), e1 = node(k + 1);
    t = (x - e0) / (e1 - e0);
  }
};

enum FvRing { FV_RING_U, FV_RING_V, FV_RING_P };

// the extended coarse field at node (kx, ky), kx = 0..nx+1, ky = 0..ny+1: walls 0, the lid the coarse lid profile, p
// zero normal gradient
template <FvRing R>
__device__ __forceinline__ double fv_prolong_node(const FvDesc& c, const double* f, int kx, int ky) {
  const int nx = c.nx, ny = c.ny;
  if (R == FV_RING_P) {
    const int i = kx < 1 ? 0 : (kx > nx ? nx - 1 : kx - 1), j = ky < 1 ? 0 : (ky > ny ? ny - 1 : ky - 1);
    return f[j * nx + i];
  }
  const bool inx = kx >= 1 && kx <= nx, iny = ky >= 1 && ky <= ny;
  if (inx && iny) return f[(ky - 1) * nx + (kx - 1)];
  if (R == FV_RING_U && inx && ky == ny + 1) return c.ulid[kx - 1];
  return 0.0;
}

template <FvRing R>
__device__ __forceinline__ double fv_prolong_at(const FvDesc& c, const double* f, int kx, double tx, int ky, double ty) {
  const double a = fv_prolong_node<R>(c, f, kx, ky), b = fv_prolong_node<R>(c, f, kx + 1, ky);
  const double lo = a + tx * (b - a);
  const double a1 = fv_prolong_node<R>(c, f, kx, ky + 1), b1 = fv_prolong_node<R>(c, f, kx + 1, ky + 1);
  const double hi = a1 + tx * (b1 - a1);
  return lo + ty * (hi - lo);
}

// the interpolated coarse p at the centre of fine cell 0: every thread computes it for itself, so the fine p[0] is
// exactly 0.0 and nothing is broadcast
__device__ __forceinline__ double fv_prolong_p0(const FvDesc& c, const FvDesc& f, FvAxis ax, FvAxis ay) {
  int kx0, ky0;
  double tx0, ty0;
  ax.locate((0 + 0.5) * f.dx, kx0, tx0);
  ay.locate((0 + 0.5) * f.dy, ky0, ty0);
  return fv_prolong_at<FV_RING_P>(c, c.p, kx0, tx0, ky0, ty0);
}

// u, v, p at the centre of fine cell `cell` (nx: the fine trial's)
__device__ __forceinline__ void fv_prolong_cell(const FvDesc& c, const FvDesc& f, FvAxis ax, FvAxis ay, int nx, double p0,
                                                int cell) {
  const int i = cell % nx, j = cell / nx;
  int kx, ky;
  double tx, ty;
  ax.locate((i + 0.5) * f.dx, kx, tx);
  ay.locate((j + 0.5) * f.dy, ky, ty);
  f.u[cell] = fv_prolong_at<FV_RING_U>(c, c.u, kx, tx, ky, ty);
  f.v[cell] = fv_prolong_at<FV_RING_V>(c, c.v, kx, tx, ky, ty);
  f.p[cell] = fv_prolong_at<FV_RING_P>(c, c.p, kx, tx, ky, ty) - p0;
}

// mdot of x-face q of ny x (nx + 1) and of y-face q of (ny + 1) x nx from the new u and v: rho (1/2 f_N + 1/2 f_P) |S|
// inside, exactly 0.0 on the walls
__device__ __forceinline__ void fv_prolong_xface(const FvDesc& f, int nx, double* fx, int q) {
  const int i = q % (nx + 1), j = q / (nx + 1);
  double m = 0.0;
  if (i > 0 && i < nx) m = f.rho * (0.5 * f.u[j * nx + i] + (1.0 - 0.5) * f.u[j * nx + i - 1]) * f.dy;
  fx[q] = m;
}
__device__ __forceinline__ void fv_prolong_yface(const FvDesc& f, int nx, int ny, double* fy, int q) {
  const int i = q % nx, j = q / nx;
  double m = 0.0;
  if (j > 0 && j < ny) m = f.rho * (0.5 * f.v[j * nx + i] + (1.0 - 0.5) * f.v[(j - 1) * nx + i]) * f.dx;
  fy[q] = m;
}

// host: one domain, nx dx and ny dy of both trials agree (to the rounding of L / n; beyond it the kernels would
// extrapolate).  T: anything with nx, ny, dx, dy (struct ldc_fv, FvDesc)
inline bool fv_same_extent(double a, double b) { return fabs(a - b) <= 1e-12 * fmax(fabs(a), fabs(b)); }
template <class T>
inline bool fv_same_domain(const T& c, const T& f) {
  return fv_same_extent(c.nx * c.dx, f.nx * f.dx) && fv_same_extent(c.ny * c.dy, f.ny * f.dy);
}

}  // namespace

#endif  // LDC_FV_PROLONG_CELLS_INC
