// ldc_fv_prolong.hip -- the state of a fine finite-volume trial from the state of a coarse one (include/ldc_fv.h,
// ldc_fv_prolong_enqueue): coarse-to-fine grid sequencing and continuation in Re.  A translation unit of its own, linked
// into libldc_hip.so beside ldc_kernels.hip and ldc_fv_post.hip: the code object of the solve kernels is the same with
// and without this file.
//
// Mapping: ONE work-group of 512 threads per (coarse, fine) pair; a launch of B pairs is B independent work-groups (no
// flags, no spins, nobody waits for anybody).  fv_prolong_kernel reads both descriptors and runs two phases:
//   1. fv_prolong_cells   u, v, p at every fine cell centre: the bilinear interpolant of the coarse field extended by a
//                         ring on the domain boundary (walls 0, the lid the coarse lid profile, p zero normal gradient);
//                         p minus its interpolated value at fine cell 0, which every thread recomputes for itself
//   2. fv_prolong_fluxes  after the barrier: mdot from the new u, v by the solver's face rule, wall faces exactly 0.0
// The kernel is memory-bound and tiny (a fine trial is at most 256 x 256 cells): plain loops over cells and faces, one
// element per thread and pass, no LDS, no reduction.  The arithmetic is the one tests/fv_prolong_numpy.py states; with
// contraction off it has no multiply-add that the compiler could fuse, so both round alike.
//
// ldc_fv_wide.hip holds COPIES of FvAxis, fv_prolong_node, fv_prolong_at and of the loop bodies of fv_prolong_cells and
// fv_prolong_fluxes (fv_wide_prolong_*: the same transfer for chip or shared trials, two launches per pair): a change to
// one goes into the other.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ldc_hip.h"
#include "ldc_fv_common.inc"

#pragma STDC FP_CONTRACT OFF

namespace {

struct FvProlongLaunch {
  const FvDesc* coarse[LDC_FV_PROLONG_LAUNCH_MAX];
  const FvDesc* fine[LDC_FV_PROLONG_LAUNCH_MAX];
};
static_assert(sizeof(FvProlongLaunch) <= 3600, "kernel arguments");

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

// the extended coarse field at node (kx, ky), kx = 0..nx+1, ky = 0..ny+1
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

// ---- 1. u, v, p at the fine cell centres
__device__ __forceinline__ void fv_prolong_cells(const FvDesc& c, const FvDesc& f) {
  const int nx = f.nx, n = f.nx * f.ny;
  const FvAxis ax = {c.nx, c.dx}, ay = {c.ny, c.dy};
  int kx0, ky0;
  double tx0, ty0;
  ax.locate((0 + 0.5) * f.dx, kx0, tx0);
  ay.locate((0 + 0.5) * f.dy, ky0, ty0);
  const double p0 = fv_prolong_at<FV_RING_P>(c, c.p, kx0, tx0, ky0, ty0);
  for (int cell = threadIdx.x; cell < n; cell += kFvThreads) {
    const int i = cell % nx, j = cell / nx;
    int kx, ky;
    double tx, ty;
    ax.locate((i + 0.5) * f.dx, kx, tx);
    ay.locate((j + 0.5) * f.dy, ky, ty);
    f.u[cell] = fv_prolong_at<FV_RING_U>(c, c.u, kx, tx, ky, ty);
    f.v[cell] = fv_prolong_at<FV_RING_V>(c, c.v, kx, tx, ky, ty);
    f.p[cell] = fv_prolong_at<FV_RING_P>(c, c.p, kx, tx, ky, ty) - p0;
  }
  __syncthreads();
}

// ---- 2. mdot = [ fx | fy ] from the new u and v: rho (1/2 f_N + 1/2 f_P) |S| inside, 0.0 on the walls
__device__ __forceinline__ void fv_prolong_fluxes(const FvDesc& f) {
  const int nx = f.nx, ny = f.ny;
  const int nfx = ny * (nx + 1), nfy = (ny + 1) * nx;
  double *fx = f.mdot, *fy = f.mdot + nfx;
  for (int q = threadIdx.x; q < nfx; q += kFvThreads) {
    const int i = q % (nx + 1), j = q / (nx + 1);
    double m = 0.0;
    if (i > 0 && i < nx) m = f.rho * (0.5 * f.u[j * nx + i] + (1.0 - 0.5) * f.u[j * nx + i - 1]) * f.dy;
    fx[q] = m;
  }
  for (int q = threadIdx.x; q < nfy; q += kFvThreads) {
    const int i = q % nx, j = q / nx;
    double m = 0.0;
    if (j > 0 && j < ny) m = f.rho * (0.5 * f.v[j * nx + i] + (1.0 - 0.5) * f.v[(j - 1) * nx + i]) * f.dx;
    fy[q] = m;
  }
}

__global__ __launch_bounds__(kFvThreads) void fv_prolong_kernel(const FvProlongLaunch L) {
  const FvDesc& c = *L.coarse[blockIdx.x];
  const FvDesc& f = *L.fine[blockIdx.x];
  fv_prolong_cells(c, f);
  fv_prolong_fluxes(f);
}

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

inline bool fv_size_ok(const ldc_fv* h) {
  return h->nx >= LDC_FV_MIN_N && h->nx <= LDC_FV_MAX_N && h->ny >= LDC_FV_MIN_N && h->ny <= LDC_FV_MAX_N;
}

// one domain: nx dx and ny dy of both trials agree (to the rounding of L / n; beyond it the kernel would extrapolate)
inline bool fv_same_extent(double a, double b) { return fabs(a - b) <= 1e-12 * fmax(fabs(a), fabs(b)); }
inline bool fv_same_domain(const ldc_fv* c, const ldc_fv* f) {
  return fv_same_extent(c->nx * c->dx, f->nx * f->dx) && fv_same_extent(c->ny * c->dy, f->ny * f->dy);
}

}  // namespace

extern "C" {

int ldc_fv_prolong_enqueue(ldc_fv* const* coarse, ldc_fv* const* fine, int n, void* stream) {
  if (!coarse || !fine || n < 1) return LDC_E_ARG;
  for (int q = 0; q < n; ++q) if (!coarse[q] || !fine[q]) return LDC_E_STATE;
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) return LDC_E_NODEVICE;
  for (int q = 0; q < n; ++q) {
    if (coarse[q]->device != dev || fine[q]->device != dev) return LDC_E_STATE;
    if (!fv_size_ok(coarse[q]) || !fv_size_ok(fine[q]) || !fv_same_domain(coarse[q], fine[q])) return LDC_E_ARG;
    // what a launch writes nobody else in it may read or write: its work-groups run in any order
    for (int r = 0; r < n; ++r)
      if (fine[q] == coarse[r] || (r != q && fine[q] == fine[r])) return LDC_E_ARG;
  }
  for (int lo = 0; lo < n; lo += LDC_FV_PROLONG_LAUNCH_MAX) {
    FvProlongLaunch L;
    const int b = n - lo < LDC_FV_PROLONG_LAUNCH_MAX ? n - lo : LDC_FV_PROLONG_LAUNCH_MAX;
    for (int q = 0; q < LDC_FV_PROLONG_LAUNCH_MAX; ++q) {
      L.coarse[q] = q < b ? coarse[lo + q]->dev : nullptr;
      L.fine[q] = q < b ? fine[lo + q]->dev : nullptr;
    }
    hipLaunchKernelGGL(fv_prolong_kernel, dim3(b), dim3(kFvThreads), 0, as_stream(stream), L);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  return 0;
}

}  // extern "C"
