// ldc_fv_prolong_tables.hip -- the state of a fine finite-volume trial from the state of a coarse one on tensor grids with
// ANY spacing per axis (include/ldc_fv.h, ldc_fv_prolong_tables_enqueue): coarse-to-fine sequencing and continuation in Re
// for wall-clustered trials.  A translation unit of its own, linked into libldc_hip.so beside the others: every other code
// object is the same with and without this file.
//
// What differs from ldc_fv_prolong_enqueue (equal spacing, csrc/ldc_fv_prolong.hip with ldc_fv_prolong_cells.inc):
//   - the nodes of the extended coarse axis are 0, the coarse centre table, L; the fine centres come from a table too;
//   - the left node of a fine centre is found by bisection (the axis is no longer equally spaced);
//   - mdot is formed by the face rule of the stretched kernels, rho (g u_N + (1 - g) u_P) |S| with g and |S| from the fine
//     trial's geometry table [h | d | g] of ldc_fv_set_grid.
// The ring values, the bilinear interpolant (x first), the pin of p at fine cell 0 and the exact zeros on the wall faces are
// those of the uniform transfer.  A job holds raw device pointers only, no handle: a uniform source has no tables on its
// handle, and one kernel serves every combination of grids.
//
// Mapping: ONE work-group of 512 threads per job, up to LDC_FV_PROLONG_TABLES_LAUNCH_MAX jobs per launch, the job structs
// travelling as kernel arguments; the work-groups are independent (no flags, no spins, nobody waits for anybody).
//   0. locate   one bisection per thread: (k, t) of the nx + ny <= 512 fine centres into LDS (6 KB)
//   1. cells    after the barrier: u, v, p at every fine cell; every thread forms the interpolated p at fine cell 0 for
//               itself, so the fine p[0] is exactly 0.0 and nothing is broadcast
//   2. faces    after the barrier: the two loops over the faces of mdot
// No reduction, no scratch in global memory.  The arithmetic is stated once, here, behind a pragma that keeps its
// multiply-adds apart, so that tests/fv_prolong_tables_numpy.py states it with the same roundings.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ldc_hip.h"
#include "ldc_fv_common.inc"

namespace {

struct FvPtLaunch {
  ldc_fv_prolong_tables_job jobs[LDC_FV_PROLONG_TABLES_LAUNCH_MAX];
};
static_assert(sizeof(ldc_fv_prolong_tables_job) == 152, "the job struct of include/ldc_fv.h");
static_assert(sizeof(FvPtLaunch) <= 3600, "kernel arguments");
static_assert(2 * LDC_FV_MAX_N <= kFvThreads, "locate: one thread per fine centre of either axis");

#pragma STDC FP_CONTRACT OFF      // (from here on no multiply-add is contracted: the transfer rounds as its NumPy statement)

// one axis of the extended coarse grid: nodes e_0 = 0, e_k = xc[k - 1] (k = 1 .. n), e_{n+1} = L
struct FvPtAxis {
  int n;
  const double* xc;
  double L;
  __device__ __forceinline__ double node(int k) const { return k == 0 ? 0.0 : (k == n + 1 ? L : xc[k - 1]); }
  // the left node of x (the largest k <= n with e_k <= x; 0 when there is none) and the weight inside its interval
  __device__ __forceinline__ void locate(double x, int& k, double& t) const {
    int lo = 0, hi = n + 1;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (node(mid) <= x) lo = mid; else hi = mid;
    }
    k = lo;
    const double e0 = node(lo), e1 = node(lo + 1);
    t = (x - e0) / (e1 - e0);
  }
};

enum FvPtRing { PT_RING_U, PT_RING_V, PT_RING_P };

// the extended coarse field at node (kx, ky), kx = 0 .. nx + 1, ky = 0 .. ny + 1: walls and corners 0, the lid the coarse
// lid profile, p repeats the nearest cell; no index leaves the coarse arrays
template <FvPtRing R>
__device__ __forceinline__ double pt_node(const double* f, const double* ulid, int nx, int ny, int kx, int ky) {
  if (R == PT_RING_P) {
    const int i = kx < 1 ? 0 : (kx > nx ? nx - 1 : kx - 1), j = ky < 1 ? 0 : (ky > ny ? ny - 1 : ky - 1);
    return f[j * nx + i];
  }
  const bool inx = kx >= 1 && kx <= nx, iny = ky >= 1 && ky <= ny;
  if (inx && iny) return f[(ky - 1) * nx + (kx - 1)];
  if (R == PT_RING_U && inx && ky == ny + 1) return ulid[kx - 1];
  return 0.0;
}

template <FvPtRing R>
__device__ __forceinline__ double pt_at(const double* f, const double* ulid, int nx, int ny, int kx, double tx, int ky,
                                        double ty) {
  const double a = pt_node<R>(f, ulid, nx, ny, kx, ky), b = pt_node<R>(f, ulid, nx, ny, kx + 1, ky);
  const double lo = a + tx * (b - a);
  const double a1 = pt_node<R>(f, ulid, nx, ny, kx, ky + 1), b1 = pt_node<R>(f, ulid, nx, ny, kx + 1, ky + 1);
  const double hi = a1 + tx * (b1 - a1);
  return lo + ty * (hi - lo);
}

__global__ __launch_bounds__(kFvThreads) void fv_prolong_tables_kernel(const FvPtLaunch L) {
  __shared__ int lk[2 * LDC_FV_MAX_N];          // [0, nx): the x axis; [nx, nx + ny): the y axis
  __shared__ double lt[2 * LDC_FV_MAX_N];
  const ldc_fv_prolong_tables_job& J = L.jobs[blockIdx.x];
  const int cnx = J.coarse_nx, cny = J.coarse_ny, nx = J.fine_nx, ny = J.fine_ny, n = nx * ny;
  const int tid = threadIdx.x;

  // ---- 0. (k, t) of every fine centre
  if (tid < nx + ny) {
    const bool xdir = tid < nx;
    const FvPtAxis ax = {xdir ? cnx : cny, xdir ? J.coarse_xc : J.coarse_yc, xdir ? J.Lx : J.Ly};
    const double x = xdir ? J.fine_xc[tid] : J.fine_yc[tid - nx];
    int k;
    double t;
    ax.locate(x, k, t);
    lk[tid] = k;
    lt[tid] = t;
  }
  __syncthreads();

  // ---- 1. u, v, p at the fine cell centres
  const double *cu = J.coarse_u, *cv = J.coarse_v, *cp = J.coarse_p, *ulid = J.coarse_ulid;
  const double p0 = pt_at<PT_RING_P>(cp, ulid, cnx, cny, lk[0], lt[0], lk[nx], lt[nx]);
  double *fu = J.fine_u, *fv = J.fine_v, *fp = J.fine_p;
  for (int cell = tid; cell < n; cell += kFvThreads) {
    const int i = cell % nx, j = cell / nx;
    const int kx = lk[i], ky = lk[nx + j];
    const double tx = lt[i], ty = lt[nx + j];
    fu[cell] = pt_at<PT_RING_U>(cu, ulid, cnx, cny, kx, tx, ky, ty);
    fv[cell] = pt_at<PT_RING_V>(cv, ulid, cnx, cny, kx, tx, ky, ty);
    fp[cell] = pt_at<PT_RING_P>(cp, ulid, cnx, cny, kx, tx, ky, ty) - p0;
  }
  __syncthreads();

  // ---- 2. mdot = [ fx | fy ] from the new u and v: rho ((g f_N + (1 - g) f_P) |S|) inside, exactly 0.0 on the walls
  const int nfx = ny * (nx + 1), nfy = (ny + 1) * nx;
  const double *hx = J.fine_x_grid, *hy = J.fine_y_grid;            // [h (n) | d (n + 1) | g (n + 1)]
  const double *gx = J.fine_x_grid + 2 * nx + 1, *gy = J.fine_y_grid + 2 * ny + 1;
  const double rho = J.rho;
  double *fx = J.fine_mdot, *fy = J.fine_mdot + nfx;
  for (int q = tid; q < nfx; q += kFvThreads) {
    const int i = q % (nx + 1), j = q / (nx + 1);
    double m = 0.0;
    if (i > 0 && i < nx) m = rho * ((gx[i] * fu[j * nx + i] + (1.0 - gx[i]) * fu[j * nx + i - 1]) * hy[j]);
    fx[q] = m;
  }
  for (int q = tid; q < nfy; q += kFvThreads) {
    const int i = q % nx, j = q / nx;
    double m = 0.0;
    if (j > 0 && j < ny) m = rho * ((gy[j] * fv[j * nx + i] + (1.0 - gy[j]) * fv[(j - 1) * nx + i]) * hx[i]);
    fy[q] = m;
  }
}

inline bool pt_size_ok(int n) { return n >= LDC_FV_MIN_N && n <= LDC_FV_MAX_N; }

}  // namespace

extern "C" {

int ldc_fv_prolong_tables_launches(int n) {
  if (n < 1) return LDC_E_ARG;
  return (n + LDC_FV_PROLONG_TABLES_LAUNCH_MAX - 1) / LDC_FV_PROLONG_TABLES_LAUNCH_MAX;
}

int ldc_fv_prolong_tables_enqueue(const struct ldc_fv_prolong_tables_job* jobs, int n, void* stream) {
  if (!jobs || n < 1) return LDC_E_ARG;
  for (int q = 0; q < n; ++q) {
    const ldc_fv_prolong_tables_job& j = jobs[q];
    const void* req[] = {j.coarse_u, j.coarse_v, j.coarse_p, j.coarse_ulid, j.coarse_xc, j.coarse_yc, j.fine_u, j.fine_v,
                         j.fine_p, j.fine_mdot, j.fine_x_grid, j.fine_y_grid, j.fine_xc, j.fine_yc};
    for (const void* x : req) if (!x) return LDC_E_ARG;
    if (!pt_size_ok(j.coarse_nx) || !pt_size_ok(j.coarse_ny) || !pt_size_ok(j.fine_nx) || !pt_size_ok(j.fine_ny)) return LDC_E_ARG;
    if (!(j.Lx > 0) || !(j.Ly > 0) || !(j.rho > 0)) return LDC_E_ARG;
  }
  // what a launch writes nobody else in it may read or write: its work-groups run in any order
  for (int q = 0; q < n; ++q) {
    const void* written[] = {jobs[q].fine_u, jobs[q].fine_v, jobs[q].fine_p, jobs[q].fine_mdot};
    for (int a = 0; a < 4; ++a) {
      for (int b = a + 1; b < 4; ++b) if (written[a] == written[b]) return LDC_E_ARG;
      for (int r = 0; r < n; ++r) {
        const void* read[] = {jobs[r].coarse_u, jobs[r].coarse_v, jobs[r].coarse_p};
        for (const void* x : read) if (written[a] == x) return LDC_E_ARG;
        if (r == q) continue;
        const void* theirs[] = {jobs[r].fine_u, jobs[r].fine_v, jobs[r].fine_p, jobs[r].fine_mdot};
        for (const void* x : theirs) if (written[a] == x) return LDC_E_ARG;
      }
    }
  }
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) return LDC_E_NODEVICE;
  for (int lo = 0; lo < n; lo += LDC_FV_PROLONG_TABLES_LAUNCH_MAX) {
    FvPtLaunch L;
    const int b = n - lo < LDC_FV_PROLONG_TABLES_LAUNCH_MAX ? n - lo : LDC_FV_PROLONG_TABLES_LAUNCH_MAX;
    for (int q = 0; q < LDC_FV_PROLONG_TABLES_LAUNCH_MAX; ++q) L.jobs[q] = jobs[lo + (q < b ? q : 0)];
    hipLaunchKernelGGL(fv_prolong_tables_kernel, dim3(b), dim3(kFvThreads), 0, as_stream(stream), L);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  return 0;
}

}  // extern "C"
