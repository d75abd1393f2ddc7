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
// No reduction, no scratch in global memory.  The arithmetic is stated once, in ldc_fv_prolong_tables_cells.inc (shared with
// the chip mapping's csrc/ldc_fv_wide_prolong_tables.hip), included behind a pragma that keeps its multiply-adds apart, so
// that tests/fv_prolong_tables_numpy.py states it with the same roundings.

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

#include "ldc_fv_prolong_tables_cells.inc"      // the arithmetic and the checks of a call: one definition for both mappings

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
  for (int q = tid; q < nfx; q += kFvThreads) fx[q] = pt_xface(fu, gx, hy, rho, nx, q);
  for (int q = tid; q < nfy; q += kFvThreads) fy[q] = pt_yface(fv, gy, hx, rho, nx, ny, q);
}

}  // namespace

extern "C" {

int ldc_fv_prolong_tables_launches(int n) {
  if (n < 1) return LDC_E_ARG;
  return (n + LDC_FV_PROLONG_TABLES_LAUNCH_MAX - 1) / LDC_FV_PROLONG_TABLES_LAUNCH_MAX;
}

int ldc_fv_prolong_tables_enqueue(const struct ldc_fv_prolong_tables_job* jobs, int n, void* stream) {
  if (!jobs || n < 1) return LDC_E_ARG;
  if (!pt_jobs_ok(jobs, n, LDC_FV_MAX_N)) return LDC_E_ARG;
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
