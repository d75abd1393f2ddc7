// ldc_fv_wide_prolong_tables.hip -- the coarse-to-fine transfer on tensor grids with any spacing per axis, over the whole chip
// (include/ldc_fv.h, ldc_fv_wide_prolong_tables_enqueue): what ldc_fv_prolong_tables_enqueue does for trials of up to
// LDC_FV_MAX_N cells per axis, for LDC_FV_MIN_N .. LDC_FV_WIDE_MAX_N cells on either side, so that a stretched chip trial can
// be sequenced, continued in Re and started from a coarser one.  A translation unit of its own, linked into libldc_hip.so
// beside the others: every other code object is the same with and without this file.
//
// The arithmetic is that of csrc/ldc_fv_prolong_tables.hip, operation for operation: both units call the functions of
// ldc_fv_prolong_tables_cells.inc behind the same pragma, so a pair that both serve gets the same bits from either.  The job
// is that unit's struct (raw device pointers, no handle: a source of any mapping or grid serves), and so are the checks.
//
// Mapping, by the chip mapping's rules (csrc/ldc_fv_wide.hip): two launches per job, one per phase, in a grid that depends on
// the FINE (nx, ny) alone; the launch boundary is the only barrier between work-groups, and no work-group reads what another
// of the same launch writes.  No scratch in global memory, no atomics, no waits.  The jobs of a call are launched one after
// another, each job travelling by value in the kernel arguments.
//   1. cells    LDC_FV_WIDE_GROUPS(fine) work-groups of 256 threads.  Every work-group first fills ITS LDS with (k, t) of
//               all nx + ny fine centres (at most 2048 entries, 24 KB: eight bisections per thread at 1024 + 1024) -- the
//               bisections are recomputed per work-group, nothing is handed over -- and after one work-group barrier strides
//               over the fine cells: u, v, p, every thread forming the interpolated p at fine cell 0 for itself, so the fine
//               p[0] is exactly 0.0 and nothing is broadcast
//   2. faces    behind the launch boundary, the same grid: strides over the x faces, then the y faces of mdot
// (k, t) of a centre does not depend on who computes it, so a job's result does not depend on the grouping or on the other
// jobs of the call, bit for bit.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ldc_hip.h"
#include "ldc_fv_common.inc"

namespace {

constexpr int kPtThreads = 256;               // threads of a work-group: the chip mapping's
constexpr int kPtCentres = 2 * LDC_FV_WIDE_MAX_N;      // entries of the LDS table: the fine centres of both axes
static_assert(sizeof(ldc_fv_prolong_tables_job) == 152, "the job struct of include/ldc_fv.h");
static_assert(kPtCentres * (sizeof(int) + sizeof(double)) <= 24 * 1024, "the LDS table of `cells`");

#pragma STDC FP_CONTRACT OFF      // (from here on no multiply-add is contracted: the transfer rounds as its NumPy statement)

#include "ldc_fv_prolong_tables_cells.inc"

// ---- 1. u, v, p at the fine cell centres
__global__ __launch_bounds__(kPtThreads) void fv_wide_prolong_tables_cells(const ldc_fv_prolong_tables_job J, const int G) {
  __shared__ int lk[kPtCentres];                // [0, nx): the x axis; [nx, nx + ny): the y axis
  __shared__ double lt[kPtCentres];
  const int cnx = J.coarse_nx, cny = J.coarse_ny, nx = J.fine_nx, ny = J.fine_ny, n = nx * ny;
  const int tid = threadIdx.x;
  for (int c = tid; c < nx + ny; c += kPtThreads) {
    const bool xdir = c < nx;
    const FvPtAxis ax = {xdir ? cnx : cny, xdir ? J.coarse_xc : J.coarse_yc, xdir ? J.Lx : J.Ly};
    const double x = xdir ? J.fine_xc[c] : J.fine_yc[c - nx];
    int k;
    double t;
    ax.locate(x, k, t);
    lk[c] = k;
    lt[c] = t;
  }
  __syncthreads();

  const double *cu = J.coarse_u, *cv = J.coarse_v, *cp = J.coarse_p, *ulid = J.coarse_ulid;
  const double p0 = pt_at<PT_RING_P>(cp, ulid, cnx, cny, lk[0], lt[0], lk[nx], lt[nx]);
  double *fu = J.fine_u, *fv = J.fine_v, *fp = J.fine_p;
  for (int cell = blockIdx.x * kPtThreads + tid; cell < n; cell += G * kPtThreads) {
    const int i = cell % nx, j = cell / nx;
    const int kx = lk[i], ky = lk[nx + j];
    const double tx = lt[i], ty = lt[nx + j];
    fu[cell] = pt_at<PT_RING_U>(cu, ulid, cnx, cny, kx, tx, ky, ty);
    fv[cell] = pt_at<PT_RING_V>(cv, ulid, cnx, cny, kx, tx, ky, ty);
    fp[cell] = pt_at<PT_RING_P>(cp, ulid, cnx, cny, kx, tx, ky, ty) - p0;
  }
}

// ---- 2. mdot = [ fx | fy ] from the new u and v: rho ((g f_N + (1 - g) f_P) |S|) inside, exactly 0.0 on the walls
__global__ __launch_bounds__(kPtThreads) void fv_wide_prolong_tables_faces(const ldc_fv_prolong_tables_job J, const int G) {
  const int nx = J.fine_nx, ny = J.fine_ny;
  const int nfx = ny * (nx + 1), nfy = (ny + 1) * nx;
  const double *hx = J.fine_x_grid, *hy = J.fine_y_grid;            // [h (n) | d (n + 1) | g (n + 1)]
  const double *gx = J.fine_x_grid + 2 * nx + 1, *gy = J.fine_y_grid + 2 * ny + 1;
  const double rho = J.rho;
  const double *fu = J.fine_u, *fv = J.fine_v;
  double *fx = J.fine_mdot, *fy = J.fine_mdot + nfx;
  for (int q = blockIdx.x * kPtThreads + threadIdx.x; q < nfx; q += G * kPtThreads) fx[q] = pt_xface(fu, gx, hy, rho, nx, q);
  for (int q = blockIdx.x * kPtThreads + threadIdx.x; q < nfy; q += G * kPtThreads) fy[q] = pt_yface(fv, gy, hx, rho, nx, ny, q);
}

}  // namespace

extern "C" {

int ldc_fv_wide_prolong_tables_launches(int n) {
  if (n < 1) return LDC_E_ARG;
  return LDC_FV_WIDE_PROLONG_TABLES_LAUNCHES * n;
}

int ldc_fv_wide_prolong_tables_enqueue(const struct ldc_fv_prolong_tables_job* jobs, int n, void* stream) {
  if (!jobs || n < 1) return LDC_E_ARG;
  if (!pt_jobs_ok(jobs, n, LDC_FV_WIDE_MAX_N)) return LDC_E_ARG;
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) return LDC_E_NODEVICE;
  for (int q = 0; q < n; ++q) {
    const int G = (int)LDC_FV_WIDE_GROUPS(jobs[q].fine_nx, jobs[q].fine_ny);
    hipLaunchKernelGGL(fv_wide_prolong_tables_cells, dim3(G), dim3(kPtThreads), 0, as_stream(stream), jobs[q], G);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(fv_wide_prolong_tables_faces, dim3(G), dim3(kPtThreads), 0, as_stream(stream), jobs[q], G);
    e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  return 0;
}

}  // extern "C"
