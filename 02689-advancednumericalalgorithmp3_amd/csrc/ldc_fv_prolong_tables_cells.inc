// ldc_fv_prolong_tables_cells.inc -- the arithmetic of the coarse-to-fine transfer on tensor grids with any spacing per axis
// (include/ldc_fv.h, "The coarse-to-fine transfer on tensor grids"), stated ONCE for both mappings: the one-CU kernel of
// csrc/ldc_fv_prolong_tables.hip (one work-group per job) and the chip kernels of csrc/ldc_fv_wide_prolong_tables.hip (two
// launches over the whole chip per job) call these functions, so a pair gives the same bits through either.
//   FvPtAxis    the extended coarse axis 0, xc, L; the left node of a fine centre by bisection and its weight
//   pt_node     the extended coarse field at a node: the ring values
//   pt_at       the bilinear interpolant, x first
//   pt_xface    mdot at one x face: rho ((g f_N + (1 - g) f_P) |S|) inside, exactly +0.0 on the two walls
//   pt_yface    likewise at one y face
//   pt_jobs_ok  (host) what both entry points refuse before any launch
// No kernel.  Include it BEHIND `#pragma STDC FP_CONTRACT OFF`: no multiply-add of
// the transfer is contracted, so that tests/fv_prolong_tables_numpy.py states it with the same roundings.

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

// mdot at x face q of the fine trial (ny rows of nx + 1 faces) from its new u: gx the face weights, hy the row heights
__device__ __forceinline__ double pt_xface(const double* fu, const double* gx, const double* hy, double rho, int nx, int q) {
  const int i = q % (nx + 1), j = q / (nx + 1);
  double m = 0.0;
  if (i > 0 && i < nx) m = rho * ((gx[i] * fu[j * nx + i] + (1.0 - gx[i]) * fu[j * nx + i - 1]) * hy[j]);
  return m;
}

// mdot at y face q (ny + 1 rows of nx faces) from the new v: gy the face weights, hx the column widths
__device__ __forceinline__ double pt_yface(const double* fv, const double* gy, const double* hx, double rho, int nx, int ny,
                                           int q) {
  const int i = q % nx, j = q / nx;
  double m = 0.0;
  if (j > 0 && j < ny) m = rho * ((gy[j] * fv[j * nx + i] + (1.0 - gy[j]) * fv[(j - 1) * nx + i]) * hx[i]);
  return m;
}

// the jobs of one call: no null pointer, sizes LDC_FV_MIN_N .. max_n, Lx, Ly, rho > 0, and nothing the call writes read or
// written by another job of it (the work-groups of a launch run in any order; the rule holds across launches too)
inline bool pt_jobs_ok(const ldc_fv_prolong_tables_job* jobs, int n, int max_n) {
  for (int q = 0; q < n; ++q) {
    const ldc_fv_prolong_tables_job& j = jobs[q];
    const void* req[] = {j.coarse_u, j.coarse_v, j.coarse_p, j.coarse_ulid, j.coarse_xc, j.coarse_yc, j.fine_u, j.fine_v,
                         j.fine_p, j.fine_mdot, j.fine_x_grid, j.fine_y_grid, j.fine_xc, j.fine_yc};
    for (const void* x : req) if (!x) return false;
    for (int s : {j.coarse_nx, j.coarse_ny, j.fine_nx, j.fine_ny}) if (s < LDC_FV_MIN_N || s > max_n) return false;
    if (!(j.Lx > 0) || !(j.Ly > 0) || !(j.rho > 0)) return false;
  }
  for (int q = 0; q < n; ++q) {
    const void* written[] = {jobs[q].fine_u, jobs[q].fine_v, jobs[q].fine_p, jobs[q].fine_mdot};
    for (int a = 0; a < 4; ++a) {
      for (int b = a + 1; b < 4; ++b) if (written[a] == written[b]) return false;
      for (int r = 0; r < n; ++r) {
        const void* read[] = {jobs[r].coarse_u, jobs[r].coarse_v, jobs[r].coarse_p};
        for (const void* x : read) if (written[a] == x) return false;
        if (r == q) continue;
        const void* theirs[] = {jobs[r].fine_u, jobs[r].fine_v, jobs[r].fine_p, jobs[r].fine_mdot};
        for (const void* x : theirs) if (written[a] == x) return false;
      }
    }
  }
  return true;
}
