// ldc_fv_wall_post_stretched.hip -- the wall-anchored streamfunction and sub-cell vortex centres of finite-volume trials on
// stretched tensor grids (include/ldc_fv.h, ldc_fv_wall_stretched_post_enqueue).  A translation unit of its own, linked into
// libldc_hip.so beside the others: every other code object is the same with and without this file.
//
// What differs from ldc_fv_wall_post_enqueue (equal spacing, csrc/ldc_fv_wall_post.hip):
//   - the geometry comes from the per-axis tables [h | d | g] of ldc_fv_set_grid, the centres and the eigenpairs from one
//     post table [xc | lam | Q] per axis;
//   - omega is the Gauss rule of the stretched kernels' record, (v_e - v_w) / hx - (u_n - u_s) / hy with g-weighted face
//     values, 0 on the walls and the lid profile on the lid; the same launch leaves B = V . omega in the second scratch field;
//   - psi solves (Hy (x) Kx^D + Ky^D (x) Hx) psi = B on ALL cells exactly with the generalised eigenpairs K^D q = lam H q,
//     Q^T H Q = I: psi = Qy ((Qy^T B Qx) / (lamy + lamx)) Qx^T, the four GEMMs of the uniform rule with cx = cy = 1;
//   - the refinement is the same six-term quadratic in physical coordinates with unequal distances to the neighbours.
//
// Mapping: that of ldc_fv_wall_post.hip and nothing new.  Seven launches per group of up to
// LDC_FV_WALL_STRETCHED_LAUNCH_MAX jobs --
//   omega, B | W1 = Qy^T B | W2 = W1 Qx / Lambda | W1 = Qy W2 | psi = W1 Qx^T | extrema | result
// -- the launch boundary the only barrier, nobody waits for anybody, no atomics.  blockIdx.y is the job, blockIdx.x the
// work-group within it (256 threads); the x extent of a launch is the largest count among its jobs and a work-group beyond
// its own job's count returns at once.  Every work-group of a sweep leaves its not-finite flag and its five (key, cell)
// candidates in its own slot of the job's scratch and `result` merges them by (larger key, then lower cell), so a job's psi,
// omega and block are the same bits whatever else is in the call.  The job structs travel as kernel arguments.
//
// The arithmetic of a GEMM tile, of the candidates, their scan and merge and of slots 0 .. 15 is NOT written here: they
// are the functions of ldc_fv_post_cells.inc.  omega, B and the refinement are written here, behind a pragma that keeps
// their multiply-adds apart, so that tests/fv_wall_stretched_numpy.py states them with the same roundings.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ldc_hip.h"
#include "ldc_fv_common.inc"
#include "ldc_fv_post_cells.inc"

namespace {

constexpr int kWsThreads = 256;
constexpr int kWsWaves = kWsThreads / 64;
constexpr int kWsSlot = 12;                 // doubles of a slot: 5 keys, 5 cells (as doubles), 2 not-finite flags
enum { WS_CELL = kFvPostBest, WS_BAD_OMEGA = 2 * kFvPostBest, WS_BAD_PSI };      // (the keys: FVP_* at 0 .. 4)
constexpr int kWsLaunches = 7;
static_assert(LDC_FV_WALL_SCRATCH_LEN(8, 8) == 2 * 64 + kWsSlot, "scratch layout");
static_assert(LDC_FV_WIDE_GROUPS(1024, 1024) <= kWsThreads, "result: one thread per slot");
static_assert(LDC_FV_WALL_RESULT_LEN == LDC_FV_POST_RESULT_LEN + 4 * LDC_FV_WALL_GROUP_LEN, "result block");

struct FvWsLaunch {
  ldc_fv_wall_stretched_job jobs[LDC_FV_WALL_STRETCHED_LAUNCH_MAX];
};
static_assert(sizeof(ldc_fv_wall_stretched_job) == 120, "the job struct of include/ldc_fv.h");
static_assert(sizeof(FvWsLaunch) < 4096, "kernel arguments");

__host__ __device__ inline int ws_groups(const ldc_fv_wall_stretched_job& J) { return (int)LDC_FV_WIDE_GROUPS(J.nx, J.ny); }
__host__ __device__ inline int ws_gemm_groups(const ldc_fv_wall_stretched_job& J) { return (int)LDC_FV_WIDE_GEMM_GROUPS(J.nx, J.ny); }
__device__ __forceinline__ double* ws_slots(const ldc_fv_wall_stretched_job& J) { return J.scratch + 2 * (J.nx * J.ny); }
// the pieces of the tables: [h (n) | d (n + 1) | g (n + 1)] and [xc (n) | lam (n) | Q (n x n)]
__device__ __forceinline__ const double* ws_d(const double* grid, int n) { return grid + n; }
__device__ __forceinline__ const double* ws_g(const double* grid, int n) { return grid + 2 * n + 1; }
__device__ __forceinline__ const double* ws_lam(const double* post, int n) { return post + n; }
__device__ __forceinline__ const double* ws_Q(const double* post, int n) { return post + 2 * n; }

#pragma STDC FP_CONTRACT OFF      // (from here on no multiply-add is contracted: omega, B and the refinement round as their NumPy statement)

// ---- 1. omega by the Gauss rule and B = V . omega into the second scratch field; slot: a value that is not finite
__global__ __launch_bounds__(kWsThreads) void fv_ws_omega(const FvWsLaunch L) {
  const ldc_fv_wall_stretched_job& J = L.jobs[blockIdx.y];
  const int g = blockIdx.x, G = ws_groups(J);
  if (g >= G) return;
  const int nx = J.nx, ny = J.ny, n = nx * ny;
  const double *u = J.u, *v = J.v;
  const double *hx = J.x_grid, *hy = J.y_grid, *gx = ws_g(J.x_grid, nx), *gy = ws_g(J.y_grid, ny);
  double* B = J.scratch + n;
  bool bad = false;
  for (int c = g * kWsThreads + threadIdx.x; c < n; c += G * kWsThreads) {
    const int i = c % nx, j = c / nx;
    const double vE = i < nx - 1 ? gx[i + 1] * v[c + 1] + (1.0 - gx[i + 1]) * v[c] : 0.0;
    const double vW = i > 0 ? gx[i] * v[c] + (1.0 - gx[i]) * v[c - 1] : 0.0;
    const double uN = j < ny - 1 ? gy[j + 1] * u[c + nx] + (1.0 - gy[j + 1]) * u[c] : J.ulid[i];
    const double uS = j > 0 ? gy[j] * u[c] + (1.0 - gy[j]) * u[c - nx] : 0.0;
    const double wc = (vE - vW) / hx[i] - (uN - uS) / hy[j];
    J.omega[c] = wc;
    B[c] = (hx[i] * hy[j]) * wc;
    bad |= !(fabs(wc) <= 1.7976931348623157e308);
  }
  const int any_bad = __syncthreads_or(bad ? 1 : 0);
  if (threadIdx.x == 0) ws_slots(J)[g * kWsSlot + WS_BAD_OMEGA] = any_bad ? 1.0 : 0.0;
}

// ---- 2. one GEMM of the fast diagonalisation, one tile per wave.  WHICH: 0 W1 = Qy^T B, 1 W2 = W1 Qx / Lambda,
// 2 W1 = Qy W2, 3 psi = W1 Qx^T; every matrix is ny x nx with leading dimension nx; B lies in W2 until launch 1 writes it
template <int WHICH>
__global__ __launch_bounds__(kWsThreads) void fv_ws_gemm(const FvWsLaunch L) {
  const ldc_fv_wall_stretched_job& J = L.jobs[blockIdx.y];
  const int nx = J.nx, ny = J.ny;
  const int t = blockIdx.x * kWsWaves + (threadIdx.x >> 6);
  if (t >= ((ny + 15) >> 4) * ((nx + 15) >> 4)) return;
  double *W1 = J.scratch, *W2 = J.scratch + nx * ny;
  const double *Qx = ws_Q(J.x_post, nx), *Qy = ws_Q(J.y_post, ny);
  if (WHICH == 0) fv_post_gemm_tile<false>(t, Qy, 1, ny, W2, nx, 1, W1, nx, ny, nx, ny, nullptr, nullptr, 0, 0);
  if (WHICH == 1) fv_post_gemm_tile<true>(t, W1, nx, 1, Qx, nx, 1, W2, nx, ny, nx, nx, ws_lam(J.x_post, nx), ws_lam(J.y_post, ny), 1.0, 1.0);
  if (WHICH == 2) fv_post_gemm_tile<false>(t, Qy, ny, 1, W2, nx, 1, W1, nx, ny, nx, ny, nullptr, nullptr, 0, 0);
  if (WHICH == 3) fv_post_gemm_tile<false>(t, W1, nx, 1, Qx, 1, nx, J.psi, nx, ny, nx, nx, nullptr, nullptr, 0, 0);
}

// ---- 3. the five extrema over this work-group's cells; slot: the winners and the not-finite flag of psi
__global__ __launch_bounds__(kWsThreads) void fv_ws_extrema(const FvWsLaunch L) {
  __shared__ double lkey[kWsWaves][kFvPostBest];
  __shared__ int lidx[kWsWaves][kFvPostBest];
  const ldc_fv_wall_stretched_job& J = L.jobs[blockIdx.y];
  const int g = blockIdx.x, G = ws_groups(J);
  if (g >= G) return;
  const int nx = J.nx, n = J.nx * J.ny;
  bool bad = false;
  FvBest best[kFvPostBest];
  fv_post_best_clear(best);
  for (int c = g * kWsThreads + threadIdx.x; c < n; c += G * kWsThreads)
    bad |= fv_post_cell_extrema(c, nx, J.psi, J.omega, J.ix_lt, J.ix_gt, J.jy_lt, J.jy_gt, best);
  fv_post_best_merge<kWsWaves>(best, lkey, lidx);
  const int any_bad = __syncthreads_or(bad ? 1 : 0);
  if (threadIdx.x == 0) {
    double* s = ws_slots(J) + g * kWsSlot;
#pragma unroll
    for (int q = 0; q < kFvPostBest; ++q) { s[q] = best[q].key; s[WS_CELL + q] = (double)best[q].idx; }
    s[WS_BAD_PSI] = any_bad ? 1.0 : 0.0;
  }
}

// f at cell (i, j) of the grid extended by odd reflection at the wall faces: the mirror cell's -f, +f across a corner; no
// index leaves [0, nx) x [0, ny) for i in -1 .. nx and j in -1 .. ny
__device__ __forceinline__ double fv_ws_reflected(const double* f, int nx, int ny, int i, int j) {
  double sign = 1.0;
  if (i < 0) { i = -1 - i; sign = -sign; }
  if (i >= nx) { i = 2 * nx - 1 - i; sign = -sign; }
  if (j < 0) { j = -1 - j; sign = -sign; }
  if (j >= ny) { j = 2 * ny - 1 - j; sign = -sign; }
  return sign * f[j * nx + i];
}

// the coefficients of the six-term quadratic through a 3 x 3 stencil with the distances dw, de, ds, dn to the neighbours
struct FvWsFit { double gx, gy, Hxx, Hyy, Hxy; };
__device__ __forceinline__ FvWsFit fv_ws_fit(double Cc, double W, double E, double S, double N, double SW, double SE,
                                             double NW, double NE, double dw, double de, double ds, double dn) {
  FvWsFit q;
  q.gx = (((E - Cc) * dw) / de + ((Cc - W) * de) / dw) / (dw + de);
  q.gy = (((N - Cc) * ds) / dn + ((Cc - S) * dn) / ds) / (ds + dn);
  q.Hxx = (2 * ((E - Cc) / de - (Cc - W) / dw)) / (dw + de);
  q.Hyy = (2 * ((N - Cc) / dn - (Cc - S) / ds)) / (ds + dn);
  q.Hxy = (((NE - NW) - SE) + SW) / ((dw + de) * (ds + dn));
  return q;
}

// One group of the result block: x, y, psi, omega, status, sx, sy, 0 for the extremum at `cell` (-1: none); `want_min`:
// the primary minimum (Hxx > 0), else a corner maximum (Hxx < 0); `none`: status 1 whatever the cell
__device__ void fv_ws_group(const ldc_fv_wall_stretched_job& J, int cell, bool want_min, bool none, double* r) {
  const int nx = J.nx, ny = J.ny;
  const double* psi = J.psi;
  const double* om = J.omega;
  const double *xc = J.x_post, *yc = J.y_post, *dxt = ws_d(J.x_grid, nx), *dyt = ws_d(J.y_grid, ny);
  const double eps = 2.220446049250313e-16;
  for (int q = 0; q < LDC_FV_WALL_GROUP_LEN; ++q) r[q] = 0.0;
  r[LDC_FV_WALL_STATUS] = J.refine ? 1.0 : -1.0;
  if (cell < 0) return;
  const int i = cell % nx, j = cell / nx;
  r[LDC_FV_WALL_X] = xc[i];
  r[LDC_FV_WALL_Y] = yc[j];
  r[LDC_FV_WALL_PSI] = psi[cell];
  r[LDC_FV_WALL_OMEGA] = om[cell];
  if (!J.refine || none) return;
  // distances to the neighbours' centres: d[k] lies between cells k-1 and k (k = 0 .. n); the mirror cell beyond a wall
  // lies at twice the wall's d
  const double dw = i > 0 ? dxt[i] : 2 * dxt[0], de = i < nx - 1 ? dxt[i + 1] : 2 * dxt[nx];
  const double ds = j > 0 ? dyt[j] : 2 * dyt[0], dn = j < ny - 1 ? dyt[j + 1] : 2 * dyt[ny];
  const double Cc = psi[cell];
  const double W = fv_ws_reflected(psi, nx, ny, i - 1, j), E = fv_ws_reflected(psi, nx, ny, i + 1, j);
  const double S = fv_ws_reflected(psi, nx, ny, i, j - 1), N = fv_ws_reflected(psi, nx, ny, i, j + 1);
  const double SW = fv_ws_reflected(psi, nx, ny, i - 1, j - 1), SE = fv_ws_reflected(psi, nx, ny, i + 1, j - 1);
  const double NW = fv_ws_reflected(psi, nx, ny, i - 1, j + 1), NE = fv_ws_reflected(psi, nx, ny, i + 1, j + 1);
  const FvWsFit f = fv_ws_fit(Cc, W, E, S, N, SW, SE, NW, NE, dw, de, ds, dn);
  const double gx = f.gx, gy = f.gy, Hxx = f.Hxx, Hyy = f.Hyy, Hxy = f.Hxy;
  const double det = Hxx * Hyy - Hxy * Hxy;
  const double Fxx = (4 * eps) * ((2 * ((fabs(E) + fabs(Cc)) / de + (fabs(Cc) + fabs(W)) / dw)) / (dw + de));
  const double Fyy = (4 * eps) * ((2 * ((fabs(N) + fabs(Cc)) / dn + (fabs(Cc) + fabs(S)) / ds)) / (ds + dn));
  const double Fxy = (4 * eps) * ((((fabs(NE) + fabs(NW)) + fabs(SE)) + fabs(SW)) / ((dw + de) * (ds + dn)));
  const bool definite = fabs(Hxx) > Fxx && fabs(Hyy) > Fyy &&
                        det > (Fxx * fabs(Hyy) + Fyy * fabs(Hxx)) + 2 * Fxy * fabs(Hxy) && (want_min ? Hxx > 0 : Hxx < 0);
  if (!definite) { r[LDC_FV_WALL_STATUS] = 2.0; return; }
  const double sx = -(Hyy * gx - Hxy * gy) / det, sy = -(Hxx * gy - Hxy * gx) / det;
  const double x = xc[i] + sx, y = yc[j] + sy;
  const double Lx = xc[nx - 1] + dxt[nx], Ly = yc[ny - 1] + dyt[ny];
  const double big = 1.7976931348623157e308;
  if (!(sx >= -dw && sx <= de) || !(sy >= -ds && sy <= dn) || !(x >= 0.0 && x <= Lx) || !(y >= 0.0 && y <= Ly)) {
    r[LDC_FV_WALL_STATUS] = 3.0;
    return;
  }
  const double ps = Cc + 0.5 * (gx * sx + gy * sy);
  double w = om[cell];
  if (i > 0 && i < nx - 1 && j > 0 && j < ny - 1) {      // the same six-term quadratic of omega, off the ring only
    const double wC = om[cell];
    const FvWsFit a = fv_ws_fit(wC, om[cell - 1], om[cell + 1], om[cell - nx], om[cell + nx], om[cell - nx - 1],
                                om[cell - nx + 1], om[cell + nx - 1], om[cell + nx + 1], dw, de, ds, dn);
    w = ((((wC + a.gx * sx) + a.gy * sy) + ((0.5 * a.Hxx) * sx) * sx) + ((0.5 * a.Hyy) * sy) * sy) + (a.Hxy * sx) * sy;
  }
  if (!(fabs(ps) <= big) || !(fabs(w) <= big)) { r[LDC_FV_WALL_STATUS] = 3.0; return; }
  r[LDC_FV_WALL_X] = x;
  r[LDC_FV_WALL_Y] = y;
  r[LDC_FV_WALL_PSI] = ps;
  r[LDC_FV_WALL_OMEGA] = w;
  r[LDC_FV_WALL_STATUS] = 0.0;
  r[LDC_FV_WALL_SX] = sx < 0 ? sx / dw : sx / de;
  r[LDC_FV_WALL_SY] = sy < 0 ? sy / ds : sy / dn;
}

// ---- 4. result (one work-group per job): thread t takes slot t, the same merge, the LDC_FV_POST_* slots, the groups
__global__ __launch_bounds__(kWsThreads) void fv_ws_result(const FvWsLaunch L) {
  __shared__ double lkey[kWsWaves][kFvPostBest];
  __shared__ int lidx[kWsWaves][kFvPostBest];
  const ldc_fv_wall_stretched_job& J = L.jobs[blockIdx.y];
  const int G = ws_groups(J), n = J.nx * J.ny;
  const bool mine = (int)threadIdx.x < G;
  const double* s = ws_slots(J) + (mine ? (int)threadIdx.x : 0) * kWsSlot;
  FvBest best[kFvPostBest];
#pragma unroll
  for (int q = 0; q < kFvPostBest; ++q) {
    best[q].key = mine ? s[q] : -HUGE_VAL;
    best[q].idx = mine ? (int)s[WS_CELL + q] : kFvPostNone;
  }
  const bool bad = mine && (s[WS_BAD_OMEGA] != 0.0 || s[WS_BAD_PSI] != 0.0);
  fv_post_best_merge<kWsWaves>(best, lkey, lidx);
  const int any_bad = __syncthreads_or(bad ? 1 : 0);
  if (threadIdx.x != 0) return;
  double* r = J.result;
  fv_post_result(n, J.psi, J.omega, best, any_bad, r);
  const bool flagged = r[LDC_FV_POST_NONFINITE] != 0.0;
  fv_ws_group(J, (int)r[LDC_FV_POST_PSI_MIN_CELL], true, flagged, r + LDC_FV_POST_RESULT_LEN);
  for (int q = 0; q < 3; ++q) {
    const bool none = flagged || !(r[LDC_FV_POST_PSI_BR + q] > 0.0);
    fv_ws_group(J, (int)r[LDC_FV_POST_PSI_BR_CELL + q], false, none,
                r + LDC_FV_POST_RESULT_LEN + (1 + q) * LDC_FV_WALL_GROUP_LEN);
  }
}

template <typename K>
inline int ws_launch(K kernel, int groups, int jobs, hipStream_t st, const FvWsLaunch& L) {
  hipLaunchKernelGGL(kernel, dim3(groups, jobs), dim3(kWsThreads), 0, st, L);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

}  // namespace

extern "C" {

int ldc_fv_wall_stretched_post_launches(int n) {
  if (n < 1) return LDC_E_ARG;
  return kWsLaunches * ((n + LDC_FV_WALL_STRETCHED_LAUNCH_MAX - 1) / LDC_FV_WALL_STRETCHED_LAUNCH_MAX);
}

int ldc_fv_wall_stretched_post_enqueue(const struct ldc_fv_wall_stretched_job* jobs, int n, void* stream) {
  if (!jobs || n < 1) return LDC_E_ARG;
  for (int q = 0; q < n; ++q) {
    const ldc_fv_wall_stretched_job& j = jobs[q];
    const void* req[] = {j.u, j.v, j.ulid, j.x_grid, j.y_grid, j.x_post, j.y_post, j.psi, j.omega, j.scratch, j.result};
    for (const void* x : req) if (!x) return LDC_E_ARG;
    if (j.nx < LDC_FV_MIN_N || j.nx > LDC_FV_WIDE_MAX_N || j.ny < LDC_FV_MIN_N || j.ny > LDC_FV_WIDE_MAX_N) return LDC_E_ARG;
    if (j.ix_lt < 0 || j.ix_lt > j.nx || j.ix_gt < 0 || j.ix_gt > j.nx) return LDC_E_ARG;
    if (j.jy_lt < 0 || j.jy_lt > j.ny || j.jy_gt < 0 || j.jy_gt > j.ny) return LDC_E_ARG;
    if (j.refine != 0 && j.refine != 1) return LDC_E_ARG;
  }
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) return LDC_E_NODEVICE;
  hipStream_t st = as_stream(stream);
  for (int lo = 0; lo < n; lo += LDC_FV_WALL_STRETCHED_LAUNCH_MAX) {
    FvWsLaunch L;
    const int b = n - lo < LDC_FV_WALL_STRETCHED_LAUNCH_MAX ? n - lo : LDC_FV_WALL_STRETCHED_LAUNCH_MAX;
    int G = 1, gg = 1;
    for (int q = 0; q < LDC_FV_WALL_STRETCHED_LAUNCH_MAX; ++q) {
      L.jobs[q] = jobs[lo + (q < b ? q : 0)];
      if (q < b && ws_groups(L.jobs[q]) > G) G = ws_groups(L.jobs[q]);
      if (q < b && ws_gemm_groups(L.jobs[q]) > gg) gg = ws_gemm_groups(L.jobs[q]);
    }
    int e = ws_launch(fv_ws_omega, G, b, st, L);
    if (!e) e = ws_launch(fv_ws_gemm<0>, gg, b, st, L);
    if (!e) e = ws_launch(fv_ws_gemm<1>, gg, b, st, L);
    if (!e) e = ws_launch(fv_ws_gemm<2>, gg, b, st, L);
    if (!e) e = ws_launch(fv_ws_gemm<3>, gg, b, st, L);
    if (!e) e = ws_launch(fv_ws_extrema, G, b, st, L);
    if (!e) e = ws_launch(fv_ws_result, 1, b, st, L);
    if (e) return e;
  }
  return 0;
}

}  // extern "C"
