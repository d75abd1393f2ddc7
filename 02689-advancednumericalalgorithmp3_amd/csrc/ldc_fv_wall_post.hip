// ldc_fv_wall_post.hip -- the wall-anchored streamfunction and sub-cell vortex centres of finite-volume trials on the
// device (include/ldc_fv.h, ldc_fv_wall_post_enqueue).  A translation unit of its own, linked into libldc_hip.so beside
// the others: every other code object is the same with and without this file.
//
// What differs from ldc_fv_post_enqueue (the reference's rule, csrc/ldc_fv_post.hip):
//   - omega's ghost above the top row is 2 ulid[i] - u, the lid PROFILE, and nothing writes psi in that phase;
//   - psi solves (cx Tx + cy Ty) psi = omega on ALL nx x ny cells, T = tridiag(-1, 2, -1) with 3 in both corners (the
//     ghost is -psi: psi = 0 on the wall FACE, not at the centres of the boundary ring), exactly, by fast diagonalisation
//     with the half-sample sine vectors C that the caller supplies: psi = Cy ((Cy^T Omega Cx) / (cy lamy + cx lamx)) Cx^T;
//   - behind the LDC_FV_POST_* slots the result block carries four groups (primary minimum, BR, BL, TL) with the extremum
//     of the quadratic through the 3 x 3 cells around the winner (refine = 1) or the cell's own values (refine = 0).
//
// Mapping: the chip chain's rules.  Seven launches per group of up to LDC_FV_WALL_LAUNCH_MAX jobs --
//   omega | W1 = Cy^T Omega | W2 = W1 Cx / Lambda | W1 = Cy W2 | psi = W1 Cx^T | extrema | result
// -- the launch boundary the only barrier, nobody waits for anybody, no atomics.  blockIdx.y is the job, blockIdx.x the
// work-group within it (256 threads, four waves); the x extent of a launch is the largest count among its jobs and a
// work-group beyond its own job's count returns at once.  Per job the counts depend on (nx, ny) alone: LDC_FV_WIDE_GROUPS
// for the cell sweeps (grid-stride by the JOB's count), one wave per 16 x 16 tile and four tiles per work-group for a
// GEMM, one work-group for `result`.  Every work-group of a sweep leaves its not-finite flag and its five (key, cell)
// candidates in its own slot of the job's scratch and `result` merges them by (larger key, then lower cell), so a job's
// psi, omega and block are the same bits whatever else is in the call.  The job structs travel as kernel arguments.
//
// The arithmetic of a GEMM tile, of the candidates, their scan and merge and of slots 0 .. 15 is NOT written here: they
// are the functions of ldc_fv_post_cells.inc.  The refinement is written here, behind a pragma that keeps its
// multiply-adds apart, so that tests/fv_wall_post_numpy.py states it with the same roundings.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ldc_hip.h"
#include "ldc_fv_common.inc"
#include "ldc_fv_post_cells.inc"

namespace {

constexpr int kWallThreads = 256;
constexpr int kWallWaves = kWallThreads / 64;
constexpr int kWallSlot = 12;               // doubles of a slot: 5 keys, 5 cells (as doubles), 2 not-finite flags
enum { WS_CELL = kFvPostBest, WS_BAD_OMEGA = 2 * kFvPostBest, WS_BAD_PSI };      // (the keys: FVP_* at 0 .. 4)
constexpr int kWallLaunches = 7;
static_assert(LDC_FV_WALL_SCRATCH_LEN(8, 8) == 2 * 64 + kWallSlot, "scratch layout");
static_assert(LDC_FV_WIDE_GROUPS(1024, 1024) <= kWallThreads, "result: one thread per slot");
static_assert(LDC_FV_WALL_RESULT_LEN == LDC_FV_POST_RESULT_LEN + 4 * LDC_FV_WALL_GROUP_LEN, "result block");

struct FvWallLaunch {
  ldc_fv_wall_job jobs[LDC_FV_WALL_LAUNCH_MAX];
};
static_assert(sizeof(ldc_fv_wall_job) == 136, "the job struct of include/ldc_fv.h");
static_assert(sizeof(FvWallLaunch) < 4096, "kernel arguments");

__host__ __device__ inline int wall_groups(const ldc_fv_wall_job& J) { return (int)LDC_FV_WIDE_GROUPS(J.nx, J.ny); }
__host__ __device__ inline int wall_gemm_groups(const ldc_fv_wall_job& J) { return (int)LDC_FV_WIDE_GEMM_GROUPS(J.nx, J.ny); }
__device__ __forceinline__ double* wall_slots(const ldc_fv_wall_job& J) { return J.scratch + 2 * (J.nx * J.ny); }

// ---- 1. omega with ghost cells: -f at the walls, 2 ulid[i] - u above the top row; slot: a value that is not finite
__global__ __launch_bounds__(kWallThreads) void fv_wall_omega(const FvWallLaunch L) {
  const ldc_fv_wall_job& J = L.jobs[blockIdx.y];
  const int g = blockIdx.x, G = wall_groups(J);
  if (g >= G) return;
  const int nx = J.nx, ny = J.ny, n = nx * ny;
  const double dx = J.dx, dy = J.dy;
  const double *u = J.u, *v = J.v;
  bool bad = false;
  for (int c = g * kWallThreads + threadIdx.x; c < n; c += G * kWallThreads) {
    const int i = c % nx, j = c / nx;
    const double vE = i < nx - 1 ? v[c + 1] : -v[c], vW = i > 0 ? v[c - 1] : -v[c];
    const double uN = j < ny - 1 ? u[c + nx] : 2 * J.ulid[i] - u[c], uS = j > 0 ? u[c - nx] : -u[c];
    const double wc = (vE - vW) / (2 * dx) - (uN - uS) / (2 * dy);
    J.omega[c] = wc;
    bad |= !(fabs(wc) <= 1.7976931348623157e308);
  }
  const int any_bad = __syncthreads_or(bad ? 1 : 0);
  if (threadIdx.x == 0) wall_slots(J)[g * kWallSlot + WS_BAD_OMEGA] = any_bad ? 1.0 : 0.0;
}

// ---- 2. one GEMM of the fast diagonalisation, one tile per wave.  WHICH: 0 W1 = Cy^T Omega, 1 W2 = W1 Cx / Lambda,
// 2 W1 = Cy W2, 3 psi = W1 Cx^T; every matrix is ny x nx with leading dimension nx
template <int WHICH>
__global__ __launch_bounds__(kWallThreads) void fv_wall_gemm(const FvWallLaunch L) {
  const ldc_fv_wall_job& J = L.jobs[blockIdx.y];
  const int nx = J.nx, ny = J.ny;
  const int t = blockIdx.x * kWallWaves + (threadIdx.x >> 6);
  if (t >= ((ny + 15) >> 4) * ((nx + 15) >> 4)) return;
  double *W1 = J.scratch, *W2 = J.scratch + nx * ny;
  const double cx = 1.0 / (J.dx * J.dx), cy = 1.0 / (J.dy * J.dy);
  if (WHICH == 0) fv_post_gemm_tile<false>(t, J.Cy, 1, ny, J.omega, nx, 1, W1, nx, ny, nx, ny, nullptr, nullptr, 0, 0);
  if (WHICH == 1) fv_post_gemm_tile<true>(t, W1, nx, 1, J.Cx, nx, 1, W2, nx, ny, nx, nx, J.lamx, J.lamy, cx, cy);
  if (WHICH == 2) fv_post_gemm_tile<false>(t, J.Cy, ny, 1, W2, nx, 1, W1, nx, ny, nx, ny, nullptr, nullptr, 0, 0);
  if (WHICH == 3) fv_post_gemm_tile<false>(t, W1, nx, 1, J.Cx, 1, nx, J.psi, nx, ny, nx, nx, nullptr, nullptr, 0, 0);
}

// ---- 3. the five extrema over this work-group's cells; slot: the winners and the not-finite flag of psi
__global__ __launch_bounds__(kWallThreads) void fv_wall_extrema(const FvWallLaunch L) {
  __shared__ double lkey[kWallWaves][kFvPostBest];
  __shared__ int lidx[kWallWaves][kFvPostBest];
  const ldc_fv_wall_job& J = L.jobs[blockIdx.y];
  const int g = blockIdx.x, G = wall_groups(J);
  if (g >= G) return;
  const int nx = J.nx, n = J.nx * J.ny;
  bool bad = false;
  FvBest best[kFvPostBest];
  fv_post_best_clear(best);
  for (int c = g * kWallThreads + threadIdx.x; c < n; c += G * kWallThreads)
    bad |= fv_post_cell_extrema(c, nx, J.psi, J.omega, J.ix_lt, J.ix_gt, J.jy_lt, J.jy_gt, best);
  fv_post_best_merge<kWallWaves>(best, lkey, lidx);
  const int any_bad = __syncthreads_or(bad ? 1 : 0);
  if (threadIdx.x == 0) {
    double* s = wall_slots(J) + g * kWallSlot;
#pragma unroll
    for (int q = 0; q < kFvPostBest; ++q) { s[q] = best[q].key; s[WS_CELL + q] = (double)best[q].idx; }
    s[WS_BAD_PSI] = any_bad ? 1.0 : 0.0;
  }
}

#pragma STDC FP_CONTRACT OFF      // (from here on no multiply-add is contracted: the refinement rounds as its NumPy statement)

// psi at cell (i, j) of the grid extended by odd reflection at the wall faces: the mirror cell's -psi, +psi across a corner
__device__ __forceinline__ double fv_wall_reflected(const double* psi, int nx, int ny, int i, int j) {
  double sign = 1.0;
  if (i < 0) { i = -1 - i; sign = -sign; }
  if (i >= nx) { i = 2 * nx - 1 - i; sign = -sign; }
  if (j < 0) { j = -1 - j; sign = -sign; }
  if (j >= ny) { j = 2 * ny - 1 - j; sign = -sign; }
  return sign * psi[j * nx + i];
}

// One group of the result block: x, y, psi, omega, status, sx, sy, 0 for the extremum at `cell` (-1: none); `want_min`:
// the primary minimum (Hxx > 0), else a corner maximum (Hxx < 0); `none`: status 1 whatever the cell
__device__ void fv_wall_group(const ldc_fv_wall_job& J, int cell, bool want_min, bool none, double* r) {
  const int nx = J.nx, ny = J.ny;
  const double* psi = J.psi;
  const double* om = J.omega;
  const double eps = 2.220446049250313e-16;
  for (int q = 0; q < LDC_FV_WALL_GROUP_LEN; ++q) r[q] = 0.0;
  r[LDC_FV_WALL_STATUS] = J.refine ? 1.0 : -1.0;
  if (cell < 0) return;
  const int i = cell % nx, j = cell / nx;
  r[LDC_FV_WALL_X] = (i + 0.5) * J.dx;
  r[LDC_FV_WALL_Y] = (j + 0.5) * J.dy;
  r[LDC_FV_WALL_PSI] = psi[cell];
  r[LDC_FV_WALL_OMEGA] = om[cell];
  if (!J.refine || none) return;
  const double Cc = psi[cell];
  const double W = fv_wall_reflected(psi, nx, ny, i - 1, j), E = fv_wall_reflected(psi, nx, ny, i + 1, j);
  const double S = fv_wall_reflected(psi, nx, ny, i, j - 1), N = fv_wall_reflected(psi, nx, ny, i, j + 1);
  const double SW = fv_wall_reflected(psi, nx, ny, i - 1, j - 1), SE = fv_wall_reflected(psi, nx, ny, i + 1, j - 1);
  const double NW = fv_wall_reflected(psi, nx, ny, i - 1, j + 1), NE = fv_wall_reflected(psi, nx, ny, i + 1, j + 1);
  const double gx = (E - W) * 0.5, gy = (N - S) * 0.5;
  const double Hxx = (E - 2 * Cc) + W, Hyy = (N - 2 * Cc) + S, Hxy = (((NE - NW) - SE) + SW) * 0.25;
  const double det = Hxx * Hyy - Hxy * Hxy;
  const double Fxx = 4 * eps * ((fabs(E) + 2 * fabs(Cc)) + fabs(W));
  const double Fyy = 4 * eps * ((fabs(N) + 2 * fabs(Cc)) + fabs(S));
  const double Fxy = eps * (((fabs(NE) + fabs(NW)) + fabs(SE)) + fabs(SW));
  const bool definite = fabs(Hxx) > Fxx && fabs(Hyy) > Fyy &&
                        det > (Fxx * fabs(Hyy) + Fyy * fabs(Hxx)) + 2 * Fxy * fabs(Hxy) && (want_min ? Hxx > 0 : Hxx < 0);
  if (!definite) { r[LDC_FV_WALL_STATUS] = 2.0; return; }
  const double sx = -(Hyy * gx - Hxy * gy) / det, sy = -(Hxx * gy - Hxy * gx) / det;
  const double x = ((i + 0.5) + sx) * J.dx, y = ((j + 0.5) + sy) * J.dy;
  const double big = 1.7976931348623157e308;
  if (!(fabs(sx) <= 1.0) || !(fabs(sy) <= 1.0) || !(x >= 0.0 && x <= nx * J.dx) || !(y >= 0.0 && y <= ny * J.dy)) {
    r[LDC_FV_WALL_STATUS] = 3.0;
    return;
  }
  const double ps = Cc + 0.5 * (gx * sx + gy * sy);
  double w = om[cell];
  if (i > 0 && i < nx - 1 && j > 0 && j < ny - 1) {      // the same six-term quadratic of omega, off the ring only
    const double wC = om[cell], wW = om[cell - 1], wE = om[cell + 1], wS = om[cell - nx], wN = om[cell + nx];
    const double wSW = om[cell - nx - 1], wSE = om[cell - nx + 1], wNW = om[cell + nx - 1], wNE = om[cell + nx + 1];
    const double ax = (wE - wW) * 0.5, ay = (wN - wS) * 0.5;
    const double Axx = (wE - 2 * wC) + wW, Ayy = (wN - 2 * wC) + wS, Axy = (((wNE - wNW) - wSE) + wSW) * 0.25;
    w = ((((wC + ax * sx) + ay * sy) + ((0.5 * Axx) * sx) * sx) + ((0.5 * Ayy) * sy) * sy) + (Axy * sx) * sy;
  }
  if (!(fabs(ps) <= big) || !(fabs(w) <= big)) { r[LDC_FV_WALL_STATUS] = 3.0; return; }
  r[LDC_FV_WALL_X] = x;
  r[LDC_FV_WALL_Y] = y;
  r[LDC_FV_WALL_PSI] = ps;
  r[LDC_FV_WALL_OMEGA] = w;
  r[LDC_FV_WALL_STATUS] = 0.0;
  r[LDC_FV_WALL_SX] = sx;
  r[LDC_FV_WALL_SY] = sy;
}

// ---- 4. result (one work-group per job): thread t takes slot t, the same merge, the LDC_FV_POST_* slots, the groups
__global__ __launch_bounds__(kWallThreads) void fv_wall_result(const FvWallLaunch L) {
  __shared__ double lkey[kWallWaves][kFvPostBest];
  __shared__ int lidx[kWallWaves][kFvPostBest];
  const ldc_fv_wall_job& J = L.jobs[blockIdx.y];
  const int G = wall_groups(J), n = J.nx * J.ny;
  const bool mine = (int)threadIdx.x < G;
  const double* s = wall_slots(J) + (mine ? (int)threadIdx.x : 0) * kWallSlot;
  FvBest best[kFvPostBest];
#pragma unroll
  for (int q = 0; q < kFvPostBest; ++q) {
    best[q].key = mine ? s[q] : -HUGE_VAL;
    best[q].idx = mine ? (int)s[WS_CELL + q] : kFvPostNone;
  }
  const bool bad = mine && (s[WS_BAD_OMEGA] != 0.0 || s[WS_BAD_PSI] != 0.0);
  fv_post_best_merge<kWallWaves>(best, lkey, lidx);
  const int any_bad = __syncthreads_or(bad ? 1 : 0);
  if (threadIdx.x != 0) return;
  double* r = J.result;
  fv_post_result(n, J.psi, J.omega, best, any_bad, r);
  const bool flagged = r[LDC_FV_POST_NONFINITE] != 0.0;
  fv_wall_group(J, (int)r[LDC_FV_POST_PSI_MIN_CELL], true, flagged, r + LDC_FV_POST_RESULT_LEN);
  for (int q = 0; q < 3; ++q) {
    const bool none = flagged || !(r[LDC_FV_POST_PSI_BR + q] > 0.0);
    fv_wall_group(J, (int)r[LDC_FV_POST_PSI_BR_CELL + q], false, none,
                  r + LDC_FV_POST_RESULT_LEN + (1 + q) * LDC_FV_WALL_GROUP_LEN);
  }
}

template <typename K>
inline int wall_launch(K kernel, int groups, int jobs, hipStream_t st, const FvWallLaunch& L) {
  hipLaunchKernelGGL(kernel, dim3(groups, jobs), dim3(kWallThreads), 0, st, L);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

}  // namespace

extern "C" {

int ldc_fv_wall_post_launches(int n) {
  if (n < 1) return LDC_E_ARG;
  return kWallLaunches * ((n + LDC_FV_WALL_LAUNCH_MAX - 1) / LDC_FV_WALL_LAUNCH_MAX);
}

int ldc_fv_wall_post_enqueue(const struct ldc_fv_wall_job* jobs, int n, void* stream) {
  if (!jobs || n < 1) return LDC_E_ARG;
  for (int q = 0; q < n; ++q) {
    const ldc_fv_wall_job& j = jobs[q];
    const void* req[] = {j.u, j.v, j.ulid, j.Cx, j.lamx, j.Cy, j.lamy, j.psi, j.omega, j.scratch, j.result};
    for (const void* x : req) if (!x) return LDC_E_ARG;
    if (j.nx < LDC_FV_MIN_N || j.nx > LDC_FV_WIDE_MAX_N || j.ny < LDC_FV_MIN_N || j.ny > LDC_FV_WIDE_MAX_N) return LDC_E_ARG;
    if (!(j.dx > 0) || !(j.dy > 0)) return LDC_E_ARG;
    if (j.ix_lt < 0 || j.ix_lt > j.nx || j.ix_gt < 0 || j.ix_gt > j.nx) return LDC_E_ARG;
    if (j.jy_lt < 0 || j.jy_lt > j.ny || j.jy_gt < 0 || j.jy_gt > j.ny) return LDC_E_ARG;
    if (j.refine != 0 && j.refine != 1) return LDC_E_ARG;
  }
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) return LDC_E_NODEVICE;
  hipStream_t st = as_stream(stream);
  for (int lo = 0; lo < n; lo += LDC_FV_WALL_LAUNCH_MAX) {
    FvWallLaunch L;
    const int b = n - lo < LDC_FV_WALL_LAUNCH_MAX ? n - lo : LDC_FV_WALL_LAUNCH_MAX;
    int G = 1, gg = 1;
    for (int q = 0; q < LDC_FV_WALL_LAUNCH_MAX; ++q) {
      L.jobs[q] = jobs[lo + (q < b ? q : 0)];
      if (q < b && wall_groups(L.jobs[q]) > G) G = wall_groups(L.jobs[q]);
      if (q < b && wall_gemm_groups(L.jobs[q]) > gg) gg = wall_gemm_groups(L.jobs[q]);
    }
    int e = wall_launch(fv_wall_omega, G, b, st, L);
    if (!e) e = wall_launch(fv_wall_gemm<0>, gg, b, st, L);
    if (!e) e = wall_launch(fv_wall_gemm<1>, gg, b, st, L);
    if (!e) e = wall_launch(fv_wall_gemm<2>, gg, b, st, L);
    if (!e) e = wall_launch(fv_wall_gemm<3>, gg, b, st, L);
    if (!e) e = wall_launch(fv_wall_extrema, G, b, st, L);
    if (!e) e = wall_launch(fv_wall_result, 1, b, st, L);
    if (e) return e;
  }
  return 0;
}

}  // extern "C"
