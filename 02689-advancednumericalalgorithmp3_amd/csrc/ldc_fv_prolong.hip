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
//
// The arithmetic is NOT written here: the axes, the interpolant, one fine cell and one face are the functions of
// ldc_fv_prolong_cells.inc, which ldc_fv_wide.hip calls too (fv_wide_prolong_*: the same transfer for chip or shared
// trials, two launches per pair).  What this unit adds is the mapping: the loops of a work-group of 512 threads and the
// barrier between the phases.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ldc_hip.h"
#include "ldc_fv_common.inc"

#pragma STDC FP_CONTRACT OFF

#include "ldc_fv_prolong_cells.inc"     // (behind the pragma: its arithmetic rounds with contraction off)

namespace {

struct FvProlongLaunch {
  const FvDesc* coarse[LDC_FV_PROLONG_LAUNCH_MAX];
  const FvDesc* fine[LDC_FV_PROLONG_LAUNCH_MAX];
};
static_assert(sizeof(FvProlongLaunch) <= 3600, "kernel arguments");

// ---- 1. u, v, p at the fine cell centres
__device__ __forceinline__ void fv_prolong_cells(const FvDesc& c, const FvDesc& f) {
  const int nx = f.nx, n = f.nx * f.ny;
  const FvAxis ax = {c.nx, c.dx}, ay = {c.ny, c.dy};
  const double p0 = fv_prolong_p0(c, f, ax, ay);
  for (int cell = threadIdx.x; cell < n; cell += kFvThreads) fv_prolong_cell(c, f, ax, ay, nx, p0, cell);
  __syncthreads();
}

// ---- 2. mdot = [ fx | fy ] from the new u and v
__device__ __forceinline__ void fv_prolong_fluxes(const FvDesc& f) {
  const int nx = f.nx, ny = f.ny;
  const int nfx = ny * (nx + 1), nfy = (ny + 1) * nx;
  double *fx = f.mdot, *fy = f.mdot + nfx;
  for (int q = threadIdx.x; q < nfx; q += kFvThreads) fv_prolong_xface(f, nx, fx, q);
  for (int q = threadIdx.x; q < nfy; q += kFvThreads) fv_prolong_yface(f, nx, ny, fy, q);
}

__global__ __launch_bounds__(kFvThreads) void fv_prolong_kernel(const FvProlongLaunch L) {
  const FvDesc& c = *L.coarse[blockIdx.x];
  const FvDesc& f = *L.fine[blockIdx.x];
  fv_prolong_cells(c, f);
  fv_prolong_fluxes(f);
}

inline bool fv_size_ok(const ldc_fv* h) {
  return h->nx >= LDC_FV_MIN_N && h->nx <= LDC_FV_MAX_N && h->ny >= LDC_FV_MIN_N && h->ny <= LDC_FV_MAX_N;
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
    if (!fv_size_ok(coarse[q]) || !fv_size_ok(fine[q]) || !fv_same_domain(*coarse[q], *fine[q])) return LDC_E_ARG;
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
