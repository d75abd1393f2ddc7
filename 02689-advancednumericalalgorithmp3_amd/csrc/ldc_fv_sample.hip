// ldc_fv_sample.hip -- a finite-volume state sampled at the nodes of a tensor grid (include/ldc_fv.h,
// ldc_fv_sample_nodes): the initial guess of a spectral trial from a converged finite-volume trial of the same cavity.
// A translation unit of its own, linked into libldc_hip.so beside the others: every other code object is the same with
// and without this file.
//
// Mapping: blockIdx.y is the job, the work-groups of a job (256 threads each) stride over its Mx My nodes, one node per
// thread and pass.  A node reads at most four cells of each source field and writes its own three values: nobody waits
// for anybody, no atomics, no LDS, no reduction, so a job's result is the same bits whatever else is in the call.  The
// kernel is memory-bound and tiny (a spectral grid has at most 257 x 257 nodes).
//
// The arithmetic is NOT written here: the axes, the ring-extended field and its bilinear interpolant (x first) are
// FvAxis::locate, fv_prolong_node and fv_prolong_at of ldc_fv_prolong_cells.inc, included behind the pragma below so
// that no multiply-add is contracted; tests/fv_sample_numpy.py states the same transfer in NumPy.  What this unit adds:
//   - interior nodes (0 < ix < Mx - 1, 0 < iy < My - 1): U, V the interpolants of u, v with the ring of walls and lid, P
//     the interpolant of p with the zero-gradient ring, not shifted (only grad p enters the spectral residual);
//   - boundary nodes: the TARGET's values, bit for bit: u = v = 0.0 on the three walls, v = 0.0 and u = ulid_nodes[ix] on
//     iy = My - 1, the two top corners included; P has no boundary nodes.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ldc_hip.h"
#include "ldc_fv_common.inc"

#pragma STDC FP_CONTRACT OFF

#include "ldc_fv_prolong_cells.inc"     // (behind the pragma: its arithmetic rounds with contraction off)

namespace {

constexpr int kSampleThreads = 256;
constexpr int kSampleGroupsMax = 256;      // work-groups of one job: one per CU is plenty for 257 x 257 nodes

struct FvSampleLaunch {
  ldc_fv_sample_job jobs[LDC_FV_SAMPLE_LAUNCH_MAX];
};
static_assert(sizeof(FvSampleLaunch) <= 3600, "kernel arguments");

__global__ __launch_bounds__(kSampleThreads) void fv_sample_kernel(const FvSampleLaunch L) {
  const ldc_fv_sample_job& J = L.jobs[blockIdx.y];
  const int Mx = J.Mx, My = J.My;
  const long long nodes = (long long)Mx * My;
  FvDesc c = {};                            // what fv_prolong_node reads of a descriptor: the sizes and the lid profile
  c.nx = J.nx; c.ny = J.ny; c.ulid = J.ulid;
  const FvAxis ax = {J.nx, J.dx}, ay = {J.ny, J.dy};
  const long long stride = (long long)gridDim.x * kSampleThreads;
  for (long long q = (long long)blockIdx.x * kSampleThreads + threadIdx.x; q < nodes; q += stride) {
    const int ix = (int)(q / My), iy = (int)(q % My);
    if (iy == My - 1) {                     // the lid, top corners included
      J.U[q] = J.ulid_nodes[ix];
      J.V[q] = 0.0;
    } else if (ix == 0 || ix == Mx - 1 || iy == 0) {
      J.U[q] = 0.0;
      J.V[q] = 0.0;
    } else {
      int kx, ky;
      double tx, ty;
      ax.locate(J.x[ix], kx, tx);
      ay.locate(J.y[iy], ky, ty);
      J.U[q] = fv_prolong_at<FV_RING_U>(c, J.u, kx, tx, ky, ty);
      J.V[q] = fv_prolong_at<FV_RING_V>(c, J.v, kx, tx, ky, ty);
      J.P[(long long)(ix - 1) * (My - 2) + (iy - 1)] = fv_prolong_at<FV_RING_P>(c, J.p, kx, tx, ky, ty);
    }
  }
}

}  // namespace

extern "C" {

int ldc_fv_sample_nodes(const struct ldc_fv_sample_job* jobs, int n, void* stream) {
  if (!jobs || n < 1) return LDC_E_ARG;
  for (int q = 0; q < n; ++q) {
    const ldc_fv_sample_job& j = jobs[q];
    if (!j.u || !j.v || !j.p || !j.ulid || !j.x || !j.y || !j.ulid_nodes || !j.U || !j.V || !j.P) return LDC_E_ARG;
    if (j.nx < LDC_FV_MIN_N || j.nx > LDC_FV_WIDE_MAX_N || j.ny < LDC_FV_MIN_N || j.ny > LDC_FV_WIDE_MAX_N) return LDC_E_ARG;
    if (j.Mx < 3 || j.My < 3) return LDC_E_ARG;
    if (!(j.dx > 0) || !(j.dy > 0)) return LDC_E_ARG;
  }
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) return LDC_E_NODEVICE;
  for (int lo = 0; lo < n; lo += LDC_FV_SAMPLE_LAUNCH_MAX) {
    FvSampleLaunch L;
    const int b = n - lo < LDC_FV_SAMPLE_LAUNCH_MAX ? n - lo : LDC_FV_SAMPLE_LAUNCH_MAX;
    long long most = 0;
    for (int q = 0; q < LDC_FV_SAMPLE_LAUNCH_MAX; ++q) {
      L.jobs[q] = jobs[lo + (q < b ? q : 0)];
      const long long nodes = (long long)L.jobs[q].Mx * L.jobs[q].My;
      if (q < b && nodes > most) most = nodes;
    }
    const long long want = (most + kSampleThreads - 1) / kSampleThreads;
    const int groups = (int)(want < kSampleGroupsMax ? want : kSampleGroupsMax);
    hipLaunchKernelGGL(fv_sample_kernel, dim3(groups, b), dim3(kSampleThreads), 0, as_stream(stream), L);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  return 0;
}

}  // extern "C"
