// ldc_fv_wide.hip -- ONE finite-volume trial advanced by the whole chip (include/ldc_fv.h, ldc_fv_wide_*).  A translation
// unit of its own, linked into libldc_hip.so beside ldc_kernels.hip and the other FV units: the code object of the solve
// kernels is the same with and without this file.
//
// Mapping: one kernel launch per phase of the SIMPLE iteration, up to 256 work-groups of 256 threads each, every cell
// sweep a grid-stride loop.  The launch boundary is the only barrier between work-groups: nobody waits for anybody, so
// there are no flags, no spin limits and no co-residency.  The arithmetic is NOT written here: every phase calls the
// cell functions of ldc_fv_cells.inc, which ldc_fv_kernel.inc (one trial per CU) calls too, on the same work vectors
// (FvVec), so after one iteration `work` holds the intermediates ldc_fv_step_debug copies out.  What this unit adds is
// the mapping: the gate, the grid-stride cell loop, the slots the partial sums go through, `par`, the BiCGSTAB scalars
// in scratch, the block maps of a batch and the graphs.  (Two cell bodies are copies, not calls: the x sweep of
// wide_bicg_x and wide_correct; ldc_fv_cells.inc says why.)
// One iteration is the chain
//   assemble | min(lin_budget, max_lin_iters) x (p, v, s, t, x) | linfinish | faces | gemm x 4 | correct | fluxvort |
//   sums | record
// and, for a trial with Anderson mixing attached (ldc_fv_wide_set_anderson; ldc_fv_wide_anderson.inc), behind it
//   push | mix | close
// A trial with the consistent pressure equation (ldc_fv_wide_set_pressure; ldc_fv_wide_pressure.inc) replaces
// `faces | gemm x 4` and `fluxvort` by
//   faces | init | min(pressure budget, pressure_max_iters) x (gemm x 4 | rz | ap | xr) | pfinish    and    fluxvort
// of its own: conjugate gradients on the a_P-weighted operator, preconditioned by the same four GEMMs.
// A lone trial with geometry tables (ldc_fv_wide_set_grid; ldc_fv_wide_stretched.inc) runs either chain on a wall-clustered
// tensor grid: launch for launch the same, with stretched twins of the phases that read the geometry (assemble, faces,
// correct, fluxvort, sums, ap) around the cell bodies of ldc_fv_stretched_cells.inc, which the one-CU stretched units call too.
// With the tables of the separable scaled preconditioner attached as well (ldc_fv_wide_set_preconditioner;
// ldc_fv_wide_separable.inc) the consistent chain of such a trial takes twins of init, rz, ap and xr and hands the four GEMMs
// the eigenpairs of the fitted operator: z = s . L_s+ (s . r), launch for launch the same chain.
// Rules every kernel keeps:
//  - the grid is a function of (nx, ny) alone;
//  - a work-group writes its partial sums to its own slot; the NEXT launch lets every work-group add all slots in one
//    fixed order, so all work-groups hold the same scalars and runs repeat bit for bit;
//  - no work-group reads a word another work-group of the same launch writes: the slots and the BiCGSTAB scalars exist
//    twice and alternate by launch (`par`), and the latch, the NaN word, the overflow word and the record row are
//    written by launches of ONE work-group only (begin, linfinish, record);
//  - every kernel but `begin` starts at the gate: latch, NaN word or overflow word set -> return at once (the mixing
//    launches have a gate of their own: ctrl[1] == astate[2] -> return at once).
// The data-dependent BiCGSTAB loop is a fixed number of launches; once both components have finished their launches
// only carry the scalars on.  A component still active after lin_budget < max_lin_iters iterations sets the overflow
// word in `linfinish`, BEFORE u, v, p or mdot have been touched (assemble and BiCGSTAB write work vectors only), and
// the host repeats the rest of the chunk with twice the budget: the result does not depend on the budget.
//
// scratch (LDC_FV_WIDE_SCRATCH_LEN doubles): 16 int64 words (overflow: 1 from linfinish, 2 from pfinish; record row, pending give-ups, pending BiCGSTAB
// iterations, the enqueue's quota of iterations), 2 x 32 doubles of BiCGSTAB scalars, 2 x G x 10 slot sums, G x 10 sums
// of the record row.
//
// Several trials in the same launches (ldc_fv_wide_batch_*, mapping="shared"): none of the rules needs a trial to be
// alone on the card, so every phase is a device function of (the trial's arguments, the work-group's index g WITHIN its
// trial) and exists as two kernels.  The lone one passes (its argument block, blockIdx.x).  The batch one looks its
// work-group up in a table in device memory that ldc_fv_wide_batch_create wrote once: a block map `blockIdx.x -> (trial
// q, g)` for the cell sweeps and one for the GEMMs (one scalar load, the same for every lane; a prefix array would cost a
// chain of eight dependent loads at 256 trials), q = blockIdx.x for the launches of one work-group per trial, then a copy
// of entry q of the argument table.  No kernel ever writes the table, so these are scalar loads.  The arithmetic, the
// sweep order, the slots, `par` and the trial's own G are the lone kernels': a trial in a batch is bit-identical to its
// lone run.  An enqueue gives every trial a quota of iterations (the word WW_QUOTA, written by `begin`) and runs
// max(quota) chains; the gate also returns once the trial's record row has reached its quota, so a trial that is
// finished, capped, NaN, overflowed or not meant at all (quota 0) costs empty work-groups and the table is never rebuilt.
//
// Behind the solve, at the end of this file: the post-processing chain (ldc_fv_wide_post_enqueue: omega, psi and the vortex
// extrema of one trial in seven launches) and the prolongation (ldc_fv_wide_prolong_enqueue: two launches per pair), by
// the same rules for trials of up to 1024 x 1024 cells.  They have no gate and touch neither ctrl, rec nor `scratch`.
// Their arithmetic, and that of the mixing, is not written here either: ldc_fv_post_cells.inc, ldc_fv_prolong_cells.inc
// and ldc_fv_anderson_cells.inc hold it for this unit and for the one-CU units ldc_fv_post.hip, ldc_fv_prolong.hip and
// ldc_fv_anderson.hip alike.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <mutex>
#include <new>
#include <utility>
#include <vector>

#include "ldc_hip.h"
#include "ldc_fv_common.inc"
#include "ldc_fv_cells.inc"
#include "ldc_fv_pressure_cells.inc"
#include "ldc_fv_anderson_cells.inc"
#include "ldc_fv_post_cells.inc"
// (ldc_fv_prolong_cells.inc: at the prolongation section, behind its FP_CONTRACT pragma)

namespace {

constexpr int kWT = 256;                    // threads of a work-group
constexpr int kWW = kWT / 64;
constexpr int kWS = 10;                     // doubles of a slot
constexpr int kWMaxG = 256;                 // most work-groups of a sweep: one per CU, and one slot per thread to add
constexpr int kWWords = 16;
constexpr int kWKry = 32;                   // doubles of one copy of the BiCGSTAB scalars: 16 per component
enum { WW_OVF, WW_ROW, WW_GIVEUPS, WW_LIN_ITERS, WW_QUOTA };
static_assert(LDC_FV_WIDE_SCRATCH_LEN(8, 8) == kWWords + 2 * kWKry + 3 * kWS * 1, "scratch layout");
static_assert(LDC_FV_WIDE_SCRATCH_LEN(1024, 1024) == kWWords + 2 * kWKry + 3 * kWS * kWMaxG, "scratch layout");

struct FvWideArgs {
  FvDesc d;
  double* scr;
  int G;                                    // work-groups of a sweep
  int pmax;                                 // pressure_max_iters of a trial with the consistent pressure equation; 0: the
                                            // reference's (in what was padding: the struct keeps its 208 bytes)
};

// The per-trial Anderson mixing block (ldc_fv_wide_set_anderson; ldc_fv_wide_anderson.inc): in the handle, by value in the
// lone kernels' arguments, behind FvWideArgs in the table entry.  All zero: no mixing.
struct FvWideMix {
  double* hist;
  long long* astate;
  double* mscr;
  int depth, start;
};
static_assert(sizeof(FvWideMix) == 32, "the mixing block");

// The table of a batch in the caller's device buffer (LDC_FV_WIDE_BATCH_TABLE_LEN bytes): n entries, then the block map
// of the cell sweeps (sum of G_q words) and that of the GEMMs (sum of LDC_FV_WIDE_GEMM_GROUPS words), one word
// q << 16 | g per work-group, trial after trial.
// The per-trial block of the consistent pressure equation (ldc_fv_wide_set_pressure; ldc_fv_wide_pressure.inc), behind the
// mixing block in the table entry: with it the entry's 256 bytes are full.
struct FvWidePcg {
  double tol;
  long long* stats;                         // LDC_FV_WIDE_PRESSURE_SCRATCH_LEN words: iterations, solves, cap hits, last count
};
static_assert(sizeof(FvWidePcg) == 16, "the pressure block");

struct FvWideEntry {
  FvWideArgs a;
  FvWideMix m;
  FvWidePcg x;
};
static_assert(sizeof(FvWideEntry) == LDC_FV_WIDE_BATCH_ENTRY_BYTES && sizeof(FvWideArgs) == 208, "table entry");
static_assert(LDC_FV_WIDE_BATCH_MAX <= 1 << 15 && LDC_FV_WIDE_GEMM_GROUPS(LDC_FV_WIDE_MAX_N, LDC_FV_WIDE_MAX_N) <= 1 << 16,
              "a block-map word");

struct FvWideTable {
  const FvWideEntry* __restrict__ entries;
  const uint32_t* __restrict__ sweep;
  const uint32_t* __restrict__ gemm;
};

struct FvWideQuotas {
  int32_t q[LDC_FV_WIDE_BATCH_MAX];
};

__device__ __forceinline__ long long* wide_words(const FvWideArgs& a) { return reinterpret_cast<long long*>(a.scr); }
__device__ __forceinline__ double* wide_kry(const FvWideArgs& a, int par) { return a.scr + kWWords + kWKry * par; }
__device__ __forceinline__ double* wide_slots(const FvWideArgs& a, int par) {
  return a.scr + kWWords + 2 * kWKry + par * a.G * kWS;
}
__device__ __forceinline__ double* wide_rec_slots(const FvWideArgs& a) { return a.scr + kWWords + 2 * kWKry + 2 * a.G * kWS; }

// the gate: true when the launch has nothing to do
__device__ __forceinline__ bool wide_gate(const FvWideArgs& a) {
  const long long* w = wide_words(a);
  return a.d.ctrl[0] != 0 || a.d.ctrl[2] != 0 || w[WW_OVF] != 0 || w[WW_ROW] >= w[WW_QUOTA];
}

// sums of K values over the work-group in a fixed order; every thread gets the totals.  Ends on a barrier, so `lds`
// can be used again at once.
template <int K>
__device__ __forceinline__ void wide_block_sum(double (&a)[K], double* lds) {
  static_assert(K <= kWS, "slot");
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) a[k] += __shfl_xor(a[k], off);
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) lds[w * kWS + k] = a[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < kWW; ++q) s += lds[q * kWS + k];
    a[k] = s;
  }
  __syncthreads();
}

// the totals of entries first .. first + K - 1 over all G slots the launch before wrote: thread t takes slot t
template <int K>
__device__ __forceinline__ void wide_slot_sum(const double* slots, int G, int first, double (&a)[K], double* lds) {
#pragma unroll
  for (int k = 0; k < K; ++k) a[k] = (int)threadIdx.x < G ? slots[threadIdx.x * kWS + first + k] : 0.0;
  wide_block_sum(a, lds);
}

// the partial sums of work-group g (of its trial) into entries first .. of its own slot
template <int K>
__device__ __forceinline__ void wide_slot_put(double* slots, int g, int first, double (&a)[K], double* lds) {
  wide_block_sum(a, lds);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) slots[g * kWS + first + k] = a[k];
  }
}

__device__ __forceinline__ void wide_kry_load(const double* K, FvKrylov (&s)[2]) {
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const double* k = K + 16 * q;
    s[q].atol = k[0]; s[q].nr2 = k[1]; s[q].rh = k[2]; s[q].rh_prev = k[3]; s[q].alpha = k[4]; s[q].omega = k[5];
    s[q].beta = k[6]; s[q].act = k[7] != 0.0; s[q].brk = k[8] != 0.0; s[q].fin = k[9] != 0.0; s[q].its = (int)k[10];
  }
}

// (work-group 0 alone writes the copy the NEXT launch reads)
__device__ __forceinline__ void wide_kry_store(double* K, int g, const FvKrylov (&s)[2]) {
  if (g != 0 || threadIdx.x != 0) return;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    double* k = K + 16 * q;
    k[0] = s[q].atol; k[1] = s[q].nr2; k[2] = s[q].rh; k[3] = s[q].rh_prev; k[4] = s[q].alpha; k[5] = s[q].omega;
    k[6] = s[q].beta; k[7] = s[q].act ? 1.0 : 0.0; k[8] = s[q].brk ? 1.0 : 0.0; k[9] = s[q].fin ? 1.0 : 0.0;
    k[10] = (double)s[q].its;
  }
}

// ---- begin: the first launch of an enqueue (one work-group): the overflow word and the record row start at 0, the
//      quota is the number of iterations the enqueue means for this trial
__device__ __forceinline__ void wide_begin(const FvWideArgs& a, int quota) {
  if (threadIdx.x == 0) {
    wide_words(a)[WW_OVF] = 0;
    wide_words(a)[WW_ROW] = 0;
    wide_words(a)[WW_QUOTA] = quota;
  }
}

// ---- 1. grad p, the five diagonals, the relaxed right-hand sides, the BiCGSTAB start; slot: |b_u|^2, |b_v|^2
__device__ __forceinline__ void wide_assemble(const FvWideArgs& a, int g, int par, double* lds) {
  if (wide_gate(a)) return;
  const FvCtx x(a.d);
  double b2[2] = {0.0, 0.0};
  for (int c = g * kWT + threadIdx.x; c < x.n; c += a.G * kWT) fv_cell_assemble(x, c, b2);
  wide_slot_put(wide_slots(a, par ^ 1), g, 0, b2, lds);
}

// ---- 2. the joint u / v BiCGSTAB, iteration `it`, one launch per sweep of fv_bicgstab.  Each reads the scalars of
//         copy `par` and the slots `par`, and writes the copies par ^ 1.
// p: the scalars from the sums of the launch before (it = 0: |b|^2 of assemble), the head test; p and phat
__device__ __forceinline__ void wide_bicg_p(const FvWideArgs& a, int g, int it, int par, double* lds) {
  if (wide_gate(a)) return;
  const FvCtx x(a.d);
  FvKrylov s[2];
  if (it == 0) {
    double b2[2];
    wide_slot_sum(wide_slots(a, par), a.G, 0, b2, lds);
#pragma unroll
    for (int q = 0; q < 2; ++q) fv_kry_start(s[q], b2[q], x.d.lin_tol);
  } else {
    wide_kry_load(wide_kry(a, par), s);
    double s4[4];
    wide_slot_sum(wide_slots(a, par), a.G, 0, s4, lds);
#pragma unroll
    for (int q = 0; q < 2; ++q) fv_kry_after_x(s[q], s4[2 * q], s4[2 * q + 1], it);
  }
#pragma unroll
  for (int q = 0; q < 2; ++q) fv_kry_head(s[q], it);
  wide_kry_store(wide_kry(a, par ^ 1), g, s);
  if (!s[0].act && !s[1].act) return;
  for (int c = g * kWT + threadIdx.x; c < x.n; c += a.G * kWT) {
    const double dg = x.w[FV_AP * x.n + c] * x.inv_a;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      if (!s[q].act) continue;
      fv_cell_p(x, c, q, it, s[q], dg);
    }
  }
}

// v = A phat; slot: rtilde . v
__device__ __forceinline__ void wide_bicg_v(const FvWideArgs& a, int g, int par, double* lds) {
  if (wide_gate(a)) return;
  const FvCtx x(a.d);
  FvKrylov s[2];
  wide_kry_load(wide_kry(a, par), s);
  wide_kry_store(wide_kry(a, par ^ 1), g, s);
  if (!s[0].act && !s[1].act) return;
  double s2[2] = {0, 0};
  for (int c = g * kWT + threadIdx.x; c < x.n; c += a.G * kWT) {
    const int i = c % x.nx, j = c / x.nx;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      if (!s[q].act) continue;
      fv_cell_v(x, c, i, j, q, s2[q]);
    }
  }
  wide_slot_put(wide_slots(a, par ^ 1), g, 0, s2, lds);
}

// alpha; s = r - alpha v (into r) and shat
__device__ __forceinline__ void wide_bicg_s(const FvWideArgs& a, int g, int par, double* lds) {
  if (wide_gate(a)) return;
  const FvCtx x(a.d);
  FvKrylov s[2];
  wide_kry_load(wide_kry(a, par), s);
  if (s[0].act || s[1].act) {
    double s2[2];
    wide_slot_sum(wide_slots(a, par), a.G, 0, s2, lds);
#pragma unroll
    for (int q = 0; q < 2; ++q) fv_kry_alpha(s[q], s2[q]);
  }
  wide_kry_store(wide_kry(a, par ^ 1), g, s);
  if (!s[0].act && !s[1].act) return;
  for (int c = g * kWT + threadIdx.x; c < x.n; c += a.G * kWT) {
    const double dg = x.w[FV_AP * x.n + c] * x.inv_a;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      if (!s[q].act || s[q].brk) continue;
      fv_cell_s(x, c, q, s[q], dg);
    }
  }
}

// t = A shat; slot: s.s, t.s, t.t per component
__device__ __forceinline__ void wide_bicg_t(const FvWideArgs& a, int g, int par, double* lds) {
  if (wide_gate(a)) return;
  const FvCtx x(a.d);
  FvKrylov s[2];
  wide_kry_load(wide_kry(a, par), s);
  wide_kry_store(wide_kry(a, par ^ 1), g, s);
  if (!s[0].act && !s[1].act) return;
  double s3[6] = {0, 0, 0, 0, 0, 0};
  for (int c = g * kWT + threadIdx.x; c < x.n; c += a.G * kWT) {
    const int i = c % x.nx, j = c / x.nx;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      if (!s[q].act || s[q].brk) continue;
      fv_cell_t(x, c, i, j, q, s3 + 3 * q);
    }
  }
  wide_slot_put(wide_slots(a, par ^ 1), g, 0, s3, lds);
}

// omega (or the early finish on |s|); x and r; slot: r.r, rtilde.r per component
__device__ __forceinline__ void wide_bicg_x(const FvWideArgs& a, int g, int it, int par, double* lds) {
  if (wide_gate(a)) return;
  const FvCtx x(a.d);
  FvKrylov s[2];
  wide_kry_load(wide_kry(a, par), s);
  if (s[0].act || s[1].act) {
    double s3[6];
    wide_slot_sum(wide_slots(a, par), a.G, 0, s3, lds);
#pragma unroll
    for (int q = 0; q < 2; ++q) fv_kry_omega(s[q], s3[3 * q], s3[3 * q + 1], s3[3 * q + 2], it);
  }
  wide_kry_store(wide_kry(a, par ^ 1), g, s);
  if (!s[0].act && !s[1].act) return;
  double s4[4] = {0, 0, 0, 0};
  for (int c = g * kWT + threadIdx.x; c < x.n; c += a.G * kWT) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {               // (a copy of the x sweep of fv_bicgstab, ldc_fv_kernel.inc: a change to
      if (!s[q].act) continue;                  // one goes into the other; ldc_fv_cells.inc says why)
      double *xs = x.vec(FV_XU, q), *ph = x.vec(FV_PHU, q);
      if (s[q].fin) xs[c] += s[q].alpha * ph[c];
      else {
        double* rs = x.vec(FV_RU, q);
        double xn = xs[c]; xn += s[q].alpha * ph[c]; xn += s[q].omega * x.vec(FV_SHU, q)[c]; xs[c] = xn;
        const double r = rs[c] - s[q].omega * x.vec(FV_TU, q)[c];
        rs[c] = r; s4[2 * q] += r * r; s4[2 * q + 1] += x.vec(FV_RTU, q)[c] * r;
      }
    }
  }
  wide_slot_put(wide_slots(a, par ^ 1), g, 0, s4, lds);
}

// linfinish (one work-group), after `nb` = min(lin_budget, max_lin_iters) iterations: the last sums; a component still
// active at nb = max_lin_iters is the accepted give-up, at nb < max_lin_iters the overflow (nothing but work vectors
// has been written so far).  The counters wait in the scratch words for the record launch.
__device__ __forceinline__ void wide_linfinish(const FvWideArgs& a, int nb, int par, double* lds) {
  if (wide_gate(a)) return;
  FvKrylov s[2];
  wide_kry_load(wide_kry(a, par), s);
  double s4[4];
  wide_slot_sum(wide_slots(a, par), a.G, 0, s4, lds);
#pragma unroll
  for (int q = 0; q < 2; ++q) fv_kry_after_x(s[q], s4[2 * q], s4[2 * q + 1], nb);
  long long giveups = 0, lin_iters = 0;
  bool overflow = false;
  if (nb < a.d.maxit) {
#pragma unroll
    for (int q = 0; q < 2; ++q) fv_kry_head(s[q], nb);        // (what iteration nb would find first)
    overflow = s[0].act || s[1].act;
  } else {
    giveups = (s[0].act ? 1 : 0) + (s[1].act ? 1 : 0);
  }
  lin_iters = s[0].its + s[1].its;
  if (threadIdx.x == 0) {
    long long* w = wide_words(a);
    if (overflow) w[WW_OVF] = 1;
    else { w[WW_GIVEUPS] = giveups; w[WW_LIN_ITERS] = lin_iters; }
  }
}

// ---- 3. Rhie-Chow face velocities, mdot*, rhs_p = -div mdot* (entry 0 = 0); slot: the sum of rhs_p, whose negative
//         is the cell-0 entry of the pinned solve (the first GEMM puts it in as it reads C)
__device__ __forceinline__ void wide_faces(const FvWideArgs& a, int g, int par, double* lds) {
  if (wide_gate(a)) return;
  const FvCtx x(a.d);
  double csum[1] = {0.0};
  for (int c = g * kWT + threadIdx.x; c < x.n; c += a.G * kWT) {
    double rhs;
    fv_cell_faces(x, c, rhs);
    csum[0] += rhs;
  }
  wide_slot_put(wide_slots(a, par ^ 1), g, 0, csum, lds);
}

// ---- 4. one GEMM of the fast diagonalisation: C[r][c] = sum_k A(r, k) B(k, c) as fv_gemm, one wave per 16 x 16 tile,
//         four tiles per work-group, operands from L2 with zero fill at the edges.  FIRST: B is rhs_p, whose entry 0 is
//         minus the sum the launch before left in the slots.  SCALE: the epilogue / (ax lamx + ay lamy), zero mode dropped.
struct FvWideGemm {
  const double *A, *B;
  double* C;
  int sar, sak, sbk, sbc, M, N, K;
};

// the four GEMMs of a trial: W1 = Qy^T C, W2 = W1 Qx / Lambda, W1 = Qy W2, Y = W1 Qx^T
__host__ __device__ inline FvWideGemm wide_gemm_of(const FvDesc& d, int which) {
  const int nx = d.nx, ny = d.ny;
  const int64_t n = (int64_t)nx * ny;
  double* w = d.work;
  double *Cv = w + FV_C * n, *W1 = w + FV_W1 * n, *W2 = w + FV_W2 * n, *Y = w + FV_Y * n;
  if (which == 0) return {d.Qy, Cv, W1, 1, ny, nx, 1, ny, nx, ny};
  if (which == 1) return {W1, d.Qx, W2, nx, 1, nx, 1, ny, nx, nx};
  if (which == 2) return {d.Qy, W2, W1, ny, 1, nx, 1, ny, nx, ny};
  return {W1, d.Qx, Y, nx, 1, 1, nx, ny, nx, nx};
}

// (gb: the work-group's index among the trial's LDC_FV_WIDE_GEMM_GROUPS)
template <bool FIRST, bool SCALE>
__device__ __forceinline__ void wide_gemm(const FvWideArgs& a, int gb, const FvWideGemm& g, int par, double* lds) {
  if (wide_gate(a)) return;
  double b00 = 0.0;
  if (FIRST) {
    double csum[1];
    wide_slot_sum(wide_slots(a, par), a.G, 0, csum, lds);
    b00 = -csum[0];
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int tn = (g.N + 15) >> 4, tiles = ((g.M + 15) >> 4) * tn;
  const int t = gb * kWW + w;
  if (t >= tiles) return;
  fv_gemm_tile<SCALE, FIRST>(g.A, g.sar, g.sak, g.B, g.sbk, g.sbc, g.C, g.M, g.N, g.K, (t / tn) * 16, (t % tn) * 16, lane,
                             a.d.lamx, a.d.lamy, a.d.dy / a.d.dx, a.d.dx / a.d.dy, b00);
}

// ---- 5. u' = -D grad p', u = u* + u', p += alpha_p p'; record sums 0 .. 6 of this work-group.  The cell body is a copy
//         of fv_correct's in ldc_fv_kernel.inc (ldc_fv_cells.inc, 5.): a change to one goes into the other
__device__ __forceinline__ void wide_correct(const FvWideArgs& a, int g, double* lds) {
  if (wide_gate(a)) return;
  const FvCtx x(a.d);
  const FvDesc& d = x.d;
  const int nx = x.nx, ny = x.ny, n = x.n;
  const double y0 = x.vec(FV_Y)[0];
  double part[7] = {0, 0, 0, 0, 0, 0, 0};
  for (int c = g * kWT + threadIdx.x; c < n; c += a.G * kWT) {
    const int i = c % nx, j = c / nx;
    double gx, gy;
    fv_grad(x.vec(FV_Y), c, i, j, nx, ny, x.dx, x.dy, gx, gy);
    const double D = x.V / (x.w[FV_AP * n + c] + 1e-14);
    const double upc = -D * gx, vpc = -D * gy;
    const double un = x.vec(FV_XU)[c] + upc, vn = x.vec(FV_XV)[c] + vpc, uo = d.u[c], vo = d.v[c];
    const double pp = x.vec(FV_Y)[c] - y0;
    d.p[c] += d.alpha_p * pp;
    d.u[c] = un; d.v[c] = vn; x.vec(FV_UP)[c] = upc; x.vec(FV_VP)[c] = vpc;
    part[0] += (un - uo) * (un - uo); part[1] += uo * uo;
    part[2] += (vn - vo) * (vn - vo); part[3] += vo * vo;
    part[4] += upc * upc; part[5] += vpc * vpc; part[6] += un * un + vn * vn;
  }
  wide_slot_put(wide_rec_slots(a), g, 0, part, lds);
}

// ---- 6. mdot += rho interp(u', v') . S (walls: rho u'_P |S|, FV-Q4); vorticity with ghost cells; record sum 8
__device__ __forceinline__ void wide_fluxvort(const FvWideArgs& a, int g, double* lds) {
  if (wide_gate(a)) return;
  const FvCtx x(a.d);
  double part[1] = {0.0};
  for (int c = g * kWT + threadIdx.x; c < x.n; c += a.G * kWT) fv_cell_flux_vorticity(x, c, part[0]);
  wide_slot_put(wide_rec_slots(a), g, 8, part, lds);
}

// ---- 7a. |div mdot|^2 and |grad omega|^2: record sums 7 and 9
__device__ __forceinline__ void wide_sums(const FvWideArgs& a, int g, double* lds) {
  if (wide_gate(a)) return;
  const FvCtx x(a.d);
  double p7[1] = {0.0}, p9[1] = {0.0};
  for (int c = g * kWT + threadIdx.x; c < x.n; c += a.G * kWT) fv_cell_div_palinstrophy(x, c, p7[0], p9[0]);
  wide_slot_put(wide_rec_slots(a), g, 7, p7, lds);
  wide_slot_put(wide_rec_slots(a), g, 9, p9, lds);
}

// ---- 7b. record (one work-group): the record row, the latch and ctrl[0 .. 5], once per iteration
__device__ __forceinline__ void wide_record(const FvWideArgs& a, double* lds) {
  if (wide_gate(a)) return;
  const FvDesc& d = a.d;
  double part[kWS];
  wide_slot_sum(wide_rec_slots(a), a.G, 0, part, lds);
  const double V = d.dx * d.dy;
  const double rel = fv_rec_rel(part);
  if (threadIdx.x == 0) {
    long long* w = wide_words(a);
    const long long k = w[WW_ROW], iter = d.ctrl[1];
    if (k >= 0 && k < d.rec_cap) fv_rec_row(d.rec + k * LDC_FV_REC_LEN, rel, part, V);
    w[WW_ROW] = k + 1;
    if (rel != rel) d.ctrl[2] = 1;
    else if (iter >= d.warmup && rel < d.tol) d.ctrl[0] = 1;
    d.ctrl[1] = iter + 1;
    d.ctrl[3] += w[WW_GIVEUPS]; d.ctrl[4] += w[WW_LIN_ITERS]; d.ctrl[5] += 2;
  }
}

// ---- 8. Anderson mixing behind `record`, for a trial that has it attached: push | mix | close
#include "ldc_fv_wide_anderson.inc"

// ---- 9. the consistent pressure equation: the launches that replace faces | gemm x 4 and fluxvort
#include "ldc_fv_wide_pressure.inc"

// ---- 10. a lone trial on a wall-clustered grid: the twins of the phases that read the geometry, from per-axis tables
#include "ldc_fv_stretched_cells.inc"
#include "ldc_fv_wide_stretched.inc"

// ---- 11. such a trial with the separable scaled preconditioner: the twins of init, rz, ap and xr
#include "ldc_fv_wide_separable.inc"

// ---- the kernels: every phase for a lone trial (arguments by value, g = blockIdx.x) and for a batch (the table)
#define WIDE_LDS __shared__ double lds[kWW * kWS]
// the trial and the work-group of this block of a batch launch, from a block map / for one work-group per trial
#define WIDE_MAPPED(map)                                   \
  const uint32_t m_ = t.map[blockIdx.x];                   \
  const FvWideArgs a = t.entries[m_ >> 16].a;              \
  const int g = (int)(m_ & 0xffffu)
#define WIDE_SINGLE const FvWideArgs a = t.entries[blockIdx.x].a

__global__ __launch_bounds__(64) void fv_wide_begin(FvWideArgs a, int quota) { wide_begin(a, quota); }
__global__ __launch_bounds__(64) void fv_wide_b_begin(FvWideTable t, FvWideQuotas quotas) {
  WIDE_SINGLE;
  wide_begin(a, quotas.q[blockIdx.x]);
}

__global__ __launch_bounds__(kWT) void fv_wide_assemble(FvWideArgs a, int par) { WIDE_LDS; wide_assemble(a, blockIdx.x, par, lds); }
__global__ __launch_bounds__(kWT) void fv_wide_b_assemble(FvWideTable t, int par) { WIDE_LDS; WIDE_MAPPED(sweep); wide_assemble(a, g, par, lds); }
__global__ __launch_bounds__(kWT) void fv_wide_bicg_p(FvWideArgs a, int it, int par) { WIDE_LDS; wide_bicg_p(a, blockIdx.x, it, par, lds); }
__global__ __launch_bounds__(kWT) void fv_wide_b_bicg_p(FvWideTable t, int it, int par) { WIDE_LDS; WIDE_MAPPED(sweep); wide_bicg_p(a, g, it, par, lds); }
__global__ __launch_bounds__(kWT) void fv_wide_bicg_v(FvWideArgs a, int par) { WIDE_LDS; wide_bicg_v(a, blockIdx.x, par, lds); }
__global__ __launch_bounds__(kWT) void fv_wide_b_bicg_v(FvWideTable t, int par) { WIDE_LDS; WIDE_MAPPED(sweep); wide_bicg_v(a, g, par, lds); }
__global__ __launch_bounds__(kWT) void fv_wide_bicg_s(FvWideArgs a, int par) { WIDE_LDS; wide_bicg_s(a, blockIdx.x, par, lds); }
__global__ __launch_bounds__(kWT) void fv_wide_b_bicg_s(FvWideTable t, int par) { WIDE_LDS; WIDE_MAPPED(sweep); wide_bicg_s(a, g, par, lds); }
__global__ __launch_bounds__(kWT) void fv_wide_bicg_t(FvWideArgs a, int par) { WIDE_LDS; wide_bicg_t(a, blockIdx.x, par, lds); }
__global__ __launch_bounds__(kWT) void fv_wide_b_bicg_t(FvWideTable t, int par) { WIDE_LDS; WIDE_MAPPED(sweep); wide_bicg_t(a, g, par, lds); }
__global__ __launch_bounds__(kWT) void fv_wide_bicg_x(FvWideArgs a, int it, int par) { WIDE_LDS; wide_bicg_x(a, blockIdx.x, it, par, lds); }
__global__ __launch_bounds__(kWT) void fv_wide_b_bicg_x(FvWideTable t, int it, int par) { WIDE_LDS; WIDE_MAPPED(sweep); wide_bicg_x(a, g, it, par, lds); }
__global__ __launch_bounds__(kWT) void fv_wide_linfinish(FvWideArgs a, int nb, int par) { WIDE_LDS; wide_linfinish(a, nb, par, lds); }
__global__ __launch_bounds__(kWT) void fv_wide_b_linfinish(FvWideTable t, int nb, int par) { WIDE_LDS; WIDE_SINGLE; wide_linfinish(a, nb, par, lds); }
__global__ __launch_bounds__(kWT) void fv_wide_faces(FvWideArgs a, int par) { WIDE_LDS; wide_faces(a, blockIdx.x, par, lds); }
__global__ __launch_bounds__(kWT) void fv_wide_b_faces(FvWideTable t, int par) { WIDE_LDS; WIDE_MAPPED(sweep); wide_faces(a, g, par, lds); }
template <bool FIRST, bool SCALE>
__global__ __launch_bounds__(kWT) void fv_wide_gemm(FvWideArgs a, FvWideGemm gd, int par) {
  WIDE_LDS;
  wide_gemm<FIRST, SCALE>(a, blockIdx.x, gd, par, lds);
}
template <bool FIRST, bool SCALE>
__global__ __launch_bounds__(kWT) void fv_wide_b_gemm(FvWideTable t, int which, int par) {
  WIDE_LDS;
  WIDE_MAPPED(gemm);
  wide_gemm<FIRST, SCALE>(a, g, wide_gemm_of(a.d, which), par, lds);
}
__global__ __launch_bounds__(kWT) void fv_wide_correct(FvWideArgs a) { WIDE_LDS; wide_correct(a, blockIdx.x, lds); }
__global__ __launch_bounds__(kWT) void fv_wide_b_correct(FvWideTable t) { WIDE_LDS; WIDE_MAPPED(sweep); wide_correct(a, g, lds); }
__global__ __launch_bounds__(kWT) void fv_wide_fluxvort(FvWideArgs a) { WIDE_LDS; wide_fluxvort(a, blockIdx.x, lds); }
__global__ __launch_bounds__(kWT) void fv_wide_b_fluxvort(FvWideTable t) { WIDE_LDS; WIDE_MAPPED(sweep); wide_fluxvort(a, g, lds); }
__global__ __launch_bounds__(kWT) void fv_wide_sums(FvWideArgs a) { WIDE_LDS; wide_sums(a, blockIdx.x, lds); }
__global__ __launch_bounds__(kWT) void fv_wide_b_sums(FvWideTable t) { WIDE_LDS; WIDE_MAPPED(sweep); wide_sums(a, g, lds); }
__global__ __launch_bounds__(kWT) void fv_wide_record(FvWideArgs a) { WIDE_LDS; wide_record(a, lds); }
__global__ __launch_bounds__(kWT) void fv_wide_b_record(FvWideTable t) { WIDE_LDS; WIDE_SINGLE; wide_record(a, lds); }

__global__ __launch_bounds__(kWT) void fv_wide_mix_push(FvWideArgs a, FvWideMix x) {
  __shared__ double part[kWW][kFvAaSums];
  wide_mix_push(a, x, blockIdx.x, part);
}
__global__ __launch_bounds__(kWT) void fv_wide_b_mix_push(FvWideTable t) {
  __shared__ double part[kWW][kFvAaSums];
  WIDE_MAPPED(sweep);
  wide_mix_push(a, t.entries[m_ >> 16].m, g, part);
}
__global__ __launch_bounds__(kWT) void fv_wide_mix_mix(FvWideArgs a, FvWideMix x) {
  __shared__ WideMixLds s;
  wide_mix_mix(a, x, blockIdx.x, s);
}
__global__ __launch_bounds__(kWT) void fv_wide_b_mix_mix(FvWideTable t) {
  __shared__ WideMixLds s;
  WIDE_MAPPED(sweep);
  wide_mix_mix(a, t.entries[m_ >> 16].m, g, s);
}
__global__ __launch_bounds__(64) void fv_wide_mix_close(FvWideArgs a, FvWideMix x) { wide_mix_close(a, x); }
__global__ __launch_bounds__(64) void fv_wide_b_mix_close(FvWideTable t) {
  WIDE_SINGLE;
  wide_mix_close(a, t.entries[blockIdx.x].m);
}

// the consistent pressure equation.  Lone: the handle's block by value.  Batch: the block of the entry; `faces` and
// `fluxvort` take the reference's body for a reference trial, whose four GEMMs of the exact solve skip the other kind.
#define WIDE_PCG const FvWidePcg& x = t.entries[m_ >> 16].x
__global__ __launch_bounds__(kWT) void fv_wide_pcg_faces(FvWideArgs a, int par) { WIDE_LDS; wide_pcg_faces(a, blockIdx.x, par, lds); }
__global__ __launch_bounds__(kWT) void fv_wide_b_pcg_faces(FvWideTable t, int par) {
  WIDE_LDS;
  WIDE_MAPPED(sweep);
  if (a.pmax) wide_pcg_faces(a, g, par, lds);
  else wide_faces(a, g, par, lds);
}
template <bool FIRST, bool SCALE>
__global__ __launch_bounds__(kWT) void fv_wide_b_pcg_refgemm(FvWideTable t, int which, int par) {
  WIDE_LDS;
  WIDE_MAPPED(gemm);
  if (a.pmax) return;
  wide_gemm<FIRST, SCALE>(a, g, wide_gemm_of(a.d, which), par, lds);
}
__global__ __launch_bounds__(kWT) void fv_wide_pcg_init(FvWideArgs a, int par) { WIDE_LDS; wide_pcg_init(a, blockIdx.x, par, lds); }
__global__ __launch_bounds__(kWT) void fv_wide_b_pcg_init(FvWideTable t, int par) { WIDE_LDS; WIDE_MAPPED(sweep); wide_pcg_init(a, g, par, lds); }
template <bool HEAD, bool SCALE>
__global__ __launch_bounds__(kWT) void fv_wide_pcg_gemm(FvWideArgs a, FvWidePcg x, FvWideGemm gd, int it, int par) {
  WIDE_LDS;
  wide_pcg_gemm<HEAD, SCALE>(a, x, blockIdx.x, gd, it, par, lds);
}
template <bool HEAD, bool SCALE>
__global__ __launch_bounds__(kWT) void fv_wide_b_pcg_gemm(FvWideTable t, int which, int it, int par) {
  WIDE_LDS;
  WIDE_MAPPED(gemm);
  WIDE_PCG;
  wide_pcg_gemm<HEAD, SCALE>(a, x, g, wide_pcg_gemm_of(a.d, which), it, par, lds);
}
__global__ __launch_bounds__(kWT) void fv_wide_pcg_rz(FvWideArgs a, int par) { WIDE_LDS; wide_pcg_rz(a, blockIdx.x, par, lds); }
__global__ __launch_bounds__(kWT) void fv_wide_b_pcg_rz(FvWideTable t, int par) { WIDE_LDS; WIDE_MAPPED(sweep); wide_pcg_rz(a, g, par, lds); }
__global__ __launch_bounds__(kWT) void fv_wide_pcg_ap(FvWideArgs a, int it, int par) { WIDE_LDS; wide_pcg_ap(a, blockIdx.x, it, par, lds); }
__global__ __launch_bounds__(kWT) void fv_wide_b_pcg_ap(FvWideTable t, int it, int par) { WIDE_LDS; WIDE_MAPPED(sweep); wide_pcg_ap(a, g, it, par, lds); }
__global__ __launch_bounds__(kWT) void fv_wide_pcg_xr(FvWideArgs a, int it, int par) { WIDE_LDS; wide_pcg_xr(a, blockIdx.x, it, par, lds); }
__global__ __launch_bounds__(kWT) void fv_wide_b_pcg_xr(FvWideTable t, int it, int par) { WIDE_LDS; WIDE_MAPPED(sweep); wide_pcg_xr(a, g, it, par, lds); }
__global__ __launch_bounds__(kWT) void fv_wide_pcg_finish(FvWideArgs a, FvWidePcg x, int nb, int par) { WIDE_LDS; wide_pcg_finish(a, x, nb, par, lds); }
__global__ __launch_bounds__(kWT) void fv_wide_b_pcg_finish(FvWideTable t, int nb, int par) {
  WIDE_LDS;
  WIDE_SINGLE;
  wide_pcg_finish(a, t.entries[blockIdx.x].x, nb, par, lds);
}
__global__ __launch_bounds__(kWT) void fv_wide_pcg_fluxvort(FvWideArgs a) { WIDE_LDS; wide_pcg_fluxvort(a, blockIdx.x, lds); }
__global__ __launch_bounds__(kWT) void fv_wide_b_pcg_fluxvort(FvWideTable t) {
  WIDE_LDS;
  WIDE_MAPPED(sweep);
  if (a.pmax) wide_pcg_fluxvort(a, g, lds);
  else wide_fluxvort(a, g, lds);
}

std::mutex g_wide_mutex;
hipStream_t g_wide_stream[64] = {};

// this unit's private non-blocking stream of the current device (call with g_wide_mutex held)
hipError_t wide_stream(hipStream_t* out) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (dev < 0 || dev >= 64) return hipErrorInvalidDevice;
  if (g_wide_stream[dev] == nullptr) {
    e = hipStreamCreateWithFlags(&g_wide_stream[dev], hipStreamNonBlocking);
    if (e != hipSuccess) return e;
  }
  *out = g_wide_stream[dev];
  return hipSuccess;
}

// a small synchronous copy on that stream (off the legacy stream, as the library's other status reads)
hipError_t wide_copy_now(void* dst, const void* src, size_t bytes, hipMemcpyKind kind = hipMemcpyDeviceToHost) {
  std::lock_guard<std::mutex> lock(g_wide_mutex);
  hipStream_t st = nullptr;
  hipError_t e = wide_stream(&st);
  if (e != hipSuccess) return e;
  e = hipMemcpyAsync(dst, src, bytes, kind, st);
  const hipError_t w = hipStreamSynchronize(st);
  return e != hipSuccess ? e : w;
}

// the captured iterations of a handle, lone or batch: (BiCGSTAB iterations | CG iterations << 16, the iteration's graph),
// kept until destroy
struct WideGraphs {
  std::vector<std::pair<int, hipGraphExec_t>> graphs;
  hipEvent_t done = nullptr;                 // behind the last graph launch: no graph is destroyed in flight
};

}  // namespace

struct ldc_fv_wide {
  FvWideArgs a;
  int device;
  signed char graph;                         // replay ONE captured iteration per budget (ldc_fv_wide_set_graph)
  signed char grid_mode;                     // LDC_FV_GRID_*: tables attached (ldc_fv_wide_set_grid), `grid` below in use.
                                             // In the head, in what was the high byte of `graph`: the calls that refuse a
                                             // handle with tables read nothing behind the first 216 bytes of one without
  short mixing;                              // the iteration ends on the mixing chain (m.depth > 0).  Here, not in `m`:
                                             // ldc_fv_wide_launches reads nothing behind these first 216 bytes
  FvWideMix m;                               // ldc_fv_wide_set_anderson; all zero: no mixing
  WideGraphs gs;
  FvWidePcg x;                               // ldc_fv_wide_set_pressure (a.pmax > 0: in use).  Behind gs: nothing in front
  int pbudget;                               // of it moves, and only a handle with a.pmax > 0 is read this far
  FvGridBlk grid;                            // ldc_fv_wide_set_grid.  At the end, for the same reason: only a handle with
                                             // grid_mode LDC_FV_GRID_TABLES is read this far
  FvPrecondBlk prec;                         // ldc_fv_wide_set_preconditioner.  Behind `grid`, and only such a handle is read
  int prec_mode;                             // this far: prec_mode != LDC_FV_PRECOND_LAPLACIAN implies grid_mode TABLES
};
static_assert(LDC_FV_PRECOND_LAPLACIAN == 0, "a handle made of zeroes has the laplacian preconditioner");
static_assert(sizeof(ldc_fv_wide) <= 512, "a handle with tables ends within 512 bytes");
static_assert(LDC_FV_GRID_UNIFORM == 0, "a handle made of zeroes has the uniform grid");
static_assert(sizeof(FvWideArgs) + sizeof(int) + 2 * sizeof(signed char) + sizeof(short) == 216, "the head of a handle");

struct ldc_fv_wide_batch {
  int n, maxit, device, graph;               // (the head, with rec_cap, is all that validation without a device reads)
  int rec_cap[LDC_FV_WIDE_BATCH_MAX];
  int sweep_groups, gemm_groups;             // work-groups of a cell sweep and of a GEMM launch
  int mixing;                                // some trial has mixing attached: every chain ends on the mixing launches
  int pressure;                              // some trial has the consistent pressure equation: the chain carries both kinds
  FvWideTable t;                             // (pointers into the caller's device buffer)
  WideGraphs gs;
  int pmax, pbudget;                         // pressure_max_iters of those trials (one value), the CG launches of an enqueue
};

namespace {

#define WIDE_LAUNCH(kernel, grid, block, ...)                                        \
  do {                                                                               \
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, st, __VA_ARGS__);         \
    const hipError_t e_ = hipGetLastError();                                         \
    if (e_ != hipSuccess) return (int)e_;                                            \
  } while (0)

// the launches of ONE iteration with `nb` BiCGSTAB iterations and, for a trial with the consistent pressure equation, `np`
// CG iterations; `par` alternates launch by launch
int wide_sg_iteration(const ldc_fv_wide* h, int nb, int np, hipStream_t st);

int wide_iteration(const ldc_fv_wide* h, int nb, int np, hipStream_t st) {
  if (h->grid_mode == LDC_FV_GRID_TABLES) return wide_sg_iteration(h, nb, np, st);
  const FvWideArgs& a = h->a;
  const FvDesc& d = a.d;
  const int G = a.G, gg = (int)LDC_FV_WIDE_GEMM_GROUPS(d.nx, d.ny);
  int par = 0;
  WIDE_LAUNCH(fv_wide_assemble, G, kWT, a, par); par ^= 1;
  for (int it = 0; it < nb; ++it) {
    WIDE_LAUNCH(fv_wide_bicg_p, G, kWT, a, it, par); par ^= 1;
    WIDE_LAUNCH(fv_wide_bicg_v, G, kWT, a, par); par ^= 1;
    WIDE_LAUNCH(fv_wide_bicg_s, G, kWT, a, par); par ^= 1;
    WIDE_LAUNCH(fv_wide_bicg_t, G, kWT, a, par); par ^= 1;
    WIDE_LAUNCH(fv_wide_bicg_x, G, kWT, a, it, par); par ^= 1;
  }
  WIDE_LAUNCH(fv_wide_linfinish, 1, kWT, a, nb, par); par ^= 1;
  if (a.pmax == 0) {
    WIDE_LAUNCH(fv_wide_faces, G, kWT, a, par); par ^= 1;
    WIDE_LAUNCH((fv_wide_gemm<true, false>), gg, kWT, a, wide_gemm_of(d, 0), par);
    WIDE_LAUNCH((fv_wide_gemm<false, true>), gg, kWT, a, wide_gemm_of(d, 1), par);
    WIDE_LAUNCH((fv_wide_gemm<false, false>), gg, kWT, a, wide_gemm_of(d, 2), par);
    WIDE_LAUNCH((fv_wide_gemm<false, false>), gg, kWT, a, wide_gemm_of(d, 3), par);
    WIDE_LAUNCH(fv_wide_correct, G, kWT, a);
    WIDE_LAUNCH(fv_wide_fluxvort, G, kWT, a);
  } else {
    const FvWidePcg& x = h->x;
    WIDE_LAUNCH(fv_wide_pcg_faces, G, kWT, a, par); par ^= 1;
    WIDE_LAUNCH(fv_wide_pcg_init, G, kWT, a, par); par ^= 1;
    for (int it = 0; it < np; ++it) {
      WIDE_LAUNCH((fv_wide_pcg_gemm<true, false>), gg, kWT, a, x, wide_pcg_gemm_of(d, 0), it, par); par ^= 1;
      WIDE_LAUNCH((fv_wide_pcg_gemm<false, true>), gg, kWT, a, x, wide_pcg_gemm_of(d, 1), it, par);
      WIDE_LAUNCH((fv_wide_pcg_gemm<false, false>), gg, kWT, a, x, wide_pcg_gemm_of(d, 2), it, par);
      WIDE_LAUNCH((fv_wide_pcg_gemm<false, false>), gg, kWT, a, x, wide_pcg_gemm_of(d, 3), it, par);
      WIDE_LAUNCH(fv_wide_pcg_rz, G, kWT, a, par); par ^= 1;
      WIDE_LAUNCH(fv_wide_pcg_ap, G, kWT, a, it, par); par ^= 1;
      WIDE_LAUNCH(fv_wide_pcg_xr, G, kWT, a, it, par); par ^= 1;
    }
    WIDE_LAUNCH(fv_wide_pcg_finish, 1, kWT, a, x, np, par);
    WIDE_LAUNCH(fv_wide_correct, G, kWT, a);
    WIDE_LAUNCH(fv_wide_pcg_fluxvort, G, kWT, a);
  }
  WIDE_LAUNCH(fv_wide_sums, G, kWT, a);
  WIDE_LAUNCH(fv_wide_record, 1, kWT, a);
  if (h->mixing) {
    WIDE_LAUNCH(fv_wide_mix_push, G, kWT, a, h->m);
    WIDE_LAUNCH(fv_wide_mix_mix, G, kWT, a, h->m);
    WIDE_LAUNCH(fv_wide_mix_close, 1, 64, a, h->m);
  }
  return 0;
}

// the same chain for a lone trial with geometry tables (ldc_fv_wide_set_grid; ldc_fv_wide_stretched.inc): launch for launch
// the chain above, in the same grids and with the same `par`; the phases that read the geometry are their stretched twins,
// and the scaled GEMM and `record` take the arguments with dx = dy = 1.  (No mixing chain: ldc_fv_wide_set_grid and
// ldc_fv_wide_set_anderson refuse the combination.)
int wide_sg_iteration(const ldc_fv_wide* h, int nb, int np, hipStream_t st) {
  const FvWideArgs& a = h->a;
  const FvWideArgs a1 = wide_sg_neutral(a);
  const FvGridBlk& gb = h->grid;
  const FvDesc& d = a.d;
  const int G = a.G, gg = (int)LDC_FV_WIDE_GEMM_GROUPS(d.nx, d.ny);
  int par = 0;
  WIDE_LAUNCH(fv_wide_sg_assemble, G, kWT, a, gb, par); par ^= 1;
  for (int it = 0; it < nb; ++it) {
    WIDE_LAUNCH(fv_wide_bicg_p, G, kWT, a, it, par); par ^= 1;
    WIDE_LAUNCH(fv_wide_bicg_v, G, kWT, a, par); par ^= 1;
    WIDE_LAUNCH(fv_wide_bicg_s, G, kWT, a, par); par ^= 1;
    WIDE_LAUNCH(fv_wide_bicg_t, G, kWT, a, par); par ^= 1;
    WIDE_LAUNCH(fv_wide_bicg_x, G, kWT, a, it, par); par ^= 1;
  }
  WIDE_LAUNCH(fv_wide_linfinish, 1, kWT, a, nb, par); par ^= 1;
  if (a.pmax == 0) {
    WIDE_LAUNCH((fv_wide_sg_faces<false>), G, kWT, a, gb, par); par ^= 1;
    WIDE_LAUNCH((fv_wide_gemm<true, false>), gg, kWT, a, wide_gemm_of(d, 0), par);
    WIDE_LAUNCH((fv_wide_gemm<false, true>), gg, kWT, a1, wide_gemm_of(d, 1), par);
    WIDE_LAUNCH((fv_wide_gemm<false, false>), gg, kWT, a, wide_gemm_of(d, 2), par);
    WIDE_LAUNCH((fv_wide_gemm<false, false>), gg, kWT, a, wide_gemm_of(d, 3), par);
    WIDE_LAUNCH(fv_wide_sg_correct, G, kWT, a, gb);
    WIDE_LAUNCH((fv_wide_sg_fluxvort<false>), G, kWT, a, gb);
  } else {
    const FvWidePcg& x = h->x;
    WIDE_LAUNCH((fv_wide_sg_faces<true>), G, kWT, a, gb, par); par ^= 1;
    if (h->prec_mode == LDC_FV_PRECOND_SEPARABLE) {       // (ldc_fv_wide_separable.inc: the same launches, z = s . L_s+ (s . r))
      const FvPrecondBlk& pb = h->prec;
      const FvWideArgs as = wide_sep_args(a, pb);
      const FvDesc& ds = as.d;
      WIDE_LAUNCH(fv_wide_sep_init, G, kWT, a, gb, pb, par); par ^= 1;
      for (int it = 0; it < np; ++it) {
        WIDE_LAUNCH((fv_wide_pcg_gemm<true, false>), gg, kWT, as, x, wide_sep_gemm_of(ds, 0), it, par); par ^= 1;
        WIDE_LAUNCH((fv_wide_pcg_gemm<false, true>), gg, kWT, as, x, wide_sep_gemm_of(ds, 1), it, par);
        WIDE_LAUNCH((fv_wide_pcg_gemm<false, false>), gg, kWT, as, x, wide_sep_gemm_of(ds, 2), it, par);
        WIDE_LAUNCH((fv_wide_pcg_gemm<false, false>), gg, kWT, as, x, wide_sep_gemm_of(ds, 3), it, par);
        WIDE_LAUNCH(fv_wide_sep_rz, G, kWT, a, par); par ^= 1;
        WIDE_LAUNCH(fv_wide_sep_ap, G, kWT, a, gb, it, par); par ^= 1;
        WIDE_LAUNCH(fv_wide_sep_xr, G, kWT, a, it, par); par ^= 1;
      }
    } else {
      WIDE_LAUNCH(fv_wide_pcg_init, G, kWT, a, par); par ^= 1;
      for (int it = 0; it < np; ++it) {
        WIDE_LAUNCH((fv_wide_pcg_gemm<true, false>), gg, kWT, a, x, wide_pcg_gemm_of(d, 0), it, par); par ^= 1;
        WIDE_LAUNCH((fv_wide_pcg_gemm<false, true>), gg, kWT, a1, x, wide_pcg_gemm_of(d, 1), it, par);
        WIDE_LAUNCH((fv_wide_pcg_gemm<false, false>), gg, kWT, a, x, wide_pcg_gemm_of(d, 2), it, par);
        WIDE_LAUNCH((fv_wide_pcg_gemm<false, false>), gg, kWT, a, x, wide_pcg_gemm_of(d, 3), it, par);
        WIDE_LAUNCH(fv_wide_pcg_rz, G, kWT, a, par); par ^= 1;
        WIDE_LAUNCH(fv_wide_sg_pcg_ap, G, kWT, a, gb, it, par); par ^= 1;
        WIDE_LAUNCH(fv_wide_pcg_xr, G, kWT, a, it, par); par ^= 1;
      }
    }
    WIDE_LAUNCH(fv_wide_pcg_finish, 1, kWT, a, x, np, par);
    WIDE_LAUNCH(fv_wide_sg_correct, G, kWT, a, gb);
    WIDE_LAUNCH((fv_wide_sg_fluxvort<true>), G, kWT, a, gb);
  }
  WIDE_LAUNCH(fv_wide_sg_sums, G, kWT, a, gb);
  WIDE_LAUNCH(fv_wide_record, 1, kWT, a1);
  return 0;
}

// the same chain for all trials of a batch: every launch carries the work-groups of all of them.  With a trial of either
// kind of pressure equation in it the chain has the launches of both, and a trial returns from those of the other kind.
int wide_iteration(const ldc_fv_wide_batch* b, int nb, int np, hipStream_t st) {
  const FvWideTable& t = b->t;
  const int G = b->sweep_groups, gg = b->gemm_groups, n = b->n;
  int par = 0;
  WIDE_LAUNCH(fv_wide_b_assemble, G, kWT, t, par); par ^= 1;
  for (int it = 0; it < nb; ++it) {
    WIDE_LAUNCH(fv_wide_b_bicg_p, G, kWT, t, it, par); par ^= 1;
    WIDE_LAUNCH(fv_wide_b_bicg_v, G, kWT, t, par); par ^= 1;
    WIDE_LAUNCH(fv_wide_b_bicg_s, G, kWT, t, par); par ^= 1;
    WIDE_LAUNCH(fv_wide_b_bicg_t, G, kWT, t, par); par ^= 1;
    WIDE_LAUNCH(fv_wide_b_bicg_x, G, kWT, t, it, par); par ^= 1;
  }
  WIDE_LAUNCH(fv_wide_b_linfinish, n, kWT, t, nb, par); par ^= 1;
  if (!b->pressure) {
    WIDE_LAUNCH(fv_wide_b_faces, G, kWT, t, par); par ^= 1;
    WIDE_LAUNCH((fv_wide_b_gemm<true, false>), gg, kWT, t, 0, par);
    WIDE_LAUNCH((fv_wide_b_gemm<false, true>), gg, kWT, t, 1, par);
    WIDE_LAUNCH((fv_wide_b_gemm<false, false>), gg, kWT, t, 2, par);
    WIDE_LAUNCH((fv_wide_b_gemm<false, false>), gg, kWT, t, 3, par);
    WIDE_LAUNCH(fv_wide_b_correct, G, kWT, t);
    WIDE_LAUNCH(fv_wide_b_fluxvort, G, kWT, t);
  } else {
    WIDE_LAUNCH(fv_wide_b_pcg_faces, G, kWT, t, par); par ^= 1;
    WIDE_LAUNCH((fv_wide_b_pcg_refgemm<true, false>), gg, kWT, t, 0, par);
    WIDE_LAUNCH((fv_wide_b_pcg_refgemm<false, true>), gg, kWT, t, 1, par);
    WIDE_LAUNCH((fv_wide_b_pcg_refgemm<false, false>), gg, kWT, t, 2, par);
    WIDE_LAUNCH((fv_wide_b_pcg_refgemm<false, false>), gg, kWT, t, 3, par);
    WIDE_LAUNCH(fv_wide_b_pcg_init, G, kWT, t, par); par ^= 1;
    for (int it = 0; it < np; ++it) {
      WIDE_LAUNCH((fv_wide_b_pcg_gemm<true, false>), gg, kWT, t, 0, it, par); par ^= 1;
      WIDE_LAUNCH((fv_wide_b_pcg_gemm<false, true>), gg, kWT, t, 1, it, par);
      WIDE_LAUNCH((fv_wide_b_pcg_gemm<false, false>), gg, kWT, t, 2, it, par);
      WIDE_LAUNCH((fv_wide_b_pcg_gemm<false, false>), gg, kWT, t, 3, it, par);
      WIDE_LAUNCH(fv_wide_b_pcg_rz, G, kWT, t, par); par ^= 1;
      WIDE_LAUNCH(fv_wide_b_pcg_ap, G, kWT, t, it, par); par ^= 1;
      WIDE_LAUNCH(fv_wide_b_pcg_xr, G, kWT, t, it, par); par ^= 1;
    }
    WIDE_LAUNCH(fv_wide_b_pcg_finish, n, kWT, t, np, par);
    WIDE_LAUNCH(fv_wide_b_correct, G, kWT, t);
    WIDE_LAUNCH(fv_wide_b_pcg_fluxvort, G, kWT, t);
  }
  WIDE_LAUNCH(fv_wide_b_sums, G, kWT, t);
  WIDE_LAUNCH(fv_wide_b_record, n, kWT, t);
  if (b->mixing) {
    WIDE_LAUNCH(fv_wide_b_mix_push, G, kWT, t);
    WIDE_LAUNCH(fv_wide_b_mix_mix, G, kWT, t);
    WIDE_LAUNCH(fv_wide_b_mix_close, n, 64, t);
  }
  return 0;
}

// Budgets above this are launched one by one: the graph of an iteration has 11 + 5 nb nodes (and the mixing chain's, and
// 7 np of the consistent pressure equation, whose budget has the same bound)
constexpr int kWideGraphMaxNb = 64;

// The graph of ONE iteration of `h` (a lone handle or a batch) with nb BiCGSTAB iterations: a linear chain captured on
// this unit's private stream (relaxed mode: kernel launches only, no call elsewhere needs to be prohibited meanwhile),
// instantiated once and kept.
template <class Handle>
int wide_graph(Handle* h, int nb, int np, hipGraphExec_t* out) {
  const int key = nb | np << 16;
  for (const auto& g : h->gs.graphs)
    if (g.first == key) { *out = g.second; return 0; }
  std::lock_guard<std::mutex> lock(g_wide_mutex);
  hipStream_t cs = nullptr;
  hipError_t e = wide_stream(&cs);
  if (e != hipSuccess) return (int)e;
  e = hipStreamBeginCapture(cs, hipStreamCaptureModeRelaxed);
  if (e != hipSuccess) return (int)e;
  const int rc = wide_iteration(h, nb, np, cs);
  hipGraph_t g = nullptr;
  const hipError_t ce = hipStreamEndCapture(cs, &g);
  if (rc != 0 || ce != hipSuccess) {
    if (g) (void)hipGraphDestroy(g);
    return rc != 0 ? rc : (int)ce;
  }
  hipGraphExec_t exec = nullptr;
  const hipError_t ie = hipGraphInstantiate(&exec, g, nullptr, nullptr, 0);
  (void)hipGraphDestroy(g);
  if (ie != hipSuccess) return (int)ie;
  h->gs.graphs.emplace_back(key, exec);
  *out = exec;
  return 0;
}

// `chains` iterations of `h` at nb BiCGSTAB iterations (and np CG iterations) each on `st`, behind the `begin` launch the
// caller has made: the handle's graph replayed, or every kernel on its own
template <class Handle>
int wide_chains(Handle* h, int chains, int nb, int np, hipStream_t st) {
  hipGraphExec_t exec = nullptr;
  if (h->graph && nb <= kWideGraphMaxNb && np <= kWideGraphMaxNb) {
    const int rc = wide_graph(h, nb, np, &exec);
    if (rc != 0) return rc;
    if (!h->gs.done) {
      const hipError_t e = hipEventCreateWithFlags(&h->gs.done, hipEventDisableTiming);
      if (e != hipSuccess) return (int)e;
    }
  }
  for (int k = 0; k < chains; ++k) {
    if (exec) {
      const hipError_t e = hipGraphLaunch(exec, st);
      if (e != hipSuccess) return (int)e;
    } else {
      const int rc = wide_iteration(h, nb, np, st);
      if (rc != 0) return rc;
    }
  }
  if (exec) {
    const hipError_t e = hipEventRecord(h->gs.done, st);
    if (e != hipSuccess) return (int)e;
  }
  return 0;
}

// destroy, and a new mixing block (the graphs hold the old one by value): wait for the last replay, then free the graphs.
// A handle that has captured nothing makes no device call here.
void wide_graphs_free(WideGraphs& gs) {
  if (gs.done) {
    (void)hipEventSynchronize(gs.done);
    (void)hipEventDestroy(gs.done);
    gs.done = nullptr;
  }
  for (const auto& g : gs.graphs) (void)hipGraphExecDestroy(g.second);
  gs.graphs.clear();
}

// the CG iterations an enqueue of `h` carries per SIMPLE iteration (0: no trial with the consistent pressure equation)
inline int wide_np(const ldc_fv_wide* h) { return h->a.pmax == 0 ? 0 : (h->pbudget < h->a.pmax ? h->pbudget : h->a.pmax); }
inline int wide_np(const ldc_fv_wide_batch* b) { return !b->pressure ? 0 : (b->pbudget < b->pmax ? b->pbudget : b->pmax); }
inline int wide_lin(int lin_budget, int maxit) { return lin_budget < maxit ? lin_budget : maxit; }

}  // namespace

extern "C" {

int ldc_fv_wide_create(const struct ldc_fv_problem* pr, double* scratch, int64_t scratch_len, ldc_fv_wide** out) {
  if (!pr || !out) return LDC_E_ARG;
  *out = nullptr;
  FvDesc h;
  const int rc = fv_desc_of(pr, LDC_FV_WIDE_MAX_N, &h);
  if (rc != 0) return rc;
  if (!scratch) return LDC_E_ARG;
  if (scratch_len < LDC_FV_WIDE_SCRATCH_LEN(pr->nx, pr->ny)) return LDC_E_ARG;
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) return LDC_E_NODEVICE;
  ldc_fv_wide* s = new (std::nothrow) ldc_fv_wide;
  if (!s) return LDC_E_STATE;
  s->a.d = h;
  s->a.scr = scratch;
  s->a.G = (int)LDC_FV_WIDE_GROUPS(pr->nx, pr->ny);
  s->a.pmax = 0;
  s->x = FvWidePcg{};
  s->pbudget = LDC_FV_WIDE_PRESSURE_BUDGET_DEFAULT;
  s->device = dev;
  s->graph = LDC_FV_WIDE_GRAPH_DEFAULT;
  s->mixing = 0;
  s->m = FvWideMix{};
  s->grid = FvGridBlk{};
  s->grid_mode = LDC_FV_GRID_UNIFORM;
  s->prec = FvPrecondBlk{};
  s->prec_mode = LDC_FV_PRECOND_LAPLACIAN;
  *out = s;
  return 0;
}

int ldc_fv_wide_destroy(ldc_fv_wide* h) {
  if (!h) return LDC_E_STATE;
  wide_graphs_free(h->gs);
  delete h;
  return 0;
}

int ldc_fv_wide_set_graph(ldc_fv_wide* h, int on) {
  if (!h) return LDC_E_STATE;
  if (on != 0 && on != 1) return LDC_E_ARG;
  h->graph = (signed char)on;
  return 0;
}

int ldc_fv_wide_set_anderson(ldc_fv_wide* h, const struct ldc_fv_anderson* acc, double* scratch, int64_t scratch_len) {
  if (!h) return LDC_E_STATE;
  FvWideMix m = {};
  if (acc) {
    if (acc->depth < 0 || acc->depth > LDC_FV_ANDERSON_MAX_DEPTH || acc->start < 1 || !acc->astate) return LDC_E_ARG;
    if (acc->depth > 0) {
      const int nx = h->a.d.nx, ny = h->a.d.ny;
      if (!acc->hist || acc->hist_len < LDC_FV_ANDERSON_HIST_LEN(nx, ny, acc->depth)) return LDC_E_ARG;
      if (!scratch || scratch_len < LDC_FV_WIDE_ANDERSON_SCRATCH_LEN(nx, ny, acc->depth)) return LDC_E_ARG;
      if (h->grid_mode == LDC_FV_GRID_TABLES) return LDC_E_ARG;             // (the mixing has not met a stretched trial)
      m.hist = acc->hist;
      m.astate = reinterpret_cast<long long*>(acc->astate);
      m.mscr = scratch;
      m.depth = acc->depth;
      m.start = acc->start;
    }
  }
  wide_graphs_free(h->gs);
  h->m = m;
  h->mixing = m.depth > 0 ? 1 : 0;
  return 0;
}

int ldc_fv_wide_set_pressure(ldc_fv_wide* h, const struct ldc_fv_pressure* cfg, double* scratch, int64_t scratch_len) {
  if (!h) return LDC_E_STATE;
  int pmax = 0;
  FvWidePcg x = {};
  if (cfg && cfg->mode != LDC_FV_PRESSURE_REFERENCE) {
    if (cfg->mode != LDC_FV_PRESSURE_CONSISTENT || cfg->max_iters < 1 || !(cfg->tol > 0 && cfg->tol < 1)) return LDC_E_ARG;
    if (!scratch || scratch_len < LDC_FV_WIDE_PRESSURE_SCRATCH_LEN) return LDC_E_ARG;
    pmax = cfg->max_iters;
    x.tol = cfg->tol;
    x.stats = reinterpret_cast<long long*>(scratch);
  }
  if (h->a.pmax == 0 && pmax == 0) return 0;                // (a plain handle stays as it is, and as short as it is)
  wide_graphs_free(h->gs);
  h->a.pmax = pmax;
  h->x = x;
  return 0;
}

int ldc_fv_wide_set_grid(ldc_fv_wide* h, const struct ldc_fv_grid* grid) {
  if (!h) return LDC_E_ARG;
  FvGridBlk blk = {};
  int mode = LDC_FV_GRID_UNIFORM;
  if (grid && grid->mode != LDC_FV_GRID_UNIFORM) {
    if (grid->mode != LDC_FV_GRID_TABLES || !grid->x_tables || !grid->y_tables) return LDC_E_ARG;
    if (grid->x_len < LDC_FV_GRID_TABLE_LEN(h->a.d.nx) || grid->y_len < LDC_FV_GRID_TABLE_LEN(h->a.d.ny)) return LDC_E_ARG;
    if (h->mixing) return LDC_E_ARG;                        // (the mixing has not met a stretched trial)
    blk.ax = grid->x_tables;
    blk.ay = grid->y_tables;
    mode = LDC_FV_GRID_TABLES;
  }
  if (mode == LDC_FV_GRID_UNIFORM && h->grid_mode == LDC_FV_GRID_UNIFORM) return 0;   // (a plain handle stays as short as it is)
  wide_graphs_free(h->gs);
  h->grid = blk;
  h->grid_mode = (signed char)mode;
  h->prec = FvPrecondBlk{};                                 // (the tables belong to the mesh they were fitted to)
  h->prec_mode = LDC_FV_PRECOND_LAPLACIAN;
  return 0;
}

int ldc_fv_wide_set_preconditioner(ldc_fv_wide* h, const struct ldc_fv_precond* cfg) {
  if (!h) return LDC_E_ARG;
  FvPrecondBlk blk = {};
  int mode = LDC_FV_PRECOND_LAPLACIAN;
  if (cfg && cfg->mode != LDC_FV_PRECOND_LAPLACIAN) {
    if (cfg->mode != LDC_FV_PRECOND_SEPARABLE || h->grid_mode != LDC_FV_GRID_TABLES) return LDC_E_ARG;
    if (!cfg->x_table || !cfg->y_table) return LDC_E_ARG;
    if (cfg->x_len < LDC_FV_PRECOND_TABLE_LEN(h->a.d.nx) || cfg->y_len < LDC_FV_PRECOND_TABLE_LEN(h->a.d.ny)) return LDC_E_ARG;
    blk.px = cfg->x_table;
    blk.py = cfg->y_table;
    mode = LDC_FV_PRECOND_SEPARABLE;
  }
  if (h->grid_mode != LDC_FV_GRID_TABLES) return 0;         // (laplacian already, and a plain handle stays as short as it is)
  wide_graphs_free(h->gs);
  h->prec = blk;
  h->prec_mode = mode;
  return 0;
}

int ldc_fv_wide_set_pressure_budget(ldc_fv_wide* h, int budget) {
  if (!h) return LDC_E_STATE;
  if (budget < 1 || h->a.pmax == 0) return LDC_E_ARG;
  h->pbudget = budget;
  return 0;
}

int ldc_fv_wide_enqueue(ldc_fv_wide* h, int n_iters, int lin_budget, void* stream) {
  if (!h) return LDC_E_STATE;
  if (n_iters < 1 || n_iters > h->a.d.rec_cap || lin_budget < 1) return LDC_E_ARG;
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) return LDC_E_NODEVICE;
  if (dev != h->device) return LDC_E_STATE;
  hipStream_t st = as_stream(stream);
  WIDE_LAUNCH(fv_wide_begin, 1, 64, h->a, n_iters);
  return wide_chains(h, n_iters, wide_lin(lin_budget, h->a.d.maxit), wide_np(h), st);
}

int ldc_fv_wide_launches(const ldc_fv_wide* h, int lin_budget) {
  if (!h || lin_budget < 1) return LDC_E_ARG;
  return 11 + 5 * wide_lin(lin_budget, h->a.d.maxit) + (h->mixing ? kWideMixLaunches : 0)
         + (h->a.pmax ? 2 - 4 + kWidePcgLaunches * wide_np(h) : 0);      // init and pfinish come, the exact solve's GEMMs go
}

int ldc_fv_wide_status(ldc_fv_wide* h) {
  if (!h) return LDC_E_STATE;
  long long nan_flag = 0, ovf = 0;
  hipError_t e = wide_copy_now(&nan_flag, h->a.d.ctrl + 2, sizeof(nan_flag));
  if (e != hipSuccess) return (int)e;
  e = wide_copy_now(&ovf, reinterpret_cast<long long*>(h->a.scr) + WW_OVF, sizeof(ovf));
  if (e != hipSuccess) return (int)e;
  return nan_flag ? LDC_FV_E_NAN : (ovf ? LDC_FV_WIDE_E_BUDGET : 0);
}

int ldc_fv_wide_batch_create(ldc_fv_wide* const* hs, int n, void* table, int64_t table_len, ldc_fv_wide_batch** out) {
  if (!out) return LDC_E_ARG;
  *out = nullptr;
  if (!hs || n < 1 || n > LDC_FV_WIDE_BATCH_MAX || !table) return LDC_E_ARG;
  for (int q = 0; q < n; ++q)
    if (!hs[q]) return LDC_E_STATE;
  int64_t sweep = 0, gemm = 0;
  int pmax = 0;                               // pressure_max_iters of the trials with the consistent equation: one value
  for (int q = 0; q < n; ++q) {
    for (int r = 0; r < q; ++r)
      if (hs[r] == hs[q]) return LDC_E_ARG;
    if (hs[q]->a.d.maxit != hs[0]->a.d.maxit) return LDC_E_ARG;
    if (hs[q]->grid_mode != LDC_FV_GRID_UNIFORM) return LDC_E_ARG;         // (the kernels of a batch assume equal spacing)
    if (hs[q]->a.pmax) {
      if (pmax && hs[q]->a.pmax != pmax) return LDC_E_ARG;
      pmax = hs[q]->a.pmax;
    }
    sweep += hs[q]->a.G;
    gemm += LDC_FV_WIDE_GEMM_GROUPS(hs[q]->a.d.nx, hs[q]->a.d.ny);
  }
  if (table_len < LDC_FV_WIDE_BATCH_TABLE_LEN(n, sweep, gemm)) return LDC_E_ARG;
  for (int q = 1; q < n; ++q)
    if (hs[q]->device != hs[0]->device) return LDC_E_STATE;
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) return LDC_E_NODEVICE;
  if (dev != hs[0]->device) return LDC_E_STATE;
  ldc_fv_wide_batch* b = new (std::nothrow) ldc_fv_wide_batch;
  if (!b) return LDC_E_STATE;
  b->n = n; b->maxit = hs[0]->a.d.maxit; b->device = dev; b->graph = LDC_FV_WIDE_GRAPH_DEFAULT;
  b->sweep_groups = (int)sweep; b->gemm_groups = (int)gemm; b->mixing = 0;
  b->pressure = 0; b->pmax = pmax; b->pbudget = LDC_FV_WIDE_PRESSURE_BUDGET_DEFAULT;
  // the image of the table: entries, the block map of the sweeps, that of the GEMMs
  std::vector<char> image((size_t)LDC_FV_WIDE_BATCH_TABLE_LEN(n, sweep, gemm), 0);
  FvWideEntry* entries = reinterpret_cast<FvWideEntry*>(image.data());
  uint32_t* smap = reinterpret_cast<uint32_t*>(image.data() + sizeof(FvWideEntry) * (size_t)n);
  uint32_t* gmap = smap + sweep;
  for (int q = 0; q < n; ++q) {
    entries[q].a = hs[q]->a;
    entries[q].m = hs[q]->m;
    if (hs[q]->mixing) b->mixing = 1;
    if (hs[q]->a.pmax) { entries[q].x = hs[q]->x; b->pressure = 1; }
    b->rec_cap[q] = hs[q]->a.d.rec_cap;
    const int gq = (int)LDC_FV_WIDE_GEMM_GROUPS(hs[q]->a.d.nx, hs[q]->a.d.ny);
    for (int g = 0; g < hs[q]->a.G; ++g) *smap++ = (uint32_t)q << 16 | (uint32_t)g;
    for (int g = 0; g < gq; ++g) *gmap++ = (uint32_t)q << 16 | (uint32_t)g;
  }
  char* base = static_cast<char*>(table);
  b->t.entries = reinterpret_cast<const FvWideEntry*>(base);
  b->t.sweep = reinterpret_cast<const uint32_t*>(base + sizeof(FvWideEntry) * (size_t)n);
  b->t.gemm = b->t.sweep + sweep;
  const hipError_t e = wide_copy_now(table, image.data(), image.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    delete b;
    return (int)e;
  }
  *out = b;
  return 0;
}

int ldc_fv_wide_batch_destroy(ldc_fv_wide_batch* b) {
  if (!b) return LDC_E_STATE;
  wide_graphs_free(b->gs);
  delete b;
  return 0;
}

int ldc_fv_wide_batch_set_graph(ldc_fv_wide_batch* b, int on) {
  if (!b) return LDC_E_STATE;
  if (on != 0 && on != 1) return LDC_E_ARG;
  b->graph = on;
  return 0;
}

int ldc_fv_wide_batch_enqueue(ldc_fv_wide_batch* b, const int32_t* n_iters, int lin_budget, void* stream) {
  if (!b) return LDC_E_STATE;
  if (!n_iters || lin_budget < 1 || b->n < 1 || b->n > LDC_FV_WIDE_BATCH_MAX) return LDC_E_ARG;
  FvWideQuotas quotas = {};
  int chains = 0;
  for (int q = 0; q < b->n; ++q) {
    if (n_iters[q] < 0 || n_iters[q] > b->rec_cap[q]) return LDC_E_ARG;
    quotas.q[q] = n_iters[q];
    if (n_iters[q] > chains) chains = n_iters[q];
  }
  if (chains < 1) return LDC_E_ARG;
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) return LDC_E_NODEVICE;
  if (dev != b->device) return LDC_E_STATE;
  hipStream_t st = as_stream(stream);
  WIDE_LAUNCH(fv_wide_b_begin, b->n, 64, b->t, quotas);
  return wide_chains(b, chains, wide_lin(lin_budget, b->maxit), wide_np(b), st);
}

int ldc_fv_wide_batch_set_pressure_budget(ldc_fv_wide_batch* b, int budget) {
  if (!b) return LDC_E_STATE;
  if (budget < 1) return LDC_E_ARG;
  b->pbudget = budget;
  return 0;
}

int ldc_fv_wide_batch_launches(const ldc_fv_wide_batch* b, int lin_budget) {
  if (!b || lin_budget < 1) return LDC_E_ARG;
  return 11 + 5 * wide_lin(lin_budget, b->maxit) + (b->mixing ? kWideMixLaunches : 0)
         + (b->pressure ? 2 + kWidePcgLaunches * wide_np(b) : 0);        // (the chain keeps the exact solve's four GEMMs)
}

}  // extern "C"

// ======================================================================================================================
// Post-processing of ONE chip or shared trial (ldc_fv_wide_post_enqueue): the work of fv_post_kernel (ldc_fv_post.hip)
// as a chain of seven launches by the rules above --
//   omega | W1 = Sy^T F | W2 = W1 Sx / Lambda | W1 = Sy W2 | psi = W1 Sx^T | extrema | result
// The cell sweeps (omega, extrema) take the trial's G work-groups, grid-stride; a GEMM launch takes one wave per 16 x 16
// tile of the (ny - 2) x (nx - 2) interior, four tiles per work-group; `result` is ONE work-group.  Every work-group of a
// sweep leaves its not-finite flag and its five (key, cell) candidates in its own slot of the caller's scratch, and
// `result` merges the slots by (larger key, then lower cell): the rule does not depend on the grouping, so the winners
// are those of the one-CU kernel.  The arithmetic is that kernel's too: both call the functions of ldc_fv_post_cells.inc.
// Nothing here reads or writes ctrl, rec, the state or the scratch of the solve, and there is no gate.
namespace {

constexpr int kWPS = 12;                    // doubles of a post slot: 5 keys, 5 cells (as doubles), 2 not-finite flags
enum { WP_CELL = kFvPostBest, WP_BAD_OMEGA = 2 * kFvPostBest, WP_BAD_PSI };     // (the keys: FVP_* at 0 .. 4)
static_assert(LDC_FV_WIDE_POST_SCRATCH_LEN(8, 8) == kWPS * 1, "post scratch layout");
static_assert(LDC_FV_WIDE_POST_SCRATCH_LEN(1024, 1024) == kWPS * kWMaxG, "post scratch layout");
constexpr int kWidePostLaunches = 7;

struct FvWidePost {
  int nx, ny, G;
  int ix_lt, ix_gt, jy_lt, jy_gt;
  double dx, dy, lid;
  const double *u, *v;
  double *psi, *omega, *result, *slots;
};

struct FvWidePostGemm {
  const double *A, *B;
  double* C;
  int sar, sak, sbk, sbc, ldc, M, N, K;
};

// ---- 1. omega with ghost cells, psi = 0 on the ring; slot: this work-group saw a value that is not finite
__global__ __launch_bounds__(kWT) void fv_wide_post_omega(FvWidePost a) {
  const int g = blockIdx.x;
  const int nx = a.nx, ny = a.ny, n = nx * ny;
  bool bad = false;
  for (int c = g * kWT + threadIdx.x; c < n; c += a.G * kWT)
    bad |= fv_post_cell_vorticity(c, nx, ny, a.dx, a.dy, a.lid, a.u, a.v, a.omega, a.psi);
  const int any_bad = __syncthreads_or(bad ? 1 : 0);
  if (threadIdx.x == 0) a.slots[g * kWPS + WP_BAD_OMEGA] = any_bad ? 1.0 : 0.0;
}

// ---- 2. one GEMM of the sine fast diagonalisation, one tile per wave.  SCALE: the Dirichlet epilogue.
template <bool SCALE>
__global__ __launch_bounds__(kWT) void fv_wide_post_gemm(FvWidePostGemm g, const double* lamx, const double* lamy, double dx,
                                                         double dy) {
  const int t = blockIdx.x * kWW + (threadIdx.x >> 6);
  if (t >= ((g.M + 15) >> 4) * ((g.N + 15) >> 4)) return;
  const double cx = 1.0 / (dx * dx), cy = 1.0 / (dy * dy);
  fv_post_gemm_tile<SCALE>(t, g.A, g.sar, g.sak, g.B, g.sbk, g.sbc, g.C, g.ldc, g.M, g.N, g.K, lamx, lamy, cx, cy);
}

// the four GEMMs: W1 = Sy^T F, W2 = W1 Sx / Lambda, W1 = Sy W2, psi = W1 Sx^T (the operands and strides of fv_post_psi)
inline FvWidePostGemm wide_post_gemm_of(const FvDesc& d, const struct ldc_fv_post& p, int which) {
  const int nx = d.nx, mx = d.nx - 2, my = d.ny - 2;
  const int64_t n = (int64_t)d.nx * d.ny;
  double *W1 = d.work + FV_W1 * n, *W2 = d.work + FV_W2 * n;
  const double* F = p.omega + nx + 1;
  if (which == 0) return {p.Sy, F, W1, 1, my, nx, 1, mx, my, mx, my};
  if (which == 1) return {W1, p.Sx, W2, mx, 1, mx, 1, mx, my, mx, mx};
  if (which == 2) return {p.Sy, W2, W1, my, 1, mx, 1, mx, my, mx, my};
  return {W1, p.Sx, p.psi + nx + 1, mx, 1, 1, mx, nx, my, mx, mx};
}

#define WIDE_POST_LDS __shared__ double lkey[kWW][kFvPostBest]; __shared__ int lidx[kWW][kFvPostBest]

// ---- 3. the five extrema over this work-group's cells; slot: the winners and the not-finite flag of psi
__global__ __launch_bounds__(kWT) void fv_wide_post_extrema(FvWidePost a) {
  WIDE_POST_LDS;
  const int g = blockIdx.x;
  const int nx = a.nx, n = a.nx * a.ny;
  bool bad = false;
  FvBest best[kFvPostBest];
  fv_post_best_clear(best);
  for (int c = g * kWT + threadIdx.x; c < n; c += a.G * kWT)
    bad |= fv_post_cell_extrema(c, nx, a.psi, a.omega, a.ix_lt, a.ix_gt, a.jy_lt, a.jy_gt, best);
  fv_post_best_merge<kWW>(best, lkey, lidx);
  const int any_bad = __syncthreads_or(bad ? 1 : 0);
  if (threadIdx.x == 0) {
    double* s = a.slots + g * kWPS;
#pragma unroll
    for (int q = 0; q < kFvPostBest; ++q) { s[q] = best[q].key; s[WP_CELL + q] = (double)best[q].idx; }
    s[WP_BAD_PSI] = any_bad ? 1.0 : 0.0;
  }
}

// ---- 4. result (one work-group): thread t takes slot t, the same merge, then the result block
__global__ __launch_bounds__(kWT) void fv_wide_post_result(FvWidePost a) {
  WIDE_POST_LDS;
  const bool mine = (int)threadIdx.x < a.G;
  const double* s = a.slots + threadIdx.x * kWPS;
  FvBest best[kFvPostBest];
#pragma unroll
  for (int q = 0; q < kFvPostBest; ++q) {
    best[q].key = mine ? s[q] : -HUGE_VAL;
    best[q].idx = mine ? (int)s[WP_CELL + q] : kFvPostNone;
  }
  const bool bad = mine && (s[WP_BAD_OMEGA] != 0.0 || s[WP_BAD_PSI] != 0.0);
  fv_post_best_merge<kWW>(best, lkey, lidx);
  const int any_bad = __syncthreads_or(bad ? 1 : 0);
  if (threadIdx.x == 0) fv_post_result(a.nx * a.ny, a.psi, a.omega, best, any_bad, a.result);
}

}  // namespace

extern "C" {

int ldc_fv_wide_post_enqueue(ldc_fv_wide* h, const struct ldc_fv_post* post, double* scratch, int64_t scratch_len,
                             void* stream) {
  if (!h) return LDC_E_STATE;
  if (!post) return LDC_E_ARG;
  if (h->grid_mode != LDC_FV_GRID_UNIFORM) return LDC_E_ARG;                // (these kernels assume equal spacing)
  const struct ldc_fv_post& p = *post;
  const void* req[] = {p.Sx, p.lamx, p.Sy, p.lamy, p.psi, p.omega, p.result};
  for (const void* x : req) if (!x) return LDC_E_ARG;
  if (p.ix_lt < 0 || p.ix_gt < 0 || p.jy_lt < 0 || p.jy_gt < 0) return LDC_E_ARG;
  const FvDesc& d = h->a.d;
  if (!scratch || scratch_len < LDC_FV_WIDE_POST_SCRATCH_LEN(d.nx, d.ny)) return LDC_E_ARG;
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) return LDC_E_NODEVICE;
  if (dev != h->device) return LDC_E_STATE;
  hipStream_t st = as_stream(stream);
  const int G = h->a.G, gg = (int)LDC_FV_WIDE_GEMM_GROUPS(d.nx - 2, d.ny - 2);
  const FvWidePost a = {d.nx, d.ny, G, p.ix_lt, p.ix_gt, p.jy_lt, p.jy_gt, d.dx, d.dy, d.lid, d.u, d.v,
                        p.psi, p.omega, p.result, scratch};
  WIDE_LAUNCH(fv_wide_post_omega, G, kWT, a);
  WIDE_LAUNCH((fv_wide_post_gemm<false>), gg, kWT, wide_post_gemm_of(d, p, 0), p.lamx, p.lamy, d.dx, d.dy);
  WIDE_LAUNCH((fv_wide_post_gemm<true>), gg, kWT, wide_post_gemm_of(d, p, 1), p.lamx, p.lamy, d.dx, d.dy);
  WIDE_LAUNCH((fv_wide_post_gemm<false>), gg, kWT, wide_post_gemm_of(d, p, 2), p.lamx, p.lamy, d.dx, d.dy);
  WIDE_LAUNCH((fv_wide_post_gemm<false>), gg, kWT, wide_post_gemm_of(d, p, 3), p.lamx, p.lamy, d.dx, d.dy);
  WIDE_LAUNCH(fv_wide_post_extrema, G, kWT, a);
  WIDE_LAUNCH(fv_wide_post_result, 1, kWT, a);
  return 0;
}

int ldc_fv_wide_post_launches(const ldc_fv_wide* h) {
  if (!h) return LDC_E_ARG;
  return kWidePostLaunches;
}

}  // extern "C"

// ======================================================================================================================
// Prolongation of ONE (coarse, fine) pair of chip or shared trials (ldc_fv_wide_prolong_enqueue): the work of
// fv_prolong_kernel (ldc_fv_prolong.hip) as two launches of the FINE trial's G work-groups, grid-stride -- `cells` (u, v,
// p; every thread recomputes the interpolated p at fine cell 0 for itself, so p[0] is exactly 0.0 and nothing is
// broadcast) and, behind the launch boundary, `fluxes` (mdot from the new u and v, wall faces exactly 0.0).  The
// arithmetic is that kernel's: both call the functions of ldc_fv_prolong_cells.inc.  Contraction is off from here to the
// end of the unit, as it is there -- the arithmetic has no multiply-add that the compiler could fuse, and the fine state is
// that kernel's, bit for bit -- so the include stands HERE, behind the pragma and behind the SIMPLE chain, whose
// multiply-adds stay fused.
#pragma STDC FP_CONTRACT OFF

#include "ldc_fv_prolong_cells.inc"

namespace {

struct FvWideProlong {
  FvDesc c, f;
  int G;                                    // work-groups of a sweep over the FINE cells
};

// ---- 1. u, v, p at the fine cell centres
__global__ __launch_bounds__(kWT) void fv_wide_prolong_cells(FvWideProlong a) {
  const FvDesc &c = a.c, &f = a.f;
  const int nx = f.nx, n = f.nx * f.ny;
  const FvAxis ax = {c.nx, c.dx}, ay = {c.ny, c.dy};
  const double p0 = fv_prolong_p0(c, f, ax, ay);
  for (int cell = blockIdx.x * kWT + threadIdx.x; cell < n; cell += a.G * kWT)
    fv_prolong_cell(c, f, ax, ay, nx, p0, cell);
}

// ---- 2. mdot = [ fx | fy ] from the new u and v
__global__ __launch_bounds__(kWT) void fv_wide_prolong_fluxes(FvWideProlong a) {
  const FvDesc& f = a.f;
  const int nx = f.nx, ny = f.ny;
  const int nfx = ny * (nx + 1), nfy = (ny + 1) * nx;
  double *fx = f.mdot, *fy = f.mdot + nfx;
  for (int q = blockIdx.x * kWT + threadIdx.x; q < nfx; q += a.G * kWT) fv_prolong_xface(f, nx, fx, q);
  for (int q = blockIdx.x * kWT + threadIdx.x; q < nfy; q += a.G * kWT) fv_prolong_yface(f, nx, ny, fy, q);
}

}  // namespace

extern "C" {

int ldc_fv_wide_prolong_enqueue(ldc_fv_wide* coarse, ldc_fv_wide* fine, void* stream) {
  if (!coarse || !fine) return LDC_E_STATE;
  if (coarse == fine || !fv_same_domain(coarse->a.d, fine->a.d)) return LDC_E_ARG;
  if (coarse->grid_mode != LDC_FV_GRID_UNIFORM || fine->grid_mode != LDC_FV_GRID_UNIFORM) return LDC_E_ARG;   // (equal spacing)
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) return LDC_E_NODEVICE;
  if (coarse->device != dev || fine->device != dev) return LDC_E_STATE;
  hipStream_t st = as_stream(stream);
  const FvWideProlong a = {coarse->a.d, fine->a.d, fine->a.G};
  WIDE_LAUNCH(fv_wide_prolong_cells, a.G, kWT, a);
  WIDE_LAUNCH(fv_wide_prolong_fluxes, a.G, kWT, a);
  return 0;
}

}  // extern "C"
