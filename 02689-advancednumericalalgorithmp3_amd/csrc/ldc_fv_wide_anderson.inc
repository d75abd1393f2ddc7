// ldc_fv_wide_anderson.inc -- Anderson mixing of a chip or shared trial (include/ldc_fv.h, ldc_fv_wide_set_anderson).
// Included by ldc_fv_wide.hip alone, inside its anonymous namespace, behind the phases of the SIMPLE iteration: the chain
// below is part of that unit's iteration and of its captured graph.
//
// The algorithm is fv_anderson_kernel's (ldc_fv_anderson.hip; tests/fv_anderson_numpy.py restates it): the fixed-point map
// x -> g = SIMPLE(x) on [u | v | p | mdot], hist = [ x | g_prev | f_prev | dG[depth] | dF[depth] ], A = dF^T dF and
// b = dF^T f over the first 3n entries with the columns in slot order, lambda = 1e-12 trace(A) / m, Cholesky by one thread,
// x_next = g - sum_i gamma_i dG_i over all L entries with p[0] written as 0.0, the same fallback and the same four astate
// words.  Its arithmetic is NOT written here: the constants, the view of hist, push and mix for one entry, the row block
// of the Gram sums and the solve are the functions of ldc_fv_anderson_cells.inc, which ldc_fv_wide.hip includes ahead of
// this file and fv_anderson_kernel calls too.  The mapping is the chip mapping's: three launches behind `record`,
//   push  (G work-groups)  f, the new columns dG and dF, g_prev, f_prev for its entries (x = g at once where the
//                          iteration is not mixed); then its partial sums of b and of the lower triangle of A into its
//                          own slot of the mixing scratch
//   mix   (G work-groups)  every work-group adds the slots (thread t takes slot t, wide_block_sum), solves the m x m
//                          system in LDS -- the same numbers by the same instructions in every work-group -- and mixes
//                          its entries; work-group 0 leaves the fell flag in the scratch
//   close (one work-group) writes astate
// The launch boundary is the only barrier; an entry e of hist and of the state is read and written by ONE thread of ONE
// work-group per launch, the same in push and mix (e = g 256 + t + j G 256).
//
// The gate is not wide_gate: after the last iteration of a quota WW_ROW == WW_QUOTA, and that iteration must still be
// mixed.  Every launch returns at once when ctrl[1] == astate[2]: `record` has not counted an iteration since the last
// close, because the trial latched or met a NaN earlier, overflowed (nothing was changed, the iteration comes again),
// has done its quota or has none.  With ctrl[0] or ctrl[2] set by this iteration only astate[2] moves.  push and mix write
// neither ctrl nor astate, so all work-groups of all three launches take the same decisions (WideMixPlan) from the same
// words; close, one work-group, is the only writer of astate, as `record` is of ctrl.  A trial without mixing (depth 0:
// its block is all zero) returns before it reads anything.
//
// Mixing scratch (LDC_FV_WIDE_ANDERSON_SCRATCH_LEN doubles): 8 int64 words (the fell flag), then G slots of
// depth (depth + 3) / 2 doubles: b[depth], then the lower triangle of A by rows.

constexpr int kWMixWords = 8;
enum { MW_FELL };
constexpr int kWMixNeed = kFvAaDepth * (kFvAaDepth + 3) / 2;  // most doubles of a slot
constexpr int kWideMixLaunches = LDC_FV_WIDE_ANDERSON_LAUNCHES;
static_assert(LDC_FV_WIDE_ANDERSON_SCRATCH_LEN(8, 8, 16) == kWMixWords + kWMixNeed * 1, "mixing scratch layout");
static_assert(LDC_FV_WIDE_ANDERSON_SCRATCH_LEN(1024, 1024, 5) == kWMixWords + 20 * kWMaxG, "mixing scratch layout");
static_assert(kWideMixLaunches == 3, "push | mix | close");

__device__ __forceinline__ int wide_mix_slot_len(int depth) { return depth * (depth + 3) / 2; }

// what this iteration's chain does, the same in every work-group of its three launches
struct WideMixPlan {
  bool go;                       // false: nothing at all
  bool count_only;               // the iteration latched or met a NaN: only astate[2] moves
  bool has_f, push, mix;         // x is known from the 2nd iteration on, g_prev from the 3rd
  int slot, m;                   // the ring slot of the new column, the valid columns
  long long it, fallbacks;
};

__device__ __forceinline__ WideMixPlan wide_mix_plan(const FvWideArgs& a, const FvWideMix& x) {
  WideMixPlan p = {};
  if (x.depth == 0) return p;
  const long long it = a.d.ctrl[1], seen = x.astate[2];
  if (it == seen) return p;
  p.go = true;
  p.it = it;
  p.count_only = a.d.ctrl[0] != 0 || a.d.ctrl[2] != 0;
  long long ncol = x.astate[0], pos = x.astate[1];
  p.fallbacks = x.astate[3];
  if (ncol < 0 || ncol > x.depth || pos < 0 || pos >= x.depth) { ncol = 0; pos = 0; }        // (words nobody zeroed)
  p.has_f = seen >= 1;
  p.push = seen >= 2;
  p.slot = (int)pos;
  p.m = p.push ? (ncol < x.depth ? (int)ncol + 1 : x.depth) : (int)ncol;
  p.mix = p.has_f && it >= x.start && p.m > 0;
  return p;
}

// ---- push: every entry of this work-group through fv_anderson_push_entry.  Then A[i][k] = dF_i . dF_k (k <= i) and
//      b[i] = dF_i . f over this work-group's share of the first 3n entries, rows i0 .. i0 + 3 per pass, into its slot.
//      `part`: kWW x kFvAaSums doubles of LDS.
__device__ __forceinline__ void wide_mix_push(const FvWideArgs& a, const FvWideMix& x, int g, double (*part)[kFvAaSums]) {
  const WideMixPlan p = wide_mix_plan(a, x);
  if (!p.go || p.count_only) return;
  const FvDesc& d = a.d;
  const int n = d.nx * d.ny, depth = x.depth, m = p.m;
  const FvAaHist H(x.hist, 3LL * n + LDC_FV_FACES(d.nx, d.ny), depth);
  const int L = (int)H.L, stride = a.G * kWT;
  double *dGs = H.dG + p.slot * H.L, *dFs = H.dF + p.slot * H.L;
  for (int e = g * kWT + threadIdx.x; e < L; e += stride)
    fv_anderson_push_entry(d, H, n, e, p.has_f, p.push, dGs, dFs, !p.mix);
  if (!p.mix) return;
  // (every entry read below was written above by this same thread, or by an earlier launch)
  const int n3 = 3 * n;
  double* slot = x.mscr + kWMixWords + (long long)g * wide_mix_slot_len(depth);
  for (int i0 = 0; i0 < m; i0 += kFvAaRows) {
    double acc[kFvAaRows][kFvAaDepth + 1];
    fv_anderson_acc_clear(acc);
    for (int e = g * kWT + threadIdx.x; e < n3; e += stride) fv_anderson_acc_entry(H, m, i0, e, acc);
    fv_anderson_acc_wave(acc, part);
    __syncthreads();
    if (threadIdx.x < kFvAaSums) {
      double s = part[0][threadIdx.x];
      for (int v = 1; v < kWW; ++v) s += part[v][threadIdx.x];
      const int i = i0 + (int)threadIdx.x / (kFvAaDepth + 1), k = (int)threadIdx.x % (kFvAaDepth + 1);
      if (i < m) {
        if (k == kFvAaDepth) slot[i] = s;
        else if (k <= i) slot[depth + i * (i + 1) / 2 + k] = s;
      }
    }
    __syncthreads();
  }
}

// the LDS of the mix launch
struct WideMixLds {
  double sum[kWW * kWS];
  double tot[kWMixNeed];
  double A[kFvAaDepth][kFvAaDepth + 1];
  double b[kFvAaDepth], gamma[kFvAaDepth];
  int fell;
};

// ---- mix: the totals of the slots, the small solve (fv_anderson_solve), then every entry of this work-group through
//      fv_anderson_mix_entry.
__device__ __forceinline__ void wide_mix_mix(const FvWideArgs& a, const FvWideMix& x, int g, WideMixLds& s) {
  const WideMixPlan p = wide_mix_plan(a, x);
  if (!p.go || p.count_only || !p.mix) return;
  const FvDesc& d = a.d;
  const int n = d.nx * d.ny, depth = x.depth, m = p.m, S = wide_mix_slot_len(depth);
  const double* slots = x.mscr + kWMixWords;
  // b[0 .. m) and the first m rows of the triangle: what push wrote
  const int need = m + m * (m + 1) / 2;
  for (int w0 = 0; w0 < need; w0 += kWS) {
    double t[kWS];
#pragma unroll
    for (int k = 0; k < kWS; ++k) {
      const int w = w0 + k, v = w < m ? w : depth + (w - m);
      t[k] = ((int)threadIdx.x < a.G && w < need) ? slots[(long long)threadIdx.x * S + v] : 0.0;
    }
    wide_block_sum(t, s.sum);
    if (threadIdx.x == 0) {
#pragma unroll
      for (int k = 0; k < kWS; ++k)
        if (w0 + k < need) s.tot[w0 + k] = t[k];
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 0; i < m; ++i) {
      s.b[i] = s.tot[i];
      for (int k = 0; k <= i; ++k) s.A[i][k] = s.tot[m + i * (i + 1) / 2 + k];
    }
    const int fell = fv_anderson_solve(m, s.A, s.b, s.gamma) ? 0 : 1;
    s.fell = fell;
    if (g == 0) reinterpret_cast<long long*>(x.mscr)[MW_FELL] = fell;
  }
  __syncthreads();
  const bool fell = s.fell != 0;
  const FvAaHist H(x.hist, 3LL * n + LDC_FV_FACES(d.nx, d.ny), depth);
  const int L = (int)H.L, stride = a.G * kWT;
  for (int e = g * kWT + threadIdx.x; e < L; e += stride) fv_anderson_mix_entry(d, H, n, e, m, fell, s.gamma);
}

// ---- close (one work-group): astate, once per iteration
__device__ __forceinline__ void wide_mix_close(const FvWideArgs& a, const FvWideMix& x) {
  const WideMixPlan p = wide_mix_plan(a, x);
  __syncthreads();                                         // (every thread has read astate: thread 0 may write it)
  if (!p.go || threadIdx.x != 0) return;
  if (p.count_only) {
    x.astate[2] = p.it;
    return;
  }
  const bool fell = p.mix && reinterpret_cast<const long long*>(x.mscr)[MW_FELL] != 0;
  x.astate[0] = fell ? 0 : p.m;
  x.astate[1] = fell ? 0 : (p.push ? (p.slot + 1) % x.depth : p.slot);
  x.astate[2] = p.it;
  x.astate[3] = p.fallbacks + (fell ? 1 : 0);
}
