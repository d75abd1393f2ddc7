// ldc_wide_kernel.inc -- the chip-wide trial kernel: one trial = T x T work-groups, ONE PER CU ON ALL XCDs, every iteration of
// a chunk in one launch.  Included by ldc_kernels.hip inside its anonymous namespace, after ldc_xcd_kernel.inc (it uses that
// file's node / fold / ring helpers and ldc_cu_kernel.inc's row16_max).
//
// It is the small-N trial kernel's mapping (ldc_xcd_kernel.inc: one contraction family per wave over the FULL contraction
// index, a node's state in the registers of its thread, packed 2-KB tiles + one flag per work-group handed to the 2T-1 mates
// of a tile's row and column, grad p without the pressure transforms, the fold beside the contractions of stage 1) without
// the one-XCD restriction, for 6 <= T <= 16 (N = 81 ... 255, and N = 16 T in the tail layout -- N = 256 -- below):
//   * state crosses work-groups THROUGH THE FABRIC in the guide's valid form 1 (MI355X_MICROARCH.md, "Workgroup dispatch, XCD
//     placement & inter-workgroup visibility"): write-through (sc1) stores of every byte another work-group reads, every
//     storing wave's s_waitcnt vmcnt(0), the work-group barrier, ONE lane's sc1 flag store on a 128-byte line of its own; one
//     wave's sc1 poll of the mates' flags, the work-group barrier, sc1 loads ONLY of handed-off bytes.  Measured before it
//     was built (tools/probes/chip_handoff_probe.hip, profiles/r04_chip_handoff_probe_*.log): a skeleton stage of N = 256
//     shape -- 256 work-groups, 4 x 32 KB of state panels per work-group by sc1 loads, 128 MFMAs per SIMD, 8 KB of tiles
//     stored, drain, flag, poll of 31 mates -- takes 8.5-9.0 us against 9-13 us for a stage LAUNCH, no stale word in 1.6e9;
//   * the four OPERATOR PANELS of a tile (Dx[I], D2x[I], Dy[J], D2y[J]: 16 rows x 16 T doubles each) are RESIDENT IN LDS for
//     the whole launch (T = 16: 128 KB), stored so that an MFMA operand is two linear ds_read_b128; per stage a contraction
//     wave streams ONE state panel through a ring of kWD2 fragments in registers (the next fragments' loads in flight under the
//     8 MFMAs of the current one) -- half the bytes per stage through the CU's one texture path of the launch path's K loop;
//   * T is a run-time value (loop trip counts and LDS offsets): one instantiation per (mode, diagnostics) serves every size;
//   * the ring of grad p in TWO LEVELS (SG): every tile publishes the partial dot products of its new pressure tile with the ring
//     rows (stage 4); in stage 1 the DIAGONAL tile (B, B) adds up the partials of its row mates and of its column mates -- the
//     four ring vectors on block B -- and publishes them; in stage 3 a tile that touches a ring line loads that line's whole
//     vector (4 loads per lane) and takes its sixteen dot products with fragments of the packed GxF / GyF (no tables in LDS):
//     every step reads what one hand-over (mates) or two (anybody) have made visible, nothing is waited for.  (First version:
//     every ring tile added up T partials per index itself -- 16 000 cycles on 60 tiles that all others then waited for.)
//     The smoother needs the ring one hand-over after the pressure: it keeps the direct form behind a wait for all flags;
//   * the stage-4 sums cross LDS as [value][thread] in the result tiles' space (free by then) and eight waves add one value
//     each; the partial sums are stored TRANSPOSED ([value][work-group]) so that the fold reads every value of all 256
//     work-groups with two 16-byte loads per lane: one round trip (the first version's fold -- four rounds of flag polls, 8-byte
//     loads strided by row -- took 28 000 cycles of stage 1 at N = 255, twice the contractions beside it);
//   * the enstrophy / palinstrophy partial sums of stages 1 / 2 are published at the START of the next stage by a wave that is
//     idle there (they are read an iteration later): no barrier, store and drain of their own behind the epilogue.
// Arithmetic: the formulas of every other path (nm_* helpers); one accumulation chain per contraction and k-step parity like
// the small-N kernel, so trajectories agree with the launch path to rounding, not bit for bit.  Parity is pinned against the
// reference's fixtures (tests/test_gpu_wide.py: g4 / g4c trajectories, converged counts, every tiling against the oracle).

constexpr int kWT = 16;                      // tiles per axis at most: T*T work-groups, one per CU
constexpr int kWTmin = 6;                    // below: the small-N kernel (one XCD) is the faster mapping
constexpr int kWD2 = 6;                      // state fragments a velocity contraction wave (two products per fragment) keeps in flight
constexpr int kWD = 4;                       // fragments per operand a single-product wave keeps in flight

struct WArgs {
  int M, LD, NB, T;                // T = ceil(M / 16) (tail: (M-1) / 16): tiles per axis of THIS kernel
  int tail;                        // index M-1 lies outside the tiles (M = 16 T + 1): rank-1 completion + edge jobs
  int Mx, My;                      // nx != ny (never with the tail layout): arrays and tiling of M = max(Mx, My), the shorter axis zero
                                   // padding; wall / lid / interior and the ring lines of grad p come from (Mx, My)
  int with_diag;
  double nu, beta2;
  const double *DxK, *D2xK, *DyK, *D2yK, *GxFK, *GyFK;   // packed operator twins
  const double *ulid, *wx, *wy;
  double *U, *UT, *V, *VT, *P;     // phi^n, row-major: read at entry, written at exit
  double *UK[3], *UTK[3], *VK[3], *VTK[3], *PK[3];      // packed exchange buffers: 0 phi^n, 1 stage buffer A, 2 stage buffer B
  double *PTK[3];                  // packed p^T buffers (borrowed: the launch path's T1TK, T2TK, WTK; its post launch rewrites them)
  double *WK, *WTK;
  const double *IxF, *IyF;         // row-major forms: the ring rows (index 0 and M-1)
  const double *Dx, *D2x, *Dy, *D2y, *GxF, *GyF;   // row-major forms (tail: their rows of index M-1 for the boundary-line nodes)
  const double *DxL, *D2xL, *DyL, *D2yL;            // columns of index M-1 (tail: the rank-1 completion of the tile nodes)
  double* wedge;                   // tail: the vorticity on the two lines of index M-1, [row line (M-1, j) | column line (i, M-1)], 2 x 16 kWT
  double* jobs;                    // tail: the boundary-line jobs' node state between two stages, (2 T + 1) x kWJobDoubles
  double* ring;                    // T*T x 64 doubles: per tile the partial dot products of its pressure tile with the ring rows
  double* rvec;                    // 4 x 16 T doubles: the four ring vectors [a_0 | a_1 | s_0 | s_1], block B by the diagonal tile (B, B)
  double *part4, *partZ0, *partP0;
  long long stride;
  FinalArgs fin;
  unsigned* flags;                 // word 32 x work-group, zeroed before the launch
  unsigned* giveup;                // sticky word of the trial (ldc_solver_status)
  double* stamps;                  // timing experiments (instrumented build only): kWStampsPerWg doubles per work-group, or null
};
constexpr int kWStampPoints = 12;
constexpr int kWStampsPerWg = kStageWaves * 4 * kWStampPoints;

struct WLaunch {
  int B, n_iters;
  const WArgs* trials;             // B argument blocks in device memory, or null: `one`
  WArgs one;
};
static_assert(sizeof(WLaunch) <= 4096, "WLaunch must fit the kernel-argument segment");
typedef const __attribute__((address_space(4))) WArgs WArgsC;

// LDS carve (doubles); run-time T
struct WLds {
  int OPS, RES, AXY, RNG, EYX, RY, TOT, RSUM, TOTAL;
};
__host__ __device__ inline WLds wlds_of(int T) {
  WLds l;
  l.OPS = 0;                       // 4 operator panels x T fragments x 256, fragment = [half][lane][2]
  l.RES = l.OPS + 4 * T * 256;     // 12 result tiles in accumulator order (grad omega takes the slots of grad p); stage 4: the sums, [value][272]
  l.AXY = l.RES + 12 * 256;        // smoother: two ring vectors over the contraction range, 2 x 16 T; tail: partial dot products of the
                                   // boundary-line jobs, [wave 4-7][5][16]
  l.RNG = l.AXY + (32 * T > 384 ? 32 * T : 384);      // ([320..383]: the four quarters of a job's line product of grad omega)
                                   // ring results [kind][2][16] (SG: [kind][0] the tile's own line c = 0, [kind][1] a job's line c = 1), then
                                   // [64..79] a job's line product of grad omega, [80..] single values of the jobs
  l.EYX = l.RNG + 128;             // IyF[0 | M-1][16 J ..] and IxF[0 | M-1][16 I ..]: [4][16]
  l.RY = l.EYX + 64;               // column partials of the four waves [4][2][16]
  l.TOT = l.RY + 128;              // totals of the fold (PS_N + 2, padded)
  l.RSUM = l.TOT + 16;             // 16-lane row sums of a diagnostics sum, kept until the next stage publishes their total; [16]: the
                                   // share of a boundary-line job (tail)
  l.TOTAL = l.RSUM + 32;
  return l;
}
inline size_t wlds_bytes(int T) { return sizeof(double) * (size_t)wlds_of(T).TOTAL; }

#ifdef LDC_TIMING
#define WSTAMP(p) do { if (stp != nullptr && (threadIdx.x & 63) == 0) stp[(p)] = (double)__builtin_amdgcn_s_memtime(); } while (0)
#define WSTAMP_LANDED(p) do { if (stp != nullptr) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); if ((threadIdx.x & 63) == 0) stp[(p)] = (double)__builtin_amdgcn_s_memtime(); } } while (0)
#else
#define WSTAMP_LANDED(p) do { (void)stp; } while (0)
#define WSTAMP(p) do { (void)stp; } while (0)
#endif

// hipcc hoists the address arithmetic of these rarely-run helpers out of the iteration loop and then spills it (the loop's
// register budget belongs to the contraction waves): an opaque copy of the lane number keeps it where it is used
__device__ __forceinline__ int wopaque(int x) { asm volatile("" : "+v"(x)); return x; }
__device__ __forceinline__ int wopaque_s(int x) { asm volatile("" : "+s"(x)); return x; }      // the same for a wave-uniform value

// write-through stores: what another work-group reads
__device__ __forceinline__ void wst1(double* p, double v) {
  __hip_atomic_store((LDC_GLOBAL double*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void wst(double* K, int blk, int off, double v) { wst1(K + ((size_t)blk << 8) + off, v); }

// an operator fragment out of LDS (two linear 16-byte reads per lane)
__device__ __forceinline__ v4d wfrag_lds(const double* f, int lane) {
  const v2d_t lo = *reinterpret_cast<const v2d_t*>(f + 2 * lane);
  const v2d_t hi = *reinterpret_cast<const v2d_t*>(f + 128 + 2 * lane);
  return (v4d){lo[0], lo[1], hi[0], hi[1]};
}

// Wait until the flags of the work-groups this one reads -- row I and column J of the tile grid; `all`: every work-group, four
// flags per lane -- have reached `phase`.  The whole wave polls (L1-bypassing loads).  false (wave-uniform) when the bounded
// wait ran out.
__device__ __forceinline__ bool wwait_flags(unsigned* flags, unsigned phase, int T, int I, int J, bool all, int lane) {
  const int nwg = T * T;
  int wg[4] = {-1, -1, -1, -1};
  if (all) {
#pragma unroll
    for (int k = 0; k < 4; ++k) wg[k] = (lane + 64 * k < nwg) ? lane + 64 * k : -1;
  } else if (lane < 2 * T) {
    wg[0] = lane < T ? I * T + lane : (lane - T) * T + J;
  }
  unsigned long long t0 = 0;
  for (unsigned spins = 0;; ++spins) {
    unsigned v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
      v[k] = ((k == 0 || all) && wg[k] >= 0) ? __hip_atomic_load((LDC_GLOBAL unsigned*)flags + 32 * wg[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : phase;
    const bool behind = (v[0] < phase) || (v[1] < phase) || (v[2] < phase) || (v[3] < phase);
    if (__builtin_amdgcn_ballot_w64(behind) == 0ull) return true;
    if ((spins & 63u) == 63u) {
      const unsigned long long t = __builtin_amdgcn_s_memrealtime();
      if (t0 == 0) t0 = t;
      else if (t - t0 > kSpinLimitTicks) return false;
    }
  }
}
__device__ __forceinline__ void wgive_up(WArgsC& a, TrialState* S) {
  S->abort = 1;
  __hip_atomic_store((LDC_GLOBAL unsigned*)a.giveup, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Hand-over between two stages: every wave's write-through stores are acknowledged (vmcnt(0)), the work-group barrier, thread
// 0 raises this work-group's flag, wave 0 waits for the flags of its mates (any two work-groups share a mate, so a work-group
// two hand-overs ahead of another is impossible: the write-after-read side is covered too), the work-group barrier.
__device__ __forceinline__ bool wbar(WArgsC& a, unsigned& phaseA, int T, int bx, int I, int J, int tid, TrialState* S, bool all,
                                     double* stp = nullptr) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  WSTAMP(7);
  __syncthreads();
  WSTAMP(8);
  ++phaseA;
  if (tid < 64) {
    if (tid == 0) __hip_atomic_store((LDC_GLOBAL unsigned*)a.flags + 32 * bx, phaseA, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!wwait_flags(a.flags, phaseA, T, I, J, all, tid) && tid == 0) wgive_up(a, S);
    WSTAMP(9);
  }
  __syncthreads();
  WSTAMP(10);
  return S->abort == 0;
}

// four consecutive doubles another work-group stored (32-byte aligned offset from a wave-uniform base): two sc1 16-byte loads
__device__ __forceinline__ v4d wld4(const double* base, size_t i) {
  const __amdgpu_buffer_rsrc_t r = raw_rsrc(base);
  const int off = (int)(i * sizeof(double));
  const v2d_t lo = __builtin_bit_cast(v2d_t, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 16));
  const v2d_t hi = __builtin_bit_cast(v2d_t, __builtin_amdgcn_raw_buffer_load_b128(r, off + 16, 0, 16));
  return (v4d){lo[0], lo[1], hi[0], hi[1]};
}
// rows of the transposed partial sums: the work-groups rounded up to whole 32-byte groups
__device__ __forceinline__ int wrows_padded(int nwg) { return (nwg + 3) & ~3; }

// Two contractions over the full index that share their streamed STATE panel (packed, written by other work-groups: sc1
// loads) and differ in the operator (two LDS-resident panels p0, p1: e.g. Dx[I] and D2x[I]).  Four independent MFMA chains
// (even / odd k-steps of the two products).  The state fragments come through a ring of D register sets, each consumed by its
// eight MFMAs and then refilled IN PLACE with fragment g + D (written as `x = f[d]; f[d] = load; mfma(x)` hipcc renamed the
// ring and copied it back at the loop's back edge -- behind a vmcnt(0) per trip).  CONST_A: the operators are the A operands.
template <bool CONST_A>
__device__ __forceinline__ void wchain2(v4d& r0, v4d& r1, const double* p0, const double* p1, const double* pan, int NB,
                                        int prow, int T, int lane) {
  constexpr int D = kWD2;
  v4d f[D];
#pragma unroll
  for (int d = 0; d < D; ++d) {
    f[d] = ldpk_t<true>(pan, NB, prow, d, lane);          // (T >= kWTmin >= D)
    // in THIS order: hipcc otherwise issues the first-needed fragment late, and the wait at the loop header (the merge of the
    // entry order and the loop's own) then drains nearly the whole ring once per trip
    __builtin_amdgcn_sched_barrier(0);
  }
  v4d c0[2], c1[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) { c0[h] = (v4d){0.0, 0.0, 0.0, 0.0}; c1[h] = (v4d){0.0, 0.0, 0.0, 0.0}; }
  auto mm = [&](const v4d& x, int g) {
    const v4d k0 = wfrag_lds(p0 + g * 256, lane), k1 = wfrag_lds(p1 + g * 256, lane);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      if (CONST_A) { c0[s & 1] = MFMA_F64(k0[s], x[s], c0[s & 1]); c1[s & 1] = MFMA_F64(k1[s], x[s], c1[s & 1]); }
      else         { c0[s & 1] = MFMA_F64(x[s], k0[s], c0[s & 1]); c1[s & 1] = MFMA_F64(x[s], k1[s], c1[s & 1]); }
    }
  };
  int g = 0;
  for (; g + 2 * D <= T; g += D) {          // steady state: every prefetch index is < T, no branch around a load
#pragma unroll
    for (int d = 0; d < D; ++d) {
      mm(f[d], g + d);
      f[d] = ldpk_t<true>(pan, NB, prow, g + d + D, lane);
      // the refill goes out HERE, behind its slot's MFMAs: left alone hipcc sinks all refills of a trip behind the trip's last
      // MFMA, and every trip then waits a full load latency at its top
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  // drain: D <= T - g < 2 D fragments left, the first D of them in flight
  const int rest = T - g - D;
#pragma unroll
  for (int d = 0; d < D; ++d) {
    mm(f[d], g + d);
    if (d < rest) f[d] = ldpk_t<true>(pan, NB, prow, g + d + D, lane);
  }
#pragma unroll
  for (int d = 0; d < D; ++d)
    if (d < rest) mm(f[d], g + D + d);
  r0 = xadd(c0[0], c0[1]);
  r1 = xadd(c1[0], c1[1]);
}

// One contraction over the full index, four chains (one per k-step).  The STATE panel is streamed with sc1 loads; the
// operator comes out of LDS (OP_LDS: a resident panel) or is streamed too (plain loads: constant data, cached).
template <bool OP_LDS, bool CONST_A>
__device__ __forceinline__ v4d wchain1(const double* opl, const double* opk, int oprow, const double* pan, int prow, int NB,
                                       int ng, int lane, int g0 = 0) {
  // ng fragments from g0 on (ng >= kWD: the halves of T >= 8 ... the callers see to it)
  constexpr int D = kWD;
  v4d f[D], o[D];
#pragma unroll
  for (int d = 0; d < D; ++d) {
    f[d] = ldpk_t<true>(pan, NB, prow, g0 + (d < ng ? d : ng - 1), lane);
    if (!OP_LDS) o[d] = ldpk(opk, NB, oprow, g0 + (d < ng ? d : ng - 1), lane);
    __builtin_amdgcn_sched_barrier(0);                    // (in this order, see wchain2)
  }
  v4d c[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) c[s] = (v4d){0.0, 0.0, 0.0, 0.0};
  auto mm = [&](const v4d& x, const v4d& k) {
#pragma unroll
    for (int s = 0; s < 4; ++s) c[s] = CONST_A ? MFMA_F64(k[s], x[s], c[s]) : MFMA_F64(x[s], k[s], c[s]);
  };
  int g = 0;
  for (; g + 2 * D <= ng; g += D) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      mm(f[d], OP_LDS ? wfrag_lds(opl + (g0 + g + d) * 256, lane) : o[d]);
      f[d] = ldpk_t<true>(pan, NB, prow, g0 + g + d + D, lane);
      if (!OP_LDS) o[d] = ldpk(opk, NB, oprow, g0 + g + d + D, lane);
      __builtin_amdgcn_sched_barrier(0);                  // (the refill stays behind its slot's MFMAs, see wchain2)
    }
  }
  const int rest = ng - g - D;                            // (negative when ng < D: the clamped prologue loads are then not all used)
#pragma unroll
  for (int d = 0; d < D; ++d) {
    if (g + d < ng) mm(f[d], OP_LDS ? wfrag_lds(opl + (g0 + g + d) * 256, lane) : o[d]);
    if (d < rest) {
      f[d] = ldpk_t<true>(pan, NB, prow, g0 + g + d + D, lane);
      if (!OP_LDS) o[d] = ldpk(opk, NB, oprow, g0 + g + d + D, lane);
    }
  }
#pragma unroll
  for (int d = 0; d < D; ++d)
    if (d < rest) mm(f[d], OP_LDS ? wfrag_lds(opl + (g0 + g + D + d) * 256, lane) : o[d]);
  return xadd(xadd(c[0], c[1]), xadd(c[2], c[3]));
}

__device__ __forceinline__ void wput(double* lds, const WLds& Ld, int slot, const v4d& acc, int lane) {
#pragma unroll
  for (int r = 0; r < 4; ++r) lds[Ld.RES + (slot * 4 + r) * 64 + lane] = acc[r];
}

// total / maximum over the 64 lanes of a wave, the same value in every lane (fixed order: 16-lane rows by DPP, the four rows
// by lane swaps)
__device__ __forceinline__ double wave_total(double x) { return quad_sum(row16_sum(x)); }
__device__ __forceinline__ double wave_top(double x) { return quad_max(row16_max(x)); }

// The fold of the stage-4 partial sums and of the lagged enstrophy / palinstrophy slabs by ONE wave of every work-group (the same
// values in the same order everywhere: dt and the latch need no broadcast): wfold_dt / wfold_record in front of wstage.  The sums
// lie transposed, [value][work-group]: lane l takes the work-groups 4 l .. 4 l + 3 of EVERY value with two 16-byte loads per
// value, all in flight together -- one round trip --, adds its four, and a wave total per value finishes it.

// ---- the boundary ring of grad p (see ldc_xcd_kernel.inc for the mathematics) ---------------------------------------
// every tile publishes the partial dot products of the pressure tile it has just produced with the ring rows of IyF / IxF:
// 64 doubles at ring + 64 bx = [a_0 | a_1 | s_0 | s_1].  All 64 lanes of waves 0-3 call.
__device__ __forceinline__ void wring_partials(WArgsC& a, const WLds& Ld, const XNode& n, double* lds, double pn, int bx,
                                               int lane, int wv) {
  double* dst = a.ring + (size_t)wopaque_s(bx) * 64;
  const double eyc[2] = {lds[Ld.EYX + n.tj], lds[Ld.EYX + 16 + n.tj]};
  const double exc[2] = {lds[Ld.EYX + 32 + n.ti], lds[Ld.EYX + 48 + n.ti]};
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const double r = row16_sum(pn * eyc[c]);                         // over the tile's 16 columns
    if ((lane & 15) == 0) wst1(dst + c * 16 + n.ti, r);
    const double q = quad_sum(exc[c] * pn);                          // over this wave's 4 rows; the 4 waves meet in LDS
    if (lane < 16) lds[Ld.RY + (wv * 2 + c) * 16 + lane] = q;
  }
}
__device__ __forceinline__ void wring_partials_finish(WArgsC& a, const WLds& Ld, const double* lds, int bx, int tid) {     // after a barrier
  if (tid < 32) {
    const double* r = lds + Ld.RY + tid;                             // tid = c * 16 + column
    wst1(a.ring + (size_t)wopaque_s(bx) * 64 + 32 + tid, ((r[0] + r[32]) + r[64]) + r[96]);
  }
}
// SG, level 1 (stage 1, one wave of the diagonal tile (B, B)): the four ring vectors on block B.  Lane (v = lane >> 4, r): a_v
// over the row mates (B, L) for v < 2, s_(v-2) over the column mates (L, B) -- the tiles whose partials the hand-over just
// passed has made visible.  All T loads of a lane in flight together.
__device__ __forceinline__ void wring_reduce(WArgsC& a, int T, int B, int lane_) {
  const int lane = wopaque(lane_);
  const int v = lane >> 4, r = lane & 15;
  double t[kWT];
#pragma unroll
  for (int L = 0; L < kWT; ++L) {
    const int Lc = L < T ? L : T - 1;
    t[L] = xld(a.ring, (size_t)(v < 2 ? B * T + Lc : Lc * T + B) * 64 + v * 16 + r);
  }
  double s = 0.0;
#pragma unroll
  for (int L = 0; L < kWT; ++L) s += (L < T) ? t[L] : 0.0;
  wst1(a.rvec + (size_t)v * 16 * T + 16 * B + r, s);
}
// Sixteen dot products of a PUBLISHED vector (16 T doubles at vec + off, stored write-through by other work-groups, visible
// since the hand-over(s) passed) with the sixteen rows of block row `oprow` of a packed operator: lane (r, q) takes row r and the
// k-quarter q of every fragment (its four vector elements by one sc1 load, the same address in the sixteen lanes of a quarter),
// the quarters meet by lane swaps.  Result (lanes < 16) to out[r].  Used for
//   SG, level 2 of the ring (stage 3): ring line c of kind 0 (ring column j = 0 | M-1: d/dx p at the tile's 16 rows, GxF[I]) or
//     kind 1 (ring row i = 0 | M-1: d/dy p at its 16 columns, GyF[J]) from the ring vector 2 kind + c;
//   the tail layout's line products of grad omega (omega on a line of index M-1 against Dy[J] / Dx[I]).
__device__ __forceinline__ void wvec_line(const double* vec, size_t off, const double* opK, int oprow, int NB, int T, int lane_,
                                          double* out, const double* opl = nullptr) {
  // opl: the operator's panel is one of the tile's LDS-resident ones (Dx[I], Dy[J]) -- no global operand loads at all
  const int lane = wopaque(lane_);
  double s = 0.0;
#pragma unroll
  for (int g0 = 0; g0 < kWT; g0 += 8) {                 // two batches of eight fragments: two round trips per line
    if (g0 < T) {
      v4d G[8], A[8];
#pragma unroll
      for (int g = 0; g < 8; ++g) {
        const int gc = g0 + g < T ? g0 + g : T - 1;
        if (opl == nullptr) G[g] = ldpk(opK, NB, oprow, gc, lane);
        A[g] = wld4(vec, off + 16 * gc + 4 * (lane >> 4));
      }
#pragma unroll
      for (int g = 0; g < 8; ++g) {
        if (g0 + g < T) {
          const v4d Gg = (opl == nullptr) ? G[g] : wfrag_lds(opl + (g0 + g) * 256, lane);
          s = nm_madd(Gg[0], A[g][0], s); s = nm_madd(Gg[1], A[g][1], s);
          s = nm_madd(Gg[2], A[g][2], s); s = nm_madd(Gg[3], A[g][3], s);
        }
      }
    }
  }
  s = quad_sum(s);
  if (lane < 16) out[lane] = s;
}
// The same for at most eight fragments g0 .. g0 + ng - 1 in ONE batch, in two steps so that a caller can put other loads between
// the request and the use (loads return in order: whatever is requested behind these finds them landed).  A lane fetches ONE
// element of each fragment's sixteen -- element 4 q + (lane & 3) for its k-quarter q = lane >> 4 -- and gets the four it needs
// from the lanes of its quad (quad broadcasts): 16 registers for a batch instead of 64.  Four independent chains, one per
// element: beside a contraction wave (the jobs' line products of stage 4) every instruction that waits for the one before it
// costs a whole MFMA of the FP64 pipe both share, 64 cycles.
struct WVecHalf { double a[8]; };
__device__ __forceinline__ void wvec_issue(WVecHalf& h, const double* vec, size_t off, int g0, int ng, int lane_) {
  const int lane = wopaque(lane_);
#pragma unroll
  for (int g = 0; g < 8; ++g) h.a[g] = xld(vec, off + 16 * (g0 + (g < ng ? g : ng - 1)) + 4 * (lane >> 4) + (lane & 3));
}
// opl: the operator's panel in LDS (resident), or null: its packed twin opK, block row oprow
__device__ __forceinline__ void wvec_finish(const WVecHalf& h, const double* opl, const double* opK, int oprow, int NB, int g0, int ng,
                                            int lane_, double* out) {
  const int lane = wopaque(lane_);
  v4d G[8];
  if (opl == nullptr) {
#pragma unroll
    for (int g = 0; g < 8; ++g) G[g] = ldpk(opK, NB, oprow, g0 + (g < ng ? g : ng - 1), lane);
  }
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll
  for (int g = 0; g < 8; ++g) {
    if (g < ng) {
      const v4d Gg = (opl == nullptr) ? G[g] : wfrag_lds(opl + (g0 + g) * 256, lane);
      s0 = nm_madd(Gg[0], dpp_move<0x00>(h.a[g]), s0); s1 = nm_madd(Gg[1], dpp_move<0x55>(h.a[g]), s1);
      s2 = nm_madd(Gg[2], dpp_move<0xAA>(h.a[g]), s2); s3 = nm_madd(Gg[3], dpp_move<0xFF>(h.a[g]), s3);
    }
  }
  const double s = quad_sum((s0 + s1) + (s2 + s3));
  if (lane < 16) out[lane] = s;
}
__device__ __forceinline__ void wring_line(WArgsC& a, int T, int blk, int lane, int kind, int c, double* out) {
  wvec_line(a.rvec, (size_t)(2 * kind + c) * 16 * T, kind == 0 ? a.GxFK : a.GyFK, blk, a.NB, T, lane, out);
}
// dot product of a row-major row (constant data) with a published vector, n <= 256 a multiple of 4: the same value in every lane
__device__ __forceinline__ double wvv(const double* row, const double* vec, size_t off, int n, int lane_) {
  const int lane = wopaque(lane_);
  double s = 0.0;
  if (4 * lane < n) {
    const v4d r = *(const LDC_GLOBAL v4d*)(row + 4 * lane);
    const v4d x = wld4(vec, off + 4 * lane);
    s = nm_madd(r[0], x[0], s); s = nm_madd(r[1], x[1], s); s = nm_madd(r[2], x[2], s); s = nm_madd(r[3], x[3], s);
  }
  return wave_total(s);
}

// ---- tail layout (M = 16 T + 1): index M-1 lies outside the tiles -------------------------------------------------
// The state on the two lines of index M-1 is a boundary condition -- constant for the whole launch (the caller runs the first
// iteration after an upload on the launch path, which leaves phi^n with its boundary values there).  So
//   * a TILE node completes its contractions for k = M-1 with six constants formed at entry (WTailNode), and the two line
//     products of grad omega with the vorticity the line nodes publish;
//   * the 2 M - 1 nodes of the lines only feed |R_u|, |R_v| (stage 4; quirk Q4: boundary nodes count), the enstrophy and the
//     palinstrophy: per block of 16 they are a JOB of one tile -- row nodes (M-1, 16 J + r) of tile (J, J), column nodes
//     (16 I + r, M-1) of tile (I, I+1 mod T), the corner of tile (1, 3) -- whose wave 6 owns one node per lane (r = lane & 15).
//     Of a node's eight derivatives the four ACROSS its line are constants (the line's own values differentiated along it);
//     the four ALONG the streamed direction are dot products of the operators' rows of index M-1 with columns (rows) of the
//     stage input: waves 4-7 of the job's tile each stream a quarter of the fragments of the panels involved (the same packed
//     panels the contraction waves read; <= 4 fragments per panel and wave, one round trip) and leave partial dot products in
//     LDS beside the contractions; wave 6 finishes the nodes beside the epilogue of the tile nodes.  grad p^n on the lines:
//     the component along the streamed direction the same way (stage 1), the other from the ring vectors (line c = 1, stage 3).
struct WTailNode {
  double cux, cvx, cuy, cvy, clu, clv;   // what k = M-1 adds to du/dx, dv/dx, du/dy, dv/dy, lap u, lap v at this tile node
  double dxl, dyl;                       // Dx[i][M-1], Dy[j][M-1]: the line products of grad omega
};
struct WJob {
  int kind;            // -1 none; 0 row node (M-1, 16 J + r); 1 column node (16 I + r, M-1); 2 the corner (lane 0)
  int blk;             // J (kind 0) or I (kind 1)
  double ue, ve;       // boundary values of u, v at the node (its stage input and its phi^n)
  double am1, am2;     // the operators' own entries at index M-1 along the streamed direction: Dx, D2x (kind 0) / Dy, D2y (kind 1) [M-1][M-1]
  double cd[4];        // the derivatives across the line (constants): kind 0: uy, uyy, vy, vyy; kind 1 and 2: ux, uxx, vx, vxx
  double ce[4];        // kind 2: uy, uyy, vy, vyy (all eight are constants at the corner)
  double pgs, pgr;     // grad p^n at the node: the streamed component (kind 0: px, kind 1: py) and the ring-line component
  double omega;        // vorticity at the node (this iteration)
  double wq;           // quadrature weight
  double opl;          // kind 0: Dy[j][M-1], kind 1: Dx[i][M-1] (the corner's share of the node's line product of grad omega)
  double wc;           // vorticity at the corner (a constant)
};
// A job's node state lives in global scratch between two stages ([field][16 lanes]; field 15: the job's uniform values): in
// registers it was live across the contraction loops of every wave (one register allocation for all roles) and hipcc spilled
// 150-240 registers per lane.  Wave 6 of the job's tile loads it beside the contractions and stores back what a stage changed.
constexpr int kWJobDoubles = 16 * 16;
constexpr double kWJobTag = 7.25e22 + 1977.0;      // field 15, entry 3 of a job's block: its constants are in place
enum { WJ_UE = 0, WJ_VE, WJ_CD0, WJ_CD1, WJ_CD2, WJ_CD3, WJ_PGS, WJ_PGR, WJ_OMEGA, WJ_WQ, WJ_OPL, WJ_CE0, WJ_CE1, WJ_CE2, WJ_CE3, WJ_UNI };
__device__ __forceinline__ int wjob_id(int kind, int blk, int T) { return kind == 0 ? blk : kind == 1 ? T + blk : 2 * T; }
__device__ __forceinline__ void wjob_load(WArgsC& a, WJob& jb, int T, int lane) {
  const double* base = a.jobs + (size_t)wjob_id(jb.kind, jb.blk, T) * kWJobDoubles;
  const int r = wopaque(lane) & 15;
  jb.ue = xld(base, WJ_UE * 16 + r); jb.ve = xld(base, WJ_VE * 16 + r);
  jb.cd[0] = xld(base, WJ_CD0 * 16 + r); jb.cd[1] = xld(base, WJ_CD1 * 16 + r);
  jb.cd[2] = xld(base, WJ_CD2 * 16 + r); jb.cd[3] = xld(base, WJ_CD3 * 16 + r);
  jb.ce[0] = xld(base, WJ_CE0 * 16 + r); jb.ce[1] = xld(base, WJ_CE1 * 16 + r);
  jb.ce[2] = xld(base, WJ_CE2 * 16 + r); jb.ce[3] = xld(base, WJ_CE3 * 16 + r);
  jb.pgs = xld(base, WJ_PGS * 16 + r); jb.pgr = xld(base, WJ_PGR * 16 + r);
  jb.omega = xld(base, WJ_OMEGA * 16 + r); jb.wq = xld(base, WJ_WQ * 16 + r); jb.opl = xld(base, WJ_OPL * 16 + r);
  jb.am1 = xld(base, WJ_UNI * 16 + 0); jb.am2 = xld(base, WJ_UNI * 16 + 1); jb.wc = xld(base, WJ_UNI * 16 + 2);
}
__device__ __forceinline__ void wjob_store(WArgsC& a, const WJob& jb, int T, int lane_, bool all) {
  const int lane = wopaque(lane_);
  double* base = a.jobs + (size_t)wjob_id(jb.kind, jb.blk, T) * kWJobDoubles;
  if (lane < 16) {
    wst1(base + WJ_PGS * 16 + lane, jb.pgs); wst1(base + WJ_PGR * 16 + lane, jb.pgr); wst1(base + WJ_OMEGA * 16 + lane, jb.omega);
    if (all) {
      wst1(base + WJ_UE * 16 + lane, jb.ue); wst1(base + WJ_VE * 16 + lane, jb.ve);
      wst1(base + WJ_CD0 * 16 + lane, jb.cd[0]); wst1(base + WJ_CD1 * 16 + lane, jb.cd[1]);
      wst1(base + WJ_CD2 * 16 + lane, jb.cd[2]); wst1(base + WJ_CD3 * 16 + lane, jb.cd[3]);
      wst1(base + WJ_CE0 * 16 + lane, jb.ce[0]); wst1(base + WJ_CE1 * 16 + lane, jb.ce[1]);
      wst1(base + WJ_CE2 * 16 + lane, jb.ce[2]); wst1(base + WJ_CE3 * 16 + lane, jb.ce[3]);
      wst1(base + WJ_WQ * 16 + lane, jb.wq); wst1(base + WJ_OPL * 16 + lane, jb.opl);
      if (lane == 0) { wst1(base + WJ_UNI * 16 + 0, jb.am1); wst1(base + WJ_UNI * 16 + 1, jb.am2); wst1(base + WJ_UNI * 16 + 2, jb.wc); }
    }
  }
}
enum { WR_JOBLINE = 64, WR_EXTRA = 96, WR_CGX = 97, WR_CGY = 98, WR_CPX = 99, WR_CPY = 100, WR_JOBRING2 = 104 };   // slots behind the ring results (WLds::RNG)

// This wave's share (fragments g = w4, w4 + 4, ...: at most four) of the dot products of a job's streamed panels with the
// operators' rows of index M-1.  MODE 1 (stage 1): [0] v (row job) | u (column job) . Dx | Dy row (the vorticity; DIAG only),
// [1] p . GxF | GyF row (grad p^n).  MODE 3 (stage 3): [0] omega . Dx | Dy row.  MODE 4 (stage 4): [0] u . D, [1] u . D2,
// [2] v . D, [3] v . D2.  Partial sums (lanes < 16) to AXY[(w4 * 5 + d) * 16 + r] (MODE 3: d = 4).
struct WEdgeLoads { double ra[4], rb[4]; v4d f0[4], f1[4]; };
// Request (no arithmetic: next to a contraction wave, which keeps the FP64 pipe of its SIMD busy with one 64-cycle MFMA after
// the other, EVERY vector instruction of another wave of that SIMD waits for a gap -- measured ~40 cycles per instruction, with
// or without raised priority: the 150 instructions of a share took 6 000 cycles) ...
template <int MODE, bool DIAGV>
__device__ __forceinline__ void wedge_issue(WEdgeLoads& w, WArgsC& a, int kind, int blk, const XStageIo io, int T, int w4, int lane_) {
  const int lane = wopaque(lane_);
  const int NB = a.NB;
  const size_t rowm = (size_t)(a.M - 1) * a.LD;
  const double *pan0, *pan1, *rA, *rB;
  if (MODE == 1) {
    pan0 = kind == 0 ? a.VTK[io.in] : a.UK[io.in]; pan1 = kind == 0 ? a.PTK[io.pin] : a.PK[io.pin];
    rA = (kind == 0 ? a.Dx : a.Dy) + rowm; rB = (kind == 0 ? a.GxF : a.GyF) + rowm;
  } else if (MODE == 3) {
    pan0 = kind == 0 ? a.WTK : a.WK; pan1 = pan0;
    rA = (kind == 0 ? a.Dx : a.Dy) + rowm; rB = rA;
  } else {
    pan0 = kind == 0 ? a.UTK[io.in] : a.UK[io.in]; pan1 = kind == 0 ? a.VTK[io.in] : a.VK[io.in];
    rA = (kind == 0 ? a.Dx : a.Dy) + rowm; rB = (kind == 0 ? a.D2x : a.D2y) + rowm;
  }
  constexpr bool use0 = !(MODE == 1 && !DIAGV), use1 = MODE != 3;
  // ONE round trip for the whole share (under the contraction waves' streams a round trip is 2 000-3 000 cycles, and a loop that
  // fetched the operators' pieces fragment by fragment behind the panels made four more of them).  The pieces of the operators'
  // rows first -- ONE element per lane, element 4 q + (lane & 3) of the fragment's 16 for k-quarter q = lane >> 4, so that the four
  // elements a lane needs sit in the four lanes of its quad and arrive by quad broadcasts; as whole four-vectors per lane they
  // took 64 registers beside the panels' 64 and pushed the kernels of the tail layout over 256 -- then the panel fragments.
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int g = w4 + 4 * m, gc = g < T ? g : T - 1;
    const int ko = 16 * gc + 4 * (lane >> 4) + (lane & 3);
    w.ra[m] = *(const LDC_GLOBAL double*)(rA + ko);
    w.rb[m] = use1 ? *(const LDC_GLOBAL double*)(rB + ko) : w.ra[m];
    // a fragment beyond the range (T not a multiple of four) counts with a zero operator piece: under a branch `g < T` hipcc
    // sank the first fragment's panel loads into the conditional block, behind the wait for the others -- a second round trip
    if (g >= T) { w.ra[m] = 0.0; w.rb[m] = 0.0; }
  }
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int g = w4 + 4 * m, gc = g < T ? g : T - 1;
    w.f0[m] = use0 ? ldpk_t<true>(pan0, NB, blk, gc, lane) : (v4d){0.0, 0.0, 0.0, 0.0};
    w.f1[m] = use1 ? ldpk_t<true>(pan1, NB, blk, gc, lane) : w.f0[m];
  }
}
// ... and the dot products, where no contraction is under way.
template <int MODE, bool DIAGV>
__device__ __forceinline__ void wedge_dots(const WEdgeLoads& w, const WLds& Ld, double* lds, int w4, int lane_) {
  const int lane = wopaque(lane_);
  constexpr bool use0 = !(MODE == 1 && !DIAGV), use1 = MODE != 3;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const v4d va = {dpp_move<0x00>(w.ra[m]), dpp_move<0x55>(w.ra[m]), dpp_move<0xAA>(w.ra[m]), dpp_move<0xFF>(w.ra[m])};
    v4d vb = va;
    if (use1) vb = (v4d){dpp_move<0x00>(w.rb[m]), dpp_move<0x55>(w.rb[m]), dpp_move<0xAA>(w.rb[m]), dpp_move<0xFF>(w.rb[m])};
    if (MODE == 1) { if (use0) fma4(acc[0], w.f0[m], va); fma4(acc[1], w.f1[m], vb); }
    if (MODE == 3) fma4(acc[0], w.f0[m], va);
    if (MODE == 4) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {          // (four independent chains, element by element)
        acc[0] = fma(w.f0[m][e], va[e], acc[0]); acc[1] = fma(w.f0[m][e], vb[e], acc[1]);
        acc[2] = fma(w.f1[m][e], va[e], acc[2]); acc[3] = fma(w.f1[m][e], vb[e], acc[3]);
      }
    }
  }
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    if ((MODE == 1 && d < 2) || (MODE == 3 && d < 1) || MODE == 4) {
      const double x = quad_sum(acc[d]);
      // (five slots per wave: the product of stage 3 goes to slot 4 -- it is read in stage 4, behind that stage's own four)
      if (lane < 16) lds[Ld.AXY + (w4 * 5 + (MODE == 3 ? 4 : d)) * 16 + lane] = x;
    }
  }
}
template <int MODE, bool DIAGV>
__device__ __forceinline__ void wedge_stream(WArgsC& a, const WLds& Ld, double* lds, int kind, int blk, const XStageIo io,
                                             int T, int w4, int lane) {
  WEdgeLoads w;
  wedge_issue<MODE, DIAGV>(w, a, kind, blk, io, T, w4, lane);
  wedge_dots<MODE, DIAGV>(w, Ld, lds, w4, lane);
}

// Wave 6 of a job's tile, beside the epilogue of the tile nodes: the four waves' partial dot products -> the node's
// derivatives -> what the stage records at the node.  ev[]: the node's share of the stage-4 sums (MODE 4).
template <int MODE, bool DIAGV>
__device__ __forceinline__ void wedge_finish(WArgsC& a, const WLds& Ld, double* lds, WJob& jb, int lane, double (&ev)[PS_N]) {
  const int r = lane & 15;
  auto P = [&](int d) { const double* e = lds + Ld.AXY + d * 16 + r; return ((e[0] + e[80]) + e[160]) + e[240]; };
  const double* rng = lds + Ld.RNG;
  double* rsum = lds + Ld.RSUM;
  const bool own = jb.kind == 2 ? (lane == 0) : (lane < 16);       // the lanes whose node counts (the other rows hold copies)
  if (MODE == 1) {
    if (jb.kind < 2) {
      if (DIAGV) {
        const double S = P(0) + jb.am1 * (jb.kind == 0 ? jb.ve : jb.ue);      // dv/dx at a row node, du/dy at a column node
        jb.omega = jb.kind == 0 ? (S - jb.cd[0]) : (jb.cd[2] - S);          // sg.py:510-522
        if (lane < 16) wst1(a.wedge + (size_t)jb.kind * 16 * kWT + 16 * jb.blk + wopaque(r), jb.omega);
      }
      jb.pgs = P(1);
    } else {
      jb.omega = jb.wc;
    }
    if (DIAGV) {
      const double z = row16_sum(own ? jb.wq * jb.omega * jb.omega : 0.0);
      if (lane == 0) rsum[16] = z;
    }
  }
  if (MODE == 3) {
    // grad p^n, the ring-line component: line c = 1 of the ring vectors (wave 7 of this tile, stage 3); at the two nodes where
    // the lines of index M-1 meet the ring lines of index 0 the streamed component is the extrapolated one too
    if (jb.kind == 0) { jb.pgr = rng[48 + r] + rng[WR_JOBRING2 + r]; if (jb.blk == 0 && r == 0) jb.pgs = rng[WR_EXTRA]; }
    if (jb.kind == 1) { jb.pgr = rng[16 + r] + rng[WR_JOBRING2 + r]; if (jb.blk == 0 && r == 0) jb.pgs = rng[WR_EXTRA]; }
    if (jb.kind == 2) { jb.pgs = rng[WR_CPX]; jb.pgr = rng[WR_CPY]; }
  }
  if (MODE == 5) {          // the nodes' share of the palinstrophy (another wave than MODE 3 / 4: it needs the node state only)
    if (DIAGV) {
      double gx, gy;                                                         // sg.py:546-547
      const double* lq = lds + Ld.AXY + 320 + r;                                    // the four quarters of the line product
      const double line = ((lq[0] + lq[16]) + lq[32]) + lq[48];
      if (jb.kind == 0) { gx = P(4) + jb.am1 * jb.omega; gy = line + jb.wc * jb.opl; }
      else if (jb.kind == 1) { gy = P(4) + jb.am1 * jb.omega; gx = line + jb.opl * jb.wc; }
      else { gx = rng[WR_CGX]; gy = rng[WR_CGY]; }
      const double pp = row16_sum(own ? jb.wq * nm_sq2(gx, gy) : 0.0);
      if (lane == 0) rsum[16] = pp;
    }
  }
  if (MODE == 4) {
    double ux, uxx, vx, vxx, uy, uyy, vy, vyy, px, py;
    if (jb.kind == 0) {
      ux = P(0) + jb.am1 * jb.ue; uxx = P(1) + jb.am2 * jb.ue; vx = P(2) + jb.am1 * jb.ve; vxx = P(3) + jb.am2 * jb.ve;
      uy = jb.cd[0]; uyy = jb.cd[1]; vy = jb.cd[2]; vyy = jb.cd[3]; px = jb.pgs; py = jb.pgr;
    } else if (jb.kind == 1) {
      uy = P(0) + jb.am1 * jb.ue; uyy = P(1) + jb.am2 * jb.ue; vy = P(2) + jb.am1 * jb.ve; vyy = P(3) + jb.am2 * jb.ve;
      ux = jb.cd[0]; uxx = jb.cd[1]; vx = jb.cd[2]; vxx = jb.cd[3]; py = jb.pgs; px = jb.pgr;
    } else {
      ux = jb.cd[0]; uxx = jb.cd[1]; vx = jb.cd[2]; vxx = jb.cd[3]; uy = jb.ce[0]; uyy = jb.ce[1]; vy = jb.ce[2]; vyy = jb.ce[3];
      px = jb.pgs; py = jb.pgr;
    }
    const double Ru = nm_momentum(jb.ue, jb.ve, ux, uy, px, a.nu, uxx + uyy);
    const double Rv = nm_momentum(jb.ue, jb.ve, vx, vy, py, a.nu, vxx + vyy);
    // (the node's value is a boundary condition and never changes: no du, dv; no continuity residual on the boundary)
    ev[PS_U02] = own ? jb.ue * jb.ue : 0.0; ev[PS_V02] = own ? jb.ve * jb.ve : 0.0;
    ev[PS_RU2] = own ? Ru * Ru : 0.0; ev[PS_RV2] = own ? Rv * Rv : 0.0;
    ev[PS_E] = own ? jb.wq * nm_sq2(jb.ue, jb.ve) : 0.0;
    ev[PS_UMAX] = own ? fabs(jb.ue) : 0.0; ev[PS_VMAX] = own ? fabs(jb.ve) : 0.0;
  }
}

// Entry: the job of this tile, if any (wave 6; every lane, the dot products are wave-cooperative).  Reads the row-major phi^n
// (its lines of index M-1 hold the boundary values) and the row-major operators.
__device__ __forceinline__ void wjob_init(WArgsC& a, WJob& jb, int T, int I, int J, int lane) {
  const int M = a.M, LD = a.LD, m1 = M - 1, r = lane & 15;
  const size_t rowm = (size_t)m1 * LD;
  jb.kind = (I == J) ? 0 : (J == (I + 1) % T) ? 1 : (I == 1 && J == 3) ? 2 : -1;
  jb.blk = jb.kind == 0 ? J : I;
  jb.ue = jb.ve = jb.am1 = jb.am2 = jb.pgs = jb.pgr = jb.omega = jb.wq = jb.opl = jb.wc = 0.0;
#pragma unroll
  for (int d = 0; d < 4; ++d) { jb.cd[d] = 0.0; jb.ce[d] = 0.0; }
  if (jb.kind < 0) return;
  // vorticity at the corner: dv/dx - du/dy with both lines' boundary values (sg.py:510-522)
  jb.wc = dot_rows(a.Dx + rowm, a.VT + rowm, M, lane) - dot_rows(a.U + rowm, a.Dy + rowm, M, lane);
  if (jb.kind == 0) {
    const int j = 16 * J + r;
    jb.ue = a.U[rowm + j]; jb.ve = a.V[rowm + j];
    jb.am1 = a.Dx[rowm + m1]; jb.am2 = a.D2x[rowm + m1];
    jb.wq = a.wx[m1] * a.wy[j]; jb.opl = a.DyL[j];
    for (int q = 0; q < 16; ++q) {                       // the east-wall row of u, v differentiated along y at node (M-1, 16 J + q)
      const size_t rj = (size_t)(16 * J + q) * LD;
      const double x0 = dot_rows(a.U + rowm, a.Dy + rj, M, lane), x1 = dot_rows(a.U + rowm, a.D2y + rj, M, lane);
      const double x2 = dot_rows(a.V + rowm, a.Dy + rj, M, lane), x3 = dot_rows(a.V + rowm, a.D2y + rj, M, lane);
      if (r == q) { jb.cd[0] = x0; jb.cd[1] = x1; jb.cd[2] = x2; jb.cd[3] = x3; }
    }
  } else if (jb.kind == 1) {
    const int i = 16 * I + r;
    jb.ue = a.UT[rowm + i]; jb.ve = a.VT[rowm + i];
    jb.am1 = a.Dy[rowm + m1]; jb.am2 = a.D2y[rowm + m1];
    jb.wq = a.wx[i] * a.wy[m1]; jb.opl = a.DxL[i];
    for (int q = 0; q < 16; ++q) {                       // the lid column of u, v differentiated along x at node (16 I + q, M-1)
      const size_t ri = (size_t)(16 * I + q) * LD;
      const double x0 = dot_rows(a.Dx + ri, a.UT + rowm, M, lane), x1 = dot_rows(a.D2x + ri, a.UT + rowm, M, lane);
      const double x2 = dot_rows(a.Dx + ri, a.VT + rowm, M, lane), x3 = dot_rows(a.D2x + ri, a.VT + rowm, M, lane);
      if (r == q) { jb.cd[0] = x0; jb.cd[1] = x1; jb.cd[2] = x2; jb.cd[3] = x3; }
    }
  } else {
    jb.ue = a.U[rowm + m1]; jb.ve = a.V[rowm + m1];
    jb.wq = a.wx[m1] * a.wy[m1];
    jb.cd[0] = dot_rows(a.Dx + rowm, a.UT + rowm, M, lane); jb.cd[1] = dot_rows(a.D2x + rowm, a.UT + rowm, M, lane);
    jb.cd[2] = dot_rows(a.Dx + rowm, a.VT + rowm, M, lane); jb.cd[3] = dot_rows(a.D2x + rowm, a.VT + rowm, M, lane);
    jb.ce[0] = dot_rows(a.U + rowm, a.Dy + rowm, M, lane); jb.ce[1] = dot_rows(a.U + rowm, a.D2y + rowm, M, lane);
    jb.ce[2] = dot_rows(a.V + rowm, a.Dy + rowm, M, lane); jb.ce[3] = dot_rows(a.V + rowm, a.D2y + rowm, M, lane);
    jb.am1 = a.Dx[rowm + m1]; jb.am2 = a.Dy[rowm + m1];        // (kind 2: the two first-derivative entries, for grad omega at the corner)
  }
}

// Smoother: the direct form.  One of the two ring waves (half = 0 / 1) takes the contraction blocks g = half, half + 2, ...: it
// adds up the tiles' partial dot products for the 16 indices of each of its blocks (one lane per index, all T loads of a pass
// in flight), keeps the vector in LDS and takes its share of the sixteen dot products.  Result: RNG[kind][half][16] (the
// epilogue adds the two halves).
__device__ __forceinline__ void wring(WArgsC& a, const WLds& Ld, double* lds, int T, int I, int J, int lane, int half,
                                      int kind, int c) {
  const int NB = a.NB;
  double* vec = lds + Ld.AXY + kind * 16 * T;
  const int nblk = (T - half + 1) / 2;                 // blocks g = half + 2 m, m < nblk
  v4d G[(kWT + 1) / 2];
#pragma unroll
  for (int m = 0; m < (kWT + 1) / 2; ++m) {
    const int g = half + 2 * (m < nblk ? m : 0);
    G[m] = ldpk(kind == 0 ? a.GxFK : a.GyFK, NB, kind == 0 ? I : J, g, lane);
  }
  for (int m0 = 0; m0 < nblk; m0 += 4) {               // four blocks per pass: lane = (block of the pass, index in the block)
    const int m = m0 + (lane >> 4), r = lane & 15;
    const int B = half + 2 * (m < nblk ? m : 0);
    double t[kWT];
#pragma unroll
    for (int L = 0; L < kWT; ++L) {
      const int Lc = L < T ? L : T - 1;
      // a_c[16 B + r]: over the tiles (B, L) of row block B;  s_c[16 B + r]: over the tiles (L, B) of column block B
      const size_t o = (size_t)(kind == 0 ? B * T + Lc : Lc * T + B) * 64 + (kind == 0 ? 0 : 32) + c * 16 + r;
      t[L] = xld(a.ring, o);
    }
    double s = 0.0;
#pragma unroll
    for (int L = 0; L < kWT; ++L) s += (L < T) ? t[L] : 0.0;
    if (m < nblk) vec[16 * B + r] = s;
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // this wave's own LDS writes, read back by other lanes below
  double s = 0.0;
#pragma unroll
  for (int m = 0; m < (kWT + 1) / 2; ++m) {
    if (m < nblk) {
      const int g = half + 2 * m;
      const v4d av = *reinterpret_cast<const v4d*>(vec + 16 * g + 4 * (lane >> 4));
      s = nm_madd(G[m][0], av[0], s); s = nm_madd(G[m][1], av[1], s);
      s = nm_madd(G[m][2], av[2], s); s = nm_madd(G[m][3], av[3], s);
    }
  }
  s = quad_sum(s);
  if (lane < 16) lds[Ld.RNG + (kind * 2 + half) * 16 + lane] = s;
}

// The fold, first half (stage 1, wave 7, beside the contractions): wait for every work-group's stage-4 flag, request ALL rows of
// the transposed partial sums (the two maxima first) and reduce the maxima -- what the NEXT dt, the only thing the epilogue of this
// stage needs, is formed from (wfold_step).  The sums stay in registers (fx) for the record (wfold_record).
struct WFoldState { bool crit, flush; double umax, vmax; };
__device__ __forceinline__ WFoldState wfold_dt(WArgsC& a, TrialState* S, int T, int I, int J, int lane, unsigned phaseA,
                                               v4d (&fx)[PS_N + 2], double* stp) {
  WFoldState f = {false, false, 0.0, 0.0};
  if (!wwait_flags(a.flags, phaseA, T, I, J, true, lane)) {
    if (lane == 0) wgive_up(a, S);
    return f;
  }
  WSTAMP(1);
  // (raised priority for the reductions: this wave shares its SIMD's FP64 pipe with the MFMA chains of a contraction wave, which
  //  always has the next MFMA ready -- every vector instruction here waits for a gap between two of them)
  __builtin_amdgcn_s_setprio(3);
  FinalArgs fin;
  __builtin_memcpy(&fin, &a.fin, sizeof(FinalArgs));
  f.crit = fin.do_critical && !S->done && (S->step > S->iter);
  f.flush = fin.with_diag && (S->flushed < S->iter) && (S->pdone >= S->iter);
  const int nwg = T * T, nwp = wrows_padded(nwg), r0 = 4 * lane;
  const bool in = r0 < nwp;
#pragma unroll
  for (int q = 0; q < PS_N + 2; ++q) fx[q] = (v4d){0.0, 0.0, 0.0, 0.0};
  if (f.crit && in) {
    fx[PS_UMAX] = wld4(a.part4, (size_t)PS_UMAX * nwp + r0);
    fx[PS_VMAX] = wld4(a.part4, (size_t)PS_VMAX * nwp + r0);
#pragma unroll
    for (int q = 0; q < PS_NSUM; ++q) fx[q] = wld4(a.part4, (size_t)q * nwp + r0);
  }
  if (f.flush && in) {
    const size_t off = (size_t)((S->iter - 1) & 1) * a.stride + r0;
    fx[PS_N] = wld4(a.partZ0, off);
    fx[PS_N + 1] = wld4(a.partP0, off);
  }
  if (f.crit) {
    auto top = [&](const v4d& x) {
      const double e0 = (r0 < nwg) ? x[0] : 0.0, e1 = (r0 + 1 < nwg) ? x[1] : 0.0;
      const double e2 = (r0 + 2 < nwg) ? x[2] : 0.0, e3 = (r0 + 3 < nwg) ? x[3] : 0.0;
      return wave_top(fmax(fmax(e0, e1), fmax(e2, e3)));
    };
    f.umax = top(fx[PS_UMAX]); f.vmax = top(fx[PS_VMAX]);
  }
  WSTAMP(9);
  return f;              // (still at raised priority: wfold_step lowers it)
}
// ... and the NEXT dt from the maxima.
__device__ __forceinline__ void wfold_step(WArgsC& a, TrialState* S, const WFoldState& f, int lane) {
  if (f.crit) {
    FinalArgs fin;
    __builtin_memcpy(&fin, &a.fin, sizeof(FinalArgs));
    // the same operations on the same operands as fin_decide_wave (which repeats them for the record): bit-identical dt
    const double xr = lane == 0 ? dt_lambda_x(f.umax, fin) : lane == 1 ? dt_lambda_y(f.vmax, fin) : 0.0;
    const double lxy = lane_value(xr, 0) + lane_value(xr, 1);
    const double dt_new = fin.cfl / lxy;
    if (lane == 0) { S->dtp = S->dt; S->dt = dt_new; }
  }
  __builtin_amdgcn_s_setprio(0);
}
// The fold, second half (after the work-group barrier, beside the epilogue and the hand-over): the remaining totals, the
// record, the latch, the counters.
__device__ __forceinline__ void wfold_record(WArgsC& a, const WLds& Ld, double* lds, TrialState* S, int T, int lane, bool writer,
                                             const WFoldState f, const v4d (&fx)[PS_N + 2], double* stp) {
  if (!f.crit && !f.flush) return;
  FinalArgs fin;
  __builtin_memcpy(&fin, &a.fin, sizeof(FinalArgs));
  const int nwg = T * T, r0 = 4 * lane;
  double* tot = lds + Ld.TOT;
#pragma unroll
  for (int q = 0; q < PS_N + 2; ++q) {
    // (entries beyond the last work-group: never written by this kernel, possibly stale from another path)
    const double e0 = (r0 < nwg) ? fx[q][0] : 0.0, e1 = (r0 + 1 < nwg) ? fx[q][1] : 0.0;
    const double e2 = (r0 + 2 < nwg) ? fx[q][2] : 0.0, e3 = (r0 + 3 < nwg) ? fx[q][3] : 0.0;
    const bool is_max = (q == PS_UMAX || q == PS_VMAX);
    const double s = is_max ? fmax(fmax(e0, e1), fmax(e2, e3)) : ((e0 + e1) + (e2 + e3));
    const double t = is_max ? wave_top(s) : wave_total(s);
    if (lane == 0) tot[q] = t;
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // this wave's own LDS writes, read back by other lanes below
  WSTAMP(11);
  const double dt_cur = f.crit ? S->dtp : S->dt;         // the step the closed iteration used (wfold_dt has installed the next)
  const FinOut o = fin_decide_wave(fin, tot, lane, f.crit, f.flush, S->iter, S->flushed, dt_cur, writer);
  if (lane == 0) {
    S->flushed = o.flushed;
    if (f.crit) {
      S->umax = o.umax; S->vmax = o.vmax; S->dt = o.dt; S->iter = o.iter;
      if (o.latch) S->done = o.latch;
    }
  }
}

// One RK stage K = 0 ... 3 of an iteration.  What the eight waves do, by phase ([A] beside the contractions, [E] beside the
// epilogue of the tile nodes, [W] the WINDOW: between a wave's own store drain and the work-group barrier that ends the stage --
// while waves 0-3 drain their tile stores and wave 0 raises the flag and polls the mates', waves 4-7 are free):
//   waves 0-3  [A] the eight velocity contractions  [E] the tile nodes (one per thread), write-through tile stores
//   stage 1    [A] w4-w6 d/dx p, d/dy p (three shares); w7 ring level 1 (diagonal tiles), then the fold's dt   [W] w7 the fold's record;
//              [W] tail jobs: the streamed dot products of stage 1 (w4-w6)
//   stage 2    [E] tail jobs: w6 finishes the line nodes' vorticity (published with this stage's hand-over)
//   stage 3    [A] w7 publishes the enstrophy sum; w4-w7 grad omega: Dx[I] . omega^T[J] and omega[I] . Dy[J], two halves of the
//              contraction range each, for this stage's epilogue   [W] w4 / w5 this tile's ring lines; tail jobs: w6 / w7 the job's
//              ring line in halves, all four the streamed product of grad omega
//   stage 4    [A] tail jobs: the REQUESTS of the streamed dot products of stage 4 (w4-w7), of the line product of grad omega (w4 / w5)
//              and of the node state (w6)   [E] tail jobs: their arithmetic (w4-w7), behind the second barrier w6: the line nodes'
//              palinstrophy and residuals; then the stage-4 sums over all eight waves, the palinstrophy sum published with them
// The smoother (SP): d/dx p, d/dy p in every stage [A]; the ring directly in stage 4 [A]; no windows.
// Returns false when the launch must end (a wait was given up) -- block-uniform.
template <bool SP, bool DIAGV, bool TAIL, int K>
__device__ __forceinline__ bool wstage(WArgsC& a, const WLds& Ld, XNode& n, const WTailNode& tn, const int jkind,
                                       const int jblk, double* lds, TrialState* S, unsigned& phaseA, const int T_, const int bx_,
                                       const int I_, const int J_, const bool fold, const bool stamp) {
  static_assert(!(TAIL && SP), "the tail layout is built for SG");
  constexpr bool GPV = SP || K == 0;                 // this stage differentiates a pressure
  constexpr bool LAST = K == 3;
  constexpr int DIAGE = !DIAGV ? 0 : K == 0 ? 1 : K == 2 ? 2 : 0;      // epilogue: 1 vorticity + enstrophy, 2 grad omega -> palinstrophy
  constexpr bool AGRADW = DIAGV && K == 2;           // grad omega, beside the contractions of stage 3 (see there)
  constexpr bool RRED = !SP && K == 0;               // ring level 1
  constexpr bool WLINES = !SP && K == 2;             // window: ring lines (and the jobs' lines)
  constexpr bool RINGE = !SP && K == 3;              // the epilogue takes grad p on the ring from the lines
  constexpr bool RING3 = SP && K == 3;               // smoother: the direct ring
  constexpr bool RPROD = SP ? K == 2 : K == 3;       // the epilogue publishes the ring partials of its pressure
  constexpr bool PUBZ = DIAGV && K == 2;             // the enstrophy sum of stage 1 is published at the start of this stage
  constexpr double alphas[4] = {0.25, 1.0 / 3.0, 0.5, 1.0};      // sg.py:430
  // 0: phi^n -> A   1: A -> B   2: B -> A   3: A -> phi^n (in place);  the pressure likewise (smoother mode)
  constexpr int bin[4] = {0, 1, 2, 1}, bout[4] = {1, 2, 1, 0};
  const XStageIo io = {bin[K], bout[K], bin[K], bout[K], alphas[K], K};
  // Opaque copies of what every address in this stage is formed from: the four stages are inlined into the iteration loop, and
  // hipcc otherwise hoists each stage's address arithmetic (dozens of 64-bit pointers and LDS offsets per lane) out of the
  // loop, where it stays live across the contraction loops of all four -- 300 scalar and up to 240 vector registers spilled.
  const int T = wopaque_s(T_), bx = wopaque_s(bx_), I = wopaque_s(I_), J = wopaque_s(J_);
  WJob jb;                           // this tile's job (tail): its node state is a guest in wave 6's registers for one stage
  jb.kind = TAIL ? jkind : -1; jb.blk = jblk;
  jb.ue = jb.ve = jb.am1 = jb.am2 = jb.pgs = jb.pgr = jb.omega = jb.wq = jb.opl = jb.wc = 0.0;
#pragma unroll
  for (int d = 0; d < 4; ++d) { jb.cd[d] = 0.0; jb.ce[d] = 0.0; }
  const int tid = wopaque((int)threadIdx.x), lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);          // wave-uniform: the role dispatch is scalar branches
#ifdef LDC_TIMING
  double* const stp = stamp ? a.stamps + (size_t)bx * kWStampsPerWg + (wv * 4 + K) * kWStampPoints : nullptr;
#else
  double* const stp = nullptr; (void)stamp;
#endif
  WSTAMP(0);
  const int NB = a.NB, nwg = T * T;
  constexpr bool has_p = SP || LAST;
  const double* ops = lds + Ld.OPS;
  const int iLast = (a.Mx - 1) / 16, jLast = (a.My - 1) / 16;      // the tile row / column that holds index Mx-1 / My-1 (tail: none, T itself)
  double* rsum = lds + Ld.RSUM;
  double* rng = lds + Ld.RNG;
  const bool job = TAIL && jb.kind >= 0;                // block-uniform
  v4d fx[PS_N + 2];                                     // the fold's sums (wave 7, stage 1)
  WFoldState fs = {false, false, 0.0, 0.0};
  WEdgeLoads jw;                                        // a job's requests of stage 4 (waves 4-7), used behind the barrier
  WVecHalf jvh;
  // ---------------------------------------------------------------- [A] contractions, one family per wave
  double wre = 0.0, wce = 0.0;       // tail, stage 3: the vorticity on the two lines of index M-1 at this node's column / row
  if (wv < 4) {
    if (TAIL && DIAGE == 2) { wre = xld(a.wedge, (size_t)n.j); wce = xld(a.wedge, (size_t)16 * kWT + n.i); }    // (published in stage 2)
    // waves 0 / 1: u^T[J] / v^T[J] against Dx[I], D2x[I] (operators = A operands); waves 2 / 3: u[I] / v[I] against Dy[J], D2y[J]
    const bool xrole = wv < 2;
    const double* pan = wv == 0 ? a.UTK[io.in] : wv == 1 ? a.VTK[io.in] : wv == 2 ? a.UK[io.in] : a.VK[io.in];
    const double* p0 = ops + (xrole ? 0 : 2) * T * 256;
    v4d c0, c1;
    if (xrole) wchain2<true>(c0, c1, p0, p0 + T * 256, pan, NB, J, T, lane);
    else wchain2<false>(c0, c1, p0, p0 + T * 256, pan, NB, I, T, lane);
    WSTAMP(1);
    // wave 0: du/dx, d2u/dx2   1: dv/dx, d2v/dx2   2: du/dy, d2u/dy2   3: dv/dy, d2v/dy2
    wput(lds, Ld, wv == 0 ? XR_UX : wv == 1 ? XR_VX : wv == 2 ? XR_UY : XR_VY, c0, lane);
    wput(lds, Ld, wv == 0 ? XR_UXX : wv == 1 ? XR_VXX : wv == 2 ? XR_UYY : XR_VYY, c1, lane);
  } else {
    if (PUBZ && wv == 7 && lane == 0) {
      // the enstrophy sum of stage 1: its sixteen row sums in a fixed order (+ the share of a boundary-line job), one
      // write-through store, drained with this stage's stores (read by the fold of the next iteration)
      const double* r = rsum;
      const double x = (((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))) +
                       (((r[8] + r[9]) + (r[10] + r[11])) + ((r[12] + r[13]) + (r[14] + r[15])));
      const int step0 = S->step;
      wst1(a.partZ0 + (size_t)((step0 > 0 ? step0 - 1 : 0) & 1) * a.stride + wopaque_s(bx), TAIL ? x + r[16] : x);
    }
    if (GPV) {
      // d/dx p = GxF[I] . p^T[J] off the ring columns, d/dy p = p[I] . GyF[J] off the ring rows (the interior rows of IxF / IyF are
      // unit rows).  128 MFMAs beside the 128 per SIMD of the velocity contractions: three shares -- wave 4 the first c1 blocks of
      // d/dx p, wave 5 the first c1 of d/dy p, wave 6 the rest of both (c1 = 2 T / 3) -- so that no SIMD carries more than ~172
      // (two waves with a whole product each: 192 on two SIMDs, the others waiting).  The smoother's stage 4 keeps two waves: its
      // waves 6 / 7 assemble the ring there.
      constexpr bool THREE = !(SP && K == 3);
      const int c1 = THREE ? (2 * T + 1) / 3 : T;
      if (wv == 4) wput(lds, Ld, XR_PX, wchain1<false, true>(nullptr, a.GxFK, I, a.PTK[io.pin], J, NB, c1, lane), lane);
      else if (wv == 5) wput(lds, Ld, XR_PY, wchain1<false, false>(nullptr, a.GyFK, J, a.PK[io.pin], I, NB, c1, lane), lane);
      else if (THREE && wv == 6) {
        wput(lds, Ld, XR_WX, wchain1<false, true>(nullptr, a.GxFK, I, a.PTK[io.pin], J, NB, T - c1, lane, c1), lane);
        wput(lds, Ld, XR_WY, wchain1<false, false>(nullptr, a.GyFK, J, a.PK[io.pin], I, NB, T - c1, lane, c1), lane);
      }
    }
    if (AGRADW) {
      // grad omega of phi^(n+1): Dx[I] . omega^T[J] (waves 4, 6) and omega[I] . Dy[J] (waves 5, 7), each over half of the
      // contraction range; omega was published by stage 1 (the operator panels are the resident ones): 32 MFMAs per SIMD beside the
      // 128 of the velocity contractions.  NOT in the window of stage 2, where they cost nothing: there the results were not
      // reproducible -- two identical runs disagreed in the palinstrophy partial sums of some tiles by anything from 1e-10 to
      // factors, in 5 % of the iterations (tools/debug/p_tiles.py; the state, the enstrophy and every other sum bit-identical).  No
      // cause found: the vorticity panels are the mates' stores of stage 1, handed over like the velocities; delaying the window
      // until every wave's stores were drained made the differences rarer, not rare; with the contractions here, 1 600 slabs equal.
      const int h0 = (T + 1) / 2, g0 = wv < 6 ? 0 : h0, ng = wv < 6 ? h0 : T - h0;
      if ((wv & 1) == 0) wput(lds, Ld, wv == 4 ? XR_PX : XR_WX, wchain1<true, true>(ops, nullptr, 0, a.WTK, J, NB, ng, lane, g0), lane);
      else wput(lds, Ld, wv == 5 ? XR_PY : XR_WY, wchain1<true, false>(ops + 2 * T * 256, nullptr, 0, a.WK, I, NB, ng, lane, g0), lane);
    }
    if (RRED && wv == 7 && I == J) wring_reduce(a, T, I, lane);      // (in front of the fold: its wait for every flag takes thousands of cycles anyway)
    if (K == 0 && wv == 7 && fold) {
      fs = wfold_dt(a, S, T, I, J, lane, phaseA, fx, stp);
      // (the step right here, beside the contractions, although its ~100 vector instructions wait ~40 cycles each for a gap between
      //  two MFMAs: behind the barrier, with the epilogue waiting where it needs the step, they are 1 400 cycles of the critical
      //  path -- N=255 32.1 us per iteration instead of 31.7; here they end about when the contractions do)
      wfold_step(a, S, fs, lane);            // (after a give-up: crit is false, nothing is installed)
    }
    if (TAIL && LAST && job) {
      // a job's share of stage 4: REQUESTS only beside the contractions -- the two halves of its line product of grad omega (the
      // vorticity of the WHOLE lines of index M-1, published by the jobs with hand-over 2 and visible to every work-group since
      // hand-over 3; waves 4 / 5), the node state (wave 6), the corner's two whole-line products (wave 7 of the corner tile) and the
      // four shares of the streamed dot products.  The arithmetic follows behind the barrier, beside the epilogue of the tile nodes.
      const size_t rowm = (size_t)(a.M - 1) * a.LD;
      // (the line product in four quarters of the contraction range, one per wave: on two waves their arithmetic behind the barrier
      //  took 3 500 cycles against the tile nodes' epilogue of 1 900)
      const int q0 = (wv - 4) * T / 4, q1 = (wv - 3) * T / 4;
      if (DIAGV && jb.kind < 2) wvec_issue(jvh, a.wedge, jb.kind == 0 ? 0 : (size_t)16 * kWT, q0, q1 - q0, lane);
      if (wv >= 6) wjob_load(a, jb, T, lane);                 // (waves 6 and 7: each finishes half of the nodes' sums behind the second barrier)
      if (jb.kind < 2) wedge_issue<4, DIAGV>(jw, a, jb.kind, jb.blk, io, T, wv - 4, lane);
      if (DIAGV && jb.kind == 2 && wv == 7) {
        const double* jbase = a.jobs + (size_t)wjob_id(2, 0, T) * kWJobDoubles;
        const int l4 = 4 * wopaque(lane), n4 = 16 * T;
        jw.ra[0] = xld(jbase, WJ_UNI * 16 + 0); jw.ra[1] = xld(jbase, WJ_UNI * 16 + 1); jw.ra[2] = xld(jbase, WJ_UNI * 16 + 2);
        const bool in = l4 < n4;
        const int lc = in ? l4 : 0;
        jw.f0[0] = *(const LDC_GLOBAL v4d*)(a.Dx + rowm + lc); jw.f0[1] = wld4(a.wedge, (size_t)16 * kWT + lc);
        jw.f0[2] = *(const LDC_GLOBAL v4d*)(a.Dy + rowm + lc); jw.f0[3] = wld4(a.wedge, (size_t)lc);
        if (!in) { jw.f0[0] = (v4d){0.0, 0.0, 0.0, 0.0}; jw.f0[2] = jw.f0[0]; }
      }
      WSTAMP(1);
    }
    if (TAIL && K == 1 && wv == 6 && job) wjob_load(a, jb, T, lane);      // (stage 2: the line nodes' vorticity is finished beside the epilogue)
    if (RING3 && wv >= 6) {
      if (!wwait_flags(a.flags, phaseA, T, I, J, true, lane)) {
        if (lane == 0) wgive_up(a, S);
      } else {
        if (J == 0 || J == jLast) wring(a, Ld, lds, T, I, J, lane, wv - 6, 0, J == 0 ? 0 : 1);
        if (I == 0 || I == iLast) wring(a, Ld, lds, T, I, J, lane, wv - 6, 1, I == 0 ? 0 : 1);
      }
    }
  }
  WSTAMP(2);
  __syncthreads();
  WSTAMP(3);
  if (S->abort != 0) return false;
  // ---------------------------------------------------------------- [E] the tile nodes: one per thread of waves 0-3; what the
  // other work-groups read goes straight to the packed buffers (write-through).  Beside them: the fold's record, a job's nodes.
  double v[PS_N], ev[PS_N];
#pragma unroll
  for (int q = 0; q < PS_N; ++q) ev[q] = 0.0;
  if (TAIL && K == 1 && wv == 6 && job) { wedge_finish<1, DIAGV>(a, Ld, lds, jb, lane, ev); wjob_store(a, jb, T, lane, false); }
  if (TAIL && LAST && job && wv >= 4) {
    // the arithmetic of the job's stage-4 requests, waves 4-7 beside the epilogue of the tile nodes (no MFMA in the way)
    if (jb.kind < 2) wedge_dots<4, DIAGV>(jw, Ld, lds, wv - 4, lane);
    if (DIAGV && jb.kind < 2) {
      const int q0 = (wv - 4) * T / 4, q1 = (wv - 3) * T / 4;
      wvec_finish(jvh, jb.kind == 0 ? ops + 2 * T * 256 : ops, nullptr, 0, NB, q0, q1 - q0, lane, lds + Ld.AXY + 320 + 16 * (wv - 4));
    }
    if (DIAGV && jb.kind == 2 && wv == 7) {
      // the corner: grad omega from the two whole lines of index M-1 (sg.py:546-547)
      double sx = 0.0, sy = 0.0;
#pragma unroll
      for (int e = 0; e < 4; ++e) { sx = nm_madd(jw.f0[0][e], jw.f0[1][e], sx); sy = nm_madd(jw.f0[2][e], jw.f0[3][e], sy); }
      const double gxc = wave_total(sx) + jw.ra[0] * jw.ra[2], gyc = wave_total(sy) + jw.ra[1] * jw.ra[2];
      if (lane == 0) { rng[WR_CGX] = gxc; rng[WR_CGY] = gyc; }
    }
  }
  if (tid < 256) {
    auto C = [&](int slot) { return lds[Ld.RES + (slot * 4 + wv) * 64 + lane]; };
    double ux = C(XR_UX), vx = C(XR_VX), uy = C(XR_UY), vy = C(XR_VY);
    double lu = C(XR_UXX) + C(XR_UYY), lv = C(XR_VXX) + C(XR_VYY);
    if (TAIL) { ux += tn.cux; vx += tn.cvx; uy += tn.cuy; vy += tn.cvy; lu += tn.clu; lv += tn.clv; }   // k = M-1
    const int blkIJ = I * NB + J, blkJI = J * NB + I;
    double dsum = 0.0;
    if (GPV) {
      constexpr bool THREE = !(SP && K == 3);
      n.px = n.valid ? (THREE ? C(XR_PX) + C(XR_WX) : C(XR_PX)) : 0.0;
      n.py = n.valid ? (THREE ? C(XR_PY) + C(XR_WY) : C(XR_PY)) : 0.0;
    }
    // on the ring: the 1-D extrapolation from the lines of the stage-3 window (before this stage the value there is unused)
    if (RINGE) {
      if (n.rc >= 0) n.px = rng[n.ti];
      if (n.rr >= 0) n.py = rng[32 + n.tj];
    }
    if (RING3) {
      if (n.rc >= 0) n.px = rng[n.ti] + rng[16 + n.ti];
      if (n.rr >= 0) n.py = rng[32 + n.tj] + rng[48 + n.tj];
    }
    if (DIAGE == 1) {
      const double w = n.valid ? (vx - uy) : 0.0;            // sg.py:510-522 on this stage's input = phi^(n+1) of the last iteration
      wst(a.WK, blkIJ, n.oU, w);
      wst(a.WTK, blkJI, n.oT, w);
      dsum = n.valid ? n.wq * w * w : 0.0;
    }
    if (DIAGE == 2) {
      // grad omega: the two halves of each contraction, parked by the window of stage 2 (sg.py:546-547)
      double gx = C(XR_PX) + C(XR_WX), gy = C(XR_PY) + C(XR_WY);
      if (TAIL) { gx = nm_madd(tn.dxl, wre, gx); gy = nm_madd(wce, tn.dyl, gy); }      // k = M-1: omega on the two lines
      dsum = n.valid ? n.wq * nm_sq2(gx, gy) : 0.0;
    }
    const double Ru = nm_momentum(n.uc, n.vc, ux, uy, n.px, a.nu, lu);
    const double Rv = nm_momentum(n.uc, n.vc, vx, vy, n.py, a.nu, lv);
    const double Rp = nm_continuity(a.beta2, ux, vy);
    const double adt = io.alpha * S->dt;
    double un = nm_madd(adt, Ru, n.u0), vn = nm_madd(adt, Rv, n.v0);
    // walls first, lid last (sg.py:348-385): the lid row wins the two top corners
    if (!n.valid) { un = 0.0; vn = 0.0; }
    else if (n.lid) { un = n.lidv; vn = 0.0; }
    else if (n.wall) { un = 0.0; vn = 0.0; }
    wst(a.UK[io.out], blkIJ, n.oU, un);
    wst(a.UTK[io.out], blkJI, n.oT, un);
    wst(a.VK[io.out], blkIJ, n.oU, vn);
    wst(a.VTK[io.out], blkJI, n.oT, vn);
    double pn = 0.0;
    if (has_p) {
      pn = n.interior ? nm_madd(adt, Rp, n.p0) : 0.0;
      wst(a.PK[io.pout], blkIJ, n.oU, pn);
      wst(a.PTK[io.pout], blkJI, n.oT, pn);
      if (RPROD) wring_partials(a, Ld, n, lds, pn, bx, lane, wv);
    }
    if (LAST) {
      const double du = un - n.u0, dv = vn - n.v0;
      v[PS_DU2] = n.valid ? du * du : 0.0;
      v[PS_DV2] = n.valid ? dv * dv : 0.0;
      v[PS_U02] = n.valid ? n.u0 * n.u0 : 0.0;
      v[PS_V02] = n.valid ? n.v0 * n.v0 : 0.0;
      v[PS_RU2] = n.valid ? Ru * Ru : 0.0;
      v[PS_RV2] = n.valid ? Rv * Rv : 0.0;
      v[PS_RP2] = n.interior ? Rp * Rp : 0.0;
      v[PS_E] = n.valid ? n.wq * nm_sq2(un, vn) : 0.0;
      v[PS_UMAX] = fabs(un);
      v[PS_VMAX] = fabs(vn);
      n.u0 = un; n.v0 = vn; n.p0 = pn;
    }
    if (DIAGE != 0) {
      // sixteen row sums into LDS: published later (enstrophy: start of stage 3; palinstrophy: with the stage-4 sums)
      const double r = row16_sum(dsum);
      if ((lane & 15) == 0) rsum[n.ti] = r;
    }
    n.uc = un; n.vc = vn;
  }
  WSTAMP(4);
  if (LAST || RPROD) {
    __syncthreads();                 // every node has read its results: the result tiles are free
    WSTAMP(5);
    if (RPROD) wring_partials_finish(a, Ld, lds, bx, tid);
    if (LAST) {
      // [value][thread] through the space of the result tiles, one wave per value (fixed order), eight waves side by side
      // (tail: sixteen more entries per value, the boundary-line nodes of this tile's job -- zeros where there is none)
      constexpr int RS = TAIL ? 272 : 256;
      double* red = lds + Ld.RES;
      if (tid < 256) {
#pragma unroll
        for (int q = 0; q < PS_N; ++q) red[q * RS + tid] = v[q];
      }
      // waves 6 and 7 finish the job's nodes from what the four waves left in LDS in front of the barrier: wave 7 the palinstrophy
      // share (the lines of the stage-3 window; the streamed part of grad omega: slot 4 of the partials), wave 6 the residuals
      if (TAIL && wv == 7 && job) wedge_finish<5, DIAGV>(a, Ld, lds, jb, lane, ev);
      if (TAIL && wv == 6) {
        if (job) { wedge_finish<3, DIAGV>(a, Ld, lds, jb, lane, ev); wedge_finish<4, DIAGV>(a, Ld, lds, jb, lane, ev); }
        if (lane < 16) {
#pragma unroll
          for (int q = 0; q < PS_N; ++q) red[q * RS + 256 + lane] = ev[q];
        }
      }
      __syncthreads();
      const int nwp = wrows_padded(nwg);
      {
        const double* r = red + wv * RS + lane;
        double y = ((r[0] + r[64]) + r[128]) + r[192];
        if (TAIL) y += (lane < 16) ? r[256] : 0.0;
        const double x = wave_sum(y);
        if (lane == 0) wst1(a.part4 + (size_t)wv * nwp + wopaque_s(bx), x);          // kStageWaves == PS_NSUM
      }
      if (wv < 2) {
        const double* r = red + (PS_NSUM + wv) * RS + lane;
        double y = fmax(fmax(r[0], r[64]), fmax(r[128], r[192]));
        if (TAIL) y = fmax(y, (lane < 16) ? r[256] : 0.0);
        const double x = wave_max(y);
        if (lane == 0) wst1(a.part4 + (size_t)(PS_NSUM + wv) * nwp + wopaque_s(bx), x);
      }
      if (DIAGV && tid == 64 * 3) {
        // the palinstrophy sum of stage 3 (+ the share of a boundary-line job, formed beside this stage's epilogue)
        const double* r = rsum;
        const double x = (((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))) +
                         (((r[8] + r[9]) + (r[10] + r[11])) + ((r[12] + r[13]) + (r[14] + r[15])));
        const int step0 = S->step;
        wst1(a.partP0 + (size_t)((step0 > 0 ? step0 - 1 : 0) & 1) * a.stride + wopaque_s(bx), TAIL ? x + r[16] : x);
        S->pdone = step0; S->drows = nwg;                    // Z and P partials of state `step0` are complete
      }
      if (tid == 0) S->step = S->step + 1;                   // one more state update done (read by the fold, two barriers later)
    }
  }
  WSTAMP(6);
  // ---------------------------------------------------------------- hand-over.  Every wave: its own write-through stores are
  // acknowledged (vmcnt(0)), then it arrives at a counter in LDS.  Wave 0 waits for all eight arrivals, raises this work-group's
  // flag and polls the mates' (any two work-groups share a mate, so a work-group two hand-overs ahead of another is impossible:
  // the write-after-read side is covered too).  Waves 4-7 use the time for the window's work; the work-group barrier ends the
  // stage.  (A work-group barrier in front of the flag, as in the small-N kernel, would hold waves 4-7 idle for ~6 000 cycles.)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  WSTAMP(7);
  ++phaseA;
  if (lane == 0) __hip_atomic_fetch_add(&S->arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  if (wv == 0) {
    const unsigned want = 8u * (phaseA - 1u);                // (the entry hand-over, phase 1, has barriers of its own)
    while (__hip_atomic_load(&S->arrive, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < want) __builtin_amdgcn_s_sleep(1);
    WSTAMP(8);
    if (tid == 0) __hip_atomic_store((LDC_GLOBAL unsigned*)a.flags + 32 * bx, phaseA, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!wwait_flags(a.flags, phaseA, T, I, J, false, tid) && tid == 0) wgive_up(a, S);
    WSTAMP(9);
  } else if (wv >= 4) {
    // ------------------------------------------------------------ [W] the window
    // the fold's second half: what it stores (the record, by work-group 0) no other work-group reads
    if (K == 0 && wv == 7 && fold) wfold_record(a, Ld, lds, S, T, lane, bx == 0, fs, fx, stp);
    if (TAIL && K == 0 && job && jb.kind < 2 && wv < 7) {
      // the streamed dot products of stage 1 for this tile's job: phi^(n+1) and p^(n+1) are what this stage read (wave 7 is busy
      // with the fold's record: wave 6 takes two shares)
      wedge_stream<1, DIAGV>(a, Ld, lds, jb.kind, jb.blk, io, T, wv - 4, lane);
      if (wv == 6) wedge_stream<1, DIAGV>(a, Ld, lds, jb.kind, jb.blk, io, T, 3, lane);
    }
    if (WLINES) {
      // this tile's ring lines for the epilogue of stage 4 (the ring vectors were published two hand-overs ago)
      if (wv == 4 && (J == 0 || J == jLast)) wring_line(a, T, I, lane, 0, J == 0 ? 0 : 1, rng);
      if (wv == 5 && (I == 0 || I == iLast)) wring_line(a, T, J, lane, 1, I == 0 ? 0 : 1, rng + 32);
      if (job) {
        // the jobs' share: the streamed product of grad omega (all four waves); ring line c = 1 at the job's nodes and the two
        // nodes where it meets the ring lines of index 0 (wave 7); the line product of grad omega, the corner's values (wave 6)
        const size_t rowm = (size_t)(a.M - 1) * a.LD;
        if (DIAGV && jb.kind < 2) wedge_stream<3, DIAGV>(a, Ld, lds, jb.kind, jb.blk, io, T, wv - 4, lane);
        if (wv >= 6 && jb.kind < 2) {
          // the job's ring line c = 1 (kind 0: d/dy p at (M-1, 16 J + r) from s_1 and GyF[J]; kind 1: d/dx p at (16 I + r, M-1) from a_1
          // and GxF[I]), half of the contraction range per wave, one batch each
          const int h0 = (T + 1) / 2, g0 = wv == 6 ? 0 : h0, ng = wv == 6 ? h0 : T - h0;
          const int lk = jb.kind == 0 ? 1 : 0;                  // the line's kind: rows for a row job's nodes, columns for a column job's
          WVecHalf vh;
          wvec_issue(vh, a.rvec, (size_t)(2 * lk + 1) * 16 * T, g0, ng, lane);
          wvec_finish(vh, nullptr, lk == 0 ? a.GxFK : a.GyFK, jb.blk, NB, g0, ng, lane,
                      wv == 6 ? rng + (jb.kind == 0 ? 48 : 16) : rng + WR_JOBRING2);
          if (wv == 7 && jb.blk == 0) {
            const double e = jb.kind == 0 ? wvv(a.GxF + rowm, a.rvec, 0, 16 * T, lane)
                                          : wvv(a.GyF + rowm, a.rvec, (size_t)2 * 16 * T, 16 * T, lane);
            if (lane == 0) rng[WR_EXTRA] = e;
          }
        } else if (wv == 6 && jb.kind == 2) {
          const double pxc = wvv(a.GxF + rowm, a.rvec, (size_t)16 * T, 16 * T, lane);            // GxF[M-1] . a_1
          const double pyc = wvv(a.GyF + rowm, a.rvec, (size_t)3 * 16 * T, 16 * T, lane);        // s_1 . GyF[M-1]
          if (lane == 0) { rng[WR_CPX] = pxc; rng[WR_CPY] = pyc; }
        }
      }
    }
  }
  __syncthreads();
  WSTAMP(10);
  return S->abort == 0;
}

template <bool SP, bool DIAGV, bool TAIL>
__global__ __launch_bounds__(kStageThreads, 2) void wide_kernel(const WLaunch L) {
  static_assert(!(SP && DIAGV), "the smoother carries no diagnostics");
  static_assert(!(SP && TAIL), "the tail layout is built for SG");
  extern __shared__ __attribute__((aligned(16))) double lds[];
  __shared__ TrialState S;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  // ---- which trial, which tile: blockIdx.x = trial * T*T + tile (all trials of a launch share the geometry)
  WArgsC& a0 = L.trials ? *(WArgsC*)(uintptr_t)L.trials
                        : *(WArgsC*)((kernarg_ptr)__builtin_amdgcn_kernarg_segment_ptr() + __builtin_offsetof(WLaunch, one));
  const int T = a0.T, nwg = T * T;
  const int trial = (int)blockIdx.x / nwg, bx = (int)blockIdx.x % nwg;
  WArgsC& a = L.trials ? *(WArgsC*)(uintptr_t)(L.trials + trial) : a0;
  const WLds Ld = wlds_of(T);
  const int NB = a.NB, M = a.M, LD = a.LD;
  const int I = bx / T, J = bx % T;
  // Everything past the geometry (T, and NB / M / LD, equal in a launch group) comes from the trial's own block `a`: its state,
  // ctrl / scal words, flags, give-up word, ring / rvec / wedge / jobs, partials.  A trial latched before the launch (converged,
  // capped by the host, NaN) leaves at once -- every work-group of the trial reads the same word, nobody writes it before the
  // exit -- and touches nothing, its own words or another trial's of the group.
  if (a.fin.ctrl[LDC_CTRL_DONE] != 0) return;
  if (tid == 0) {
    S.done = a.fin.ctrl[LDC_CTRL_DONE]; S.iter = a.fin.ctrl[LDC_CTRL_ITER]; S.step = a.fin.ctrl[LDC_CTRL_STEP];
    S.flushed = a.fin.ctrl[LDC_CTRL_FLUSHED]; S.pdone = a.fin.ctrl[LDC_CTRL_PDONE]; S.drows = a.fin.ctrl[LDC_CTRL_DROWS];
    S.dt = a.fin.scal[LDC_SCAL_DT]; S.umax = a.fin.scal[LDC_SCAL_UMAX]; S.vmax = a.fin.scal[LDC_SCAL_VMAX];
    S.abort = 0; S.arrive = 0u; S.dtp = 0.0;
  }
  // ---- the operator panels of this tile, resident for the whole launch: Dx[I], D2x[I], Dy[J], D2y[J]; element (lane, s) of a
  // packed fragment goes to [half s >> 1][lane][s & 1], so that an operand read is two linear 16-byte reads per lane
  for (int q = tid; q < 4 * T * 256; q += kStageThreads) {
    const int p = q / (T * 256), r = q - p * (T * 256), g = r >> 8, e = r & 255;
    const double* src = p == 0 ? a.DxK : p == 1 ? a.D2xK : p == 2 ? a.DyK : a.D2yK;
    const int row = p < 2 ? I : J;
    lds[Ld.OPS + (p * T + g) * 256 + ((e & 3) >> 1) * 128 + (e >> 2) * 2 + (e & 1)] = src[((size_t)(row * NB + g) << 8) + e];
  }
  // ---- the node of this thread (waves 0-3) from the row-major phi^n
  XNode n;
  n.ti = 4 * (wv & 3) + (lane >> 4); n.tj = lane & 15;
  n.i = 16 * I + n.ti; n.j = 16 * J + n.tj;
  n.oU = xpk(n.ti, n.tj); n.oT = xpk(n.tj, n.ti);
  const int Mx = a.Mx, My = a.My;          // (== M unless nx != ny)
  n.valid = (n.i < Mx) && (n.j < My);
  n.interior = (n.i >= 1) && (n.i <= Mx - 2) && (n.j >= 1) && (n.j <= My - 2);
  n.lid = n.valid && (n.j == My - 1);
  n.wall = n.valid && (n.i == 0 || n.i == Mx - 1 || n.j == 0);
  n.rc = !n.valid ? -1 : n.j == 0 ? 0 : n.j == My - 1 ? 1 : -1;
  n.rr = !n.valid ? -1 : n.i == 0 ? 0 : n.i == Mx - 1 ? 1 : -1;
  n.u0 = n.v0 = n.p0 = n.px = n.py = n.lidv = n.wq = 0.0;
  const size_t ij = (size_t)n.i * LD + n.j;
  if (tid < 64) {          // the ring rows of IyF at this tile's columns, of IxF at its rows
    const int c = (tid >> 4) & 1, e = tid & 15;
    const size_t row = c ? (size_t)((tid < 32 ? My : Mx) - 1) * LD : 0;      // IyF[0 | My-1], IxF[0 | Mx-1]
    lds[Ld.EYX + tid] = (tid < 32) ? a.IyF[row + 16 * J + e] : a.IxF[row + 16 * I + e];
  }
  if (tid < 256) {
    n.u0 = a.U[ij]; n.v0 = a.V[ij]; n.p0 = a.P[ij];        // zero padded: any (i, j) < LD is readable
    n.lidv = a.ulid[n.i];
    n.wq = a.wx[n.i] * a.wy[n.j];
    // every block of the packed phi^n buffers this trial reads: this tile's blocks from the row-major values just read
    wst(a.UK[0], I * NB + J, n.oU, n.u0); wst(a.UTK[0], J * NB + I, n.oT, n.u0);
    wst(a.VK[0], I * NB + J, n.oU, n.v0); wst(a.VTK[0], J * NB + I, n.oT, n.v0);
    wst(a.PK[0], I * NB + J, n.oU, n.p0);
    wst(a.PTK[0], J * NB + I, n.oT, n.p0);
  }
  if (!SP) {                   // SG: the ring of grad p^n comes from the partials of p^n
    __syncthreads();           // (the tables above)
    if (tid < 256) wring_partials(a, Ld, n, lds, n.p0, bx, lane, wv);
    __syncthreads();
    wring_partials_finish(a, Ld, lds, bx, tid);
  }
  n.uc = n.u0; n.vc = n.v0;
  // ---- tail layout: what index M-1 adds at this tile node (constants: the lines of index M-1 hold boundary values), this tile's job
  WTailNode tn = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  int jkind = -1, jblk = 0;
  if (TAIL) {
    if (tid < 256) {
      const size_t rowm = (size_t)(M - 1) * LD;
      const double dxl = a.DxL[n.i], d2xl = a.D2xL[n.i], dyl = a.DyL[n.j], d2yl = a.D2yL[n.j];
      const double ue = a.U[rowm + n.j], ve = a.V[rowm + n.j];        // east-wall row (M-1, j)
      const double un = a.UT[rowm + n.i], vn = a.VT[rowm + n.i];      // lid column (i, M-1), read along the transposed copy
      tn.cux = dxl * ue; tn.cvx = dxl * ve; tn.cuy = un * dyl; tn.cvy = vn * dyl;
      tn.clu = nm_madd(d2xl, ue, un * d2yl); tn.clv = nm_madd(d2xl, ve, vn * d2yl);
      tn.dxl = dxl; tn.dyl = dyl;
    }
    jkind = (I == J) ? 0 : (J == (I + 1) % T) ? 1 : (I == 1 && J == 3) ? 2 : -1;
    jblk = jkind == 0 ? J : I;
    if (wv == 6 && jkind >= 0) {
      // The job's constants (boundary values, their derivatives along the line, weights: ~70 wave-wide dot products over the full
      // index, 30-50 us with every other tile waiting at the entry hand-over) are the same for every launch of a solver: formed by
      // the first one, tagged, kept in the job's block of the sync array (zeroed when the solver is made).
      double* jbase = a.jobs + (size_t)wjob_id(jkind, jblk, T) * kWJobDoubles;
      if (xld(jbase, WJ_UNI * 16 + 3) != kWJobTag) {
        WJob jb;
        wjob_init(a, jb, T, I, J, lane);
        wjob_store(a, jb, T, lane, true);
        if (lane == 0) wst1(jbase + WJ_UNI * 16 + 3, kWJobTag);
      }
    }
    if (tid < 16) lds[Ld.RSUM + 16 + tid] = 0.0;
  }
  unsigned phaseA = 0;
  bool alive = wbar(a, phaseA, T, bx, I, J, tid, &S, true);
  bool pending = false;        // an iteration whose stage 4 has run awaits its fold
  for (int it = 0; alive && it < L.n_iters; ++it) {
    if (S.done != 0) break;                                  // every work-group holds the same latch
#ifdef LDC_TIMING
    const bool stamp = a.stamps != nullptr && it == L.n_iters - 1;
#else
    const bool stamp = false;
#endif
    alive = wstage<SP, DIAGV, TAIL, 0>(a, Ld, n, tn, jkind, jblk, lds, &S, phaseA, T, bx, I, J, pending, stamp);
    if (!alive) break;
    pending = false;
    // the fold of the iteration before (its record and latch were decided beside this stage's epilogue): latched -> phi^n,
    // which only stage 4 overwrites, is the state the solve ends with; what stage 1 has stored is stage-buffer content
    if (S.done != 0) break;
    alive = wstage<SP, DIAGV, TAIL, 1>(a, Ld, n, tn, jkind, jblk, lds, &S, phaseA, T, bx, I, J, false, stamp);
    if (!alive) break;
    alive = wstage<SP, DIAGV, TAIL, 2>(a, Ld, n, tn, jkind, jblk, lds, &S, phaseA, T, bx, I, J, false, stamp);
    if (!alive) break;
    alive = wstage<SP, DIAGV, TAIL, 3>(a, Ld, n, tn, jkind, jblk, lds, &S, phaseA, T, bx, I, J, false, stamp);
    pending = true;
  }
  if (!alive) return;
  if (pending) {               // close the last iteration of the chunk
    if (wv == 7) {
      v4d fx[PS_N + 2];
      const WFoldState fs = wfold_dt(a, &S, T, I, J, lane, phaseA, fx, nullptr);
      wfold_step(a, &S, fs, lane);
      wfold_record(a, Ld, lds, &S, T, lane, bx == 0, fs, fx, nullptr);
    }
    __syncthreads();
    if (S.abort != 0) return;
  }
  // ---- leave both forms of phi behind: the packed buffers hold it already, the row-major arrays from the registers
  double* tu = lds + Ld.RES;
  double* tv = tu + 16 * 17;
  if (tid < 256) {
    a.U[ij] = n.u0; a.V[ij] = n.v0; a.P[ij] = n.p0;
    tu[n.ti * 17 + n.tj] = n.u0; tv[n.ti * 17 + n.tj] = n.v0;
  }
  __syncthreads();
  if (tid < 256) {
    const int tr = tid >> 4, tc = tid & 15;
    const size_t ot = (size_t)(16 * J + tr) * LD + 16 * I + tc;
    a.UT[ot] = tu[tc * 17 + tr];
    a.VT[ot] = tv[tc * 17 + tr];
  }
  if (bx == 0 && tid == 0) {
    a.fin.ctrl[LDC_CTRL_DONE] = S.done; a.fin.ctrl[LDC_CTRL_ITER] = S.iter; a.fin.ctrl[LDC_CTRL_STEP] = S.step;
    a.fin.ctrl[LDC_CTRL_FLUSHED] = S.flushed; a.fin.ctrl[LDC_CTRL_PDONE] = S.pdone; a.fin.ctrl[LDC_CTRL_DROWS] = S.drows;
    a.fin.ctrl[LDC_CTRL_LIVE] = 0;                           // every iteration of this launch has been closed in it
    a.fin.scal[LDC_SCAL_DT] = S.dt; a.fin.scal[LDC_SCAL_UMAX] = S.umax; a.fin.scal[LDC_SCAL_VMAX] = S.vmax;
  }
}
