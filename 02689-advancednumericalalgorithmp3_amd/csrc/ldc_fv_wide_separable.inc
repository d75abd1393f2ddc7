// ldc_fv_wide_separable.inc -- the separable scaled preconditioner of a lone chip trial on a wall-clustered grid
// (include/ldc_fv.h, "The separable scaled preconditioner of a chip trial"; ldc_fv_wide_set_preconditioner).  Included by
// ldc_fv_wide.hip alone, inside its anonymous namespace, behind ldc_fv_wide_stretched.inc: the launches below are part of
// that unit's iteration and of its captured graph.
//
// The stretched consistent chain preconditions its CG by the operator with D = V / a_P left out.  With the tables of
// ldc_fv_stretched_sep.hip attached -- per axis [a (n) | lam (n) | Q (n x n)], D fitted by a_i b_j -- the chain is, launch for
// launch, in the same grids and with the same `par`, slots and budget protocol,
//   sg_faces<true> | init* | np x (gemm x 4* | rz* | ap* | xr*) | pfinish | sg_correct | sg_fluxvort<true>
// with z = s . L_s+ (s . r), s_c = sqrt(a_i b_j / D_c) (sg_sep_scale, the one-CU kernel's):
//   init*   wide_pcg_init, and s and s . b into the work vectors WSEP_S, WSEP_SR
//   gemm*   the kernels fv_wide_pcg_gemm as they are, on a copy of the arguments whose descriptor carries Qx, lamx, Qy, lamy
//           of the separable tables and dx = dy = 1 (wide_sep_args); the first one reads s . r (wide_sep_gemm_of).  PCG_Z
//           then holds z' = L_s+ (s . r), the (0, 0) mode dropped by the epilogue as before
//   rz*     slot: (s . r) . z', which is r . z (the sum of the one-CU loop)
//   ap*     wide_sg_pcg_ap with z = s . z' wherever it reads z: at the cell and at its four neighbours
//   xr*     wide_pcg_xr, and s . r for the next GEMM
// The head test of the first GEMM, pfinish and everything outside the solve are launched as they are: the stop rule is on
// |r|, the operator, b and x = 0 are the same, so a trial differs from its laplacian run at the level of pressure_tol.
// By the rules of the chip mapping: uniform control flow, bounded loops, sums through the slots in the fixed order, no
// atomics, no flags, no waits; nobody reads what another work-group of the same launch writes (s, s . r and r are written
// at a thread's own cell and read by later launches).

// s and s . r: vectors of BiCGSTAB that nothing between linfinish and record reads (the one-CU kernel's vector 15 is the
// second copy of p here, and 16 is q)
constexpr FvVec WSEP_S = FV_PHV, WSEP_SR = FV_SHU;
static_assert(PCG_MS < PCG_Q && WSEP_S > PCG_Q + 1 && WSEP_SR > PCG_Q + 1 && WSEP_S < FV_C && WSEP_SR < FV_C && WSEP_S != WSEP_SR,
              "the scaling vectors are clear of the CG vectors PCG_MS .. PCG_Q + 1 and of FV_C ...");

// the arguments of the four GEMMs: the eigenpairs of the fitted operator, divisor lamy[a] + lamx[b]
__host__ __device__ inline FvWideArgs wide_sep_args(const FvWideArgs& a, const FvPrecondBlk& pb) {
  FvWideArgs s = wide_sg_neutral(a);
  s.d.lamx = pb.px + s.d.nx; s.d.Qx = pb.px + 2 * s.d.nx;
  s.d.lamy = pb.py + s.d.ny; s.d.Qy = pb.py + 2 * s.d.ny;
  return s;
}

// wide_pcg_gemm_of with s . r for r
__host__ __device__ inline FvWideGemm wide_sep_gemm_of(const FvDesc& d, int which) {
  FvWideGemm g = wide_pcg_gemm_of(d, which);
  if (which == 0) g.B = d.work + (int64_t)WSEP_SR * d.nx * d.ny;
  return g;
}

// ---- init*: r = b, x = 0, s, s . b; slot: |b|^2
__device__ __forceinline__ void wide_sep_init(const FvWideArgs& a, const FvGridBlk& gb, const FvPrecondBlk& pb, int g, int par,
                                              double* lds) {
  if (wide_pcg_gate(a)) return;
  const FvCtx x(a.d);
  const SgCtx sg(x, gb);
  const int nx = x.nx;
  double csum[1];
  wide_slot_sum(wide_slots(a, par), a.G, 0, csum, lds);
  const double b00 = -csum[0];
  double b2[1] = {0.0};
  for (int c = g * kWT + threadIdx.x; c < x.n; c += a.G * kWT) {
    const double b = c == 0 ? b00 : x.vec(FV_C)[c];
    const double sc = sg_sep_scale(sg, pb.px, pb.py, c, c % nx, c / nx);
    x.vec(PCG_R)[c] = b;
    x.vec(FV_Y)[c] = 0.0;
    x.vec(WSEP_S)[c] = sc;
    x.vec(WSEP_SR)[c] = sc * b;
    b2[0] += b * b;
  }
  wide_slot_put(wide_slots(a, par ^ 1), g, 0, b2, lds);
}

// ---- rz*; slot: (s . r) . z'
__device__ __forceinline__ void wide_sep_rz(const FvWideArgs& a, int g, int par, double* lds) {
  if (wide_pcg_gate(a)) return;
  const FvCtx x(a.d);
  WidePcgScalars s;
  wide_pcg_load(wide_kry(a, par), s);
  wide_pcg_store(wide_kry(a, par ^ 1), g, s);
  if (!s.act) return;
  double rz[1] = {0.0};
  const double *sr = x.vec(WSEP_SR), *z = x.vec(PCG_Z);
  for (int c = g * kWT + threadIdx.x; c < x.n; c += a.G * kWT) rz[0] += sr[c] * z[c];
  wide_slot_put(wide_slots(a, par ^ 1), g, 0, rz, lds);
}

// ---- ap*: the frame of wide_sg_pcg_ap, z = s . z'
__device__ __forceinline__ void wide_sep_ap(const FvWideArgs& a, const FvGridBlk& gb, int g, int it, int par, double* lds) {
  if (wide_pcg_gate(a)) return;
  const FvCtx x(a.d);
  const SgCtx sg(x, gb);
  WidePcgScalars s;
  wide_pcg_load(wide_kry(a, par), s);
  if (s.act) {
    double rz[1];
    wide_slot_sum(wide_slots(a, par), a.G, 0, rz, lds);
    s.beta = it > 0 ? rz[0] / s.rz : 0.0;
    s.rz = rz[0];
  }
  wide_pcg_store(wide_kry(a, par ^ 1), g, s);
  if (!s.act) return;
  const int nx = x.nx;
  const double beta = s.beta;
  const double *z = x.vec(PCG_Z), *sc = x.vec(WSEP_S), *pold = x.vec(PCG_P, (it & 1) ^ 1);
  double *pnew = x.vec(PCG_P, it & 1), *q = x.vec(PCG_Q);
  double pq[1] = {0.0};
  for (int c = g * kWT + threadIdx.x; c < x.n; c += a.G * kWT) {
    const int i = c % nx, j = c / nx;
    // (the same expression for the cell and for its neighbours: every thread gets the p its neighbour writes)
#define PCG_PV(k) (it > 0 ? fma(beta, pold[k], sc[k] * z[k]) : sc[k] * z[k])
    const double pc = PCG_PV(c);
    const double y = sg_row(sg, c, i, j, pc, [&](int k) { return PCG_PV(k); });
#undef PCG_PV
    pnew[c] = pc; q[c] = y;
    pq[0] += pc * y;
  }
  wide_slot_put(wide_slots(a, par ^ 1), g, 0, pq, lds);
}

// ---- xr*: alpha, x += alpha p, r -= alpha q, s . r; slot: |r|^2
__device__ __forceinline__ void wide_sep_xr(const FvWideArgs& a, int g, int it, int par, double* lds) {
  if (wide_pcg_gate(a)) return;
  const FvCtx x(a.d);
  WidePcgScalars s;
  wide_pcg_load(wide_kry(a, par), s);
  if (s.act) {
    double pq[1];
    wide_slot_sum(wide_slots(a, par), a.G, 0, pq, lds);
    s.alpha = s.rz / pq[0];
  }
  wide_pcg_store(wide_kry(a, par ^ 1), g, s);
  if (!s.act) return;
  const double alpha = s.alpha;
  const double *p = x.vec(PCG_P, it & 1), *q = x.vec(PCG_Q), *sc = x.vec(WSEP_S);
  double *xs = x.vec(FV_Y), *r = x.vec(PCG_R), *sr = x.vec(WSEP_SR);
  double r2[1] = {0.0};
  for (int c = g * kWT + threadIdx.x; c < x.n; c += a.G * kWT) {
    xs[c] += alpha * p[c];
    const double rn = r[c] - alpha * q[c];
    r[c] = rn;
    sr[c] = sc[c] * rn;
    r2[0] += rn * rn;
  }
  wide_slot_put(wide_slots(a, par ^ 1), g, 0, r2, lds);
}

// ---- the kernels: a lone trial only, as in ldc_fv_wide_stretched.inc
#define WIDE_SEP_LDS __shared__ double lds[kWW * kWS]
__global__ __launch_bounds__(kWT) void fv_wide_sep_init(FvWideArgs a, FvGridBlk gb, FvPrecondBlk pb, int par) {
  WIDE_SEP_LDS;
  wide_sep_init(a, gb, pb, blockIdx.x, par, lds);
}
__global__ __launch_bounds__(kWT) void fv_wide_sep_rz(FvWideArgs a, int par) {
  WIDE_SEP_LDS;
  wide_sep_rz(a, blockIdx.x, par, lds);
}
__global__ __launch_bounds__(kWT) void fv_wide_sep_ap(FvWideArgs a, FvGridBlk gb, int it, int par) {
  WIDE_SEP_LDS;
  wide_sep_ap(a, gb, blockIdx.x, it, par, lds);
}
__global__ __launch_bounds__(kWT) void fv_wide_sep_xr(FvWideArgs a, int it, int par) {
  WIDE_SEP_LDS;
  wide_sep_xr(a, blockIdx.x, it, par, lds);
}
#undef WIDE_SEP_LDS
