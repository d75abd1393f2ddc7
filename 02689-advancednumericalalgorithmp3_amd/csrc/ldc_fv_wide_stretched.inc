// ldc_fv_wide_stretched.inc -- a lone chip trial on a wall-clustered tensor grid (include/ldc_fv.h, "Stretched grids of a chip
// trial"; ldc_fv_wide_set_grid).  Included by ldc_fv_wide.hip alone, inside its anonymous namespace, behind
// ldc_fv_wide_pressure.inc: the launches below are part of that unit's iteration and of its captured graph.
//
// The phases of the chain that read the geometry get a twin here that reads it from the per-axis tables [h | d | g] of
// ldc_fv_set_grid (FvGridBlk: two pointers, by value in the kernel arguments):
//   assemble | faces, pcg_faces | correct | fluxvort, pcg_fluxvort | sums | pcg_ap
// Each twin is the uniform phase's frame -- the gate, the grid-stride cell loop, the slots, `par` -- around the cell body of
// ldc_fv_stretched_cells.inc, which the one-CU stretched kernels (ldc_fv_stretched.hip, ldc_fv_stretched_sep.hip) call too: the
// arithmetic has one definition.  Everything else of the chain is launched as it is: the BiCGSTAB sweeps and linfinish read
// the stored diagonals only, pcg_init, pcg_rz, pcg_xr and pfinish read vectors only, and the GEMMs take Qx, lamx, Qy, lamy
// from the descriptor, which the caller fills with the generalised eigenpairs of the grid.  Two launches read dx, dy for
// what the stretched sums and eigenvalues already carry: the scaled GEMM (the divisor is lamy[a] + lamx[b]: ax = ay = 1) and
// `record` (V = 1: the sums of E, Z and P carry each cell's volume); the chain hands them a copy of the arguments with
// dx = dy = 1 (wide_sg_neutral).
// The chain of a stretched trial has the uniform chain's launches one for one, in the same grids: the launch count, the
// budget protocol, the slots and the scratch are those of ldc_fv_wide.hip, and so are its rules.

// the arguments with dx = dy = 1, for the launches that must not scale by the spacing
__host__ __device__ inline FvWideArgs wide_sg_neutral(const FvWideArgs& a) {
  FvWideArgs n = a;
  n.d.dx = 1.0; n.d.dy = 1.0;
  return n;
}

// ---- 1. twin of wide_assemble
__device__ __forceinline__ void wide_sg_assemble(const FvWideArgs& a, const FvGridBlk& gb, int g, int par, double* lds) {
  if (wide_gate(a)) return;
  const FvCtx x(a.d);
  const SgCtx s(x, gb);
  double b2[2] = {0.0, 0.0};
  for (int c = g * kWT + threadIdx.x; c < x.n; c += a.G * kWT) sg_cell_assemble(s, c, b2);
  wide_slot_put(wide_slots(a, par ^ 1), g, 0, b2, lds);
}

// ---- 3. twin of wide_faces (PCG: of wide_pcg_faces, mdot* left in the work vectors PCG_MS)
template <bool PCG>
__device__ __forceinline__ void wide_sg_faces(const FvWideArgs& a, const FvGridBlk& gb, int g, int par, double* lds) {
  if (PCG ? wide_pcg_gate(a) : wide_gate(a)) return;
  const FvCtx x(a.d);
  const SgCtx s(x, gb);
  double* fx = PCG ? x.vec(PCG_MS) : x.fx;
  double* fy = PCG ? x.vec(PCG_MS) + x.ny * x.ldx : x.fy;
  double csum[1] = {0.0};
  for (int c = g * kWT + threadIdx.x; c < x.n; c += a.G * kWT) {
    double rhs;
    sg_cell_faces(s, fx, fy, c, rhs);
    csum[0] += rhs;
  }
  wide_slot_put(wide_slots(a, par ^ 1), g, 0, csum, lds);
}

// ---- twin of wide_pcg_ap: the row of A from the tables
__device__ __forceinline__ void wide_sg_pcg_ap(const FvWideArgs& a, const FvGridBlk& gb, int g, int it, int par, double* lds) {
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
  const double *z = x.vec(PCG_Z), *pold = x.vec(PCG_P, (it & 1) ^ 1);
  double *pnew = x.vec(PCG_P, it & 1), *q = x.vec(PCG_Q);
  double pq[1] = {0.0};
  for (int c = g * kWT + threadIdx.x; c < x.n; c += a.G * kWT) {
    const int i = c % nx, j = c / nx;
    // (the same expression for the cell and for its neighbours: every thread gets the p its neighbour writes)
#define PCG_PV(k) (it > 0 ? fma(beta, pold[k], z[k]) : z[k])
    const double pc = PCG_PV(c);
    const double y = sg_row(sg, c, i, j, pc, [&](int k) { return PCG_PV(k); });
#undef PCG_PV
    pnew[c] = pc; q[c] = y;
    pq[0] += pc * y;
  }
  wide_slot_put(wide_slots(a, par ^ 1), g, 0, pq, lds);
}

// ---- 5. twin of wide_correct
__device__ __forceinline__ void wide_sg_correct(const FvWideArgs& a, const FvGridBlk& gb, int g, double* lds) {
  if (wide_gate(a)) return;
  const FvCtx x(a.d);
  const SgCtx s(x, gb);
  const double y0 = x.vec(FV_Y)[0];
  double part[7] = {0, 0, 0, 0, 0, 0, 0};
  for (int c = g * kWT + threadIdx.x; c < x.n; c += a.G * kWT) sg_cell_correct(s, y0, c, part);
  wide_slot_put(wide_rec_slots(a), g, 0, part, lds);
}

// ---- 6. twin of wide_fluxvort (PCG: of wide_pcg_fluxvort)
template <bool PCG>
__device__ __forceinline__ void wide_sg_fluxvort(const FvWideArgs& a, const FvGridBlk& gb, int g, double* lds) {
  if (PCG ? wide_pcg_gate(a) : wide_gate(a)) return;
  const FvCtx x(a.d);
  const SgCtx s(x, gb);
  double part[1] = {0.0};
  for (int c = g * kWT + threadIdx.x; c < x.n; c += a.G * kWT) sg_cell_fluxvort<PCG>(s, c, part[0]);
  wide_slot_put(wide_rec_slots(a), g, 8, part, lds);
}

// ---- 7a. twin of wide_sums
__device__ __forceinline__ void wide_sg_sums(const FvWideArgs& a, const FvGridBlk& gb, int g, double* lds) {
  if (wide_gate(a)) return;
  const FvCtx x(a.d);
  const SgCtx s(x, gb);
  double p7[1] = {0.0}, p9[1] = {0.0};
  for (int c = g * kWT + threadIdx.x; c < x.n; c += a.G * kWT) sg_cell_sums(s, c, p7[0], p9[0]);
  wide_slot_put(wide_rec_slots(a), g, 7, p7, lds);
  wide_slot_put(wide_rec_slots(a), g, 9, p9, lds);
}

// ---- the kernels: a lone trial only (arguments and the grid block by value, g = blockIdx.x); a batch takes no such trial
#define WIDE_SG_LDS __shared__ double lds[kWW * kWS]
__global__ __launch_bounds__(kWT) void fv_wide_sg_assemble(FvWideArgs a, FvGridBlk gb, int par) {
  WIDE_SG_LDS;
  wide_sg_assemble(a, gb, blockIdx.x, par, lds);
}
template <bool PCG>
__global__ __launch_bounds__(kWT) void fv_wide_sg_faces(FvWideArgs a, FvGridBlk gb, int par) {
  WIDE_SG_LDS;
  wide_sg_faces<PCG>(a, gb, blockIdx.x, par, lds);
}
__global__ __launch_bounds__(kWT) void fv_wide_sg_pcg_ap(FvWideArgs a, FvGridBlk gb, int it, int par) {
  WIDE_SG_LDS;
  wide_sg_pcg_ap(a, gb, blockIdx.x, it, par, lds);
}
__global__ __launch_bounds__(kWT) void fv_wide_sg_correct(FvWideArgs a, FvGridBlk gb) {
  WIDE_SG_LDS;
  wide_sg_correct(a, gb, blockIdx.x, lds);
}
template <bool PCG>
__global__ __launch_bounds__(kWT) void fv_wide_sg_fluxvort(FvWideArgs a, FvGridBlk gb) {
  WIDE_SG_LDS;
  wide_sg_fluxvort<PCG>(a, gb, blockIdx.x, lds);
}
__global__ __launch_bounds__(kWT) void fv_wide_sg_sums(FvWideArgs a, FvGridBlk gb) {
  WIDE_SG_LDS;
  wide_sg_sums(a, gb, blockIdx.x, lds);
}
#undef WIDE_SG_LDS
