// ldc_fv_wide_pressure.inc -- the consistent pressure correction of a chip or shared trial (include/ldc_fv.h,
// ldc_fv_wide_set_pressure).  Included by ldc_fv_wide.hip alone, inside its anonymous namespace, behind the phases of the
// SIMPLE iteration and beside ldc_fv_wide_anderson.inc: the launches below are part of that unit's iteration and of its
// captured graph.
//
// The reference's pressure-correction matrix is the constant-coefficient Laplacian rho |S| / d, while the velocities are
// corrected by u' = -D grad p', D = V / a_P.  A trial with a_P-weighted faces (FvWideArgs::pmax > 0) solves
//   (A x)_P = sum over the inner faces f of P of w_f (x_P - x_N) = b,   w_f = rho (D_P / 2 + D_N / 2) |S_f| / d_f,
// b = rhs_p with entry 0 = minus the sum of the others, by conjugate gradients from x = 0, preconditioned by z = L+ r: the
// four GEMMs of the fast diagonalisation with the zero mode dropped (fv_gemm_tile and the GEMM launch geometry of the
// reference chain; no entry-0 insertion, no shift).  It stops at |r|_2 <= tol |b|_2 and after pmax iterations accepts what
// it has.  p' = x - x_0 (wide_correct, unchanged), and the inner faces take mdot = mdot* - w_f (p'_N - p'_P): the face
// fluxes then conserve mass to the tolerance of the solve.  Wall faces are exactly 0.0 (FV-Q4 does not apply).
//
// The chain of such a trial between linfinish and correct, with np = min(pressure budget, pmax):
//   faces | init | np x (gemm x 4 | rz | ap | xr) | pfinish
//   faces   fv_cell_faces on a descriptor whose mdot points at three dead work vectors: mdot* waits there, and mdot is not
//           touched before the solve has finished;  slot: the sum of rhs_p
//   init    r = b (entry 0 from the slots), x = 0;  slot: |b|^2
//   gemm    z = L+ r.  The first one is the head of iteration `it`: |r|^2 from the slots (it = 0: |b|^2 and the start), the
//           stop test; work-group 0 writes the scalars
//   rz      slot: r . z
//   ap      beta = rz / rz_prev, p = z + beta p_prev and q = A p in ONE launch: a thread needs p at its four neighbours,
//           which other work-groups hold, so everybody recomputes them from z and the copy of p the launch before last
//           wrote, and writes its own entry to the other copy (the two alternate by `it`);  slot: p . q
//   xr      alpha = rz / p.q, x += alpha p, r -= alpha q;  slot: |r|^2
//   pfinish (one work-group) the last sums; a solve still active at np < pmax sets the overflow word to 2 -- u, v, p and
//           mdot are as they were, and the host enqueues the iteration again with twice the budget -- and at np = pmax it
//           is the accepted cap hit.  Then the four statistics words.
// By the rules of the chip mapping: the grids are those of a sweep and of a GEMM; partial sums go through the slots in the
// order of wide_block_sum; the scalars live where the BiCGSTAB scalars lived (two copies, alternating by `par`); the vectors
// are BiCGSTAB's, dead after linfinish; nothing waits.  A reference trial in a batch returns from every launch here before
// it reads anything (pmax == 0), and a trial of this kind returns from the reference chain's GEMMs in turn.

// (FvWidePcg, the trial's block -- the tolerance and the statistics words -- is defined in ldc_fv_wide.hip beside the table
// entry it travels in.)
constexpr int kWidePcgLaunches = LDC_FV_WIDE_PRESSURE_LAUNCHES;         // of one CG iteration
static_assert(kWidePcgLaunches == 7, "gemm x 4 | rz | ap | xr");

// (the work vectors of the solve PCG_MS, PCG_R, PCG_Z, PCG_P, PCG_Q, wide_pcg_D, wide_pcg_w, wide_pcg_row and
// wide_pcg_cell_fluxvort: ldc_fv_pressure_cells.inc, shared with ldc_fv_cu_pressure.hip)

struct WidePcgScalars {
  double bb, rr, rz, alpha, beta;
  bool act;
  int its;
};

__device__ __forceinline__ void wide_pcg_load(const double* k, WidePcgScalars& s) {
  s.bb = k[0]; s.rr = k[1]; s.rz = k[2]; s.alpha = k[3]; s.beta = k[4]; s.act = k[5] != 0.0; s.its = (int)k[6];
}

// (work-group 0 alone writes the copy the NEXT launch reads)
__device__ __forceinline__ void wide_pcg_store(double* k, int g, const WidePcgScalars& s) {
  if (g != 0 || threadIdx.x != 0) return;
  k[0] = s.bb; k[1] = s.rr; k[2] = s.rz; k[3] = s.alpha; k[4] = s.beta; k[5] = s.act ? 1.0 : 0.0; k[6] = (double)s.its;
}

__device__ __forceinline__ bool wide_pcg_gate(const FvWideArgs& a) { return a.pmax == 0 || wide_gate(a); }

__device__ __forceinline__ bool wide_pcg_done(const WidePcgScalars& s, double tol) { return sqrt(s.rr) <= tol * sqrt(s.bb); }

// ---- faces: wide_faces with mdot* left in the work vectors PCG_MS
__device__ __forceinline__ void wide_pcg_faces(const FvWideArgs& a, int g, int par, double* lds) {
  if (wide_pcg_gate(a)) return;
  FvDesc d = a.d;
  d.mdot = d.work + (int64_t)PCG_MS * d.nx * d.ny;
  const FvCtx x(d);
  double csum[1] = {0.0};
  for (int c = g * kWT + threadIdx.x; c < x.n; c += a.G * kWT) {
    double rhs;
    fv_cell_faces(x, c, rhs);
    csum[0] += rhs;
  }
  wide_slot_put(wide_slots(a, par ^ 1), g, 0, csum, lds);
}

// ---- init: r = b, x = 0; slot: |b|^2
__device__ __forceinline__ void wide_pcg_init(const FvWideArgs& a, int g, int par, double* lds) {
  if (wide_pcg_gate(a)) return;
  const FvCtx x(a.d);
  double csum[1];
  wide_slot_sum(wide_slots(a, par), a.G, 0, csum, lds);
  const double b00 = -csum[0];
  double b2[1] = {0.0};
  for (int c = g * kWT + threadIdx.x; c < x.n; c += a.G * kWT) {
    const double b = c == 0 ? b00 : x.vec(FV_C)[c];
    x.vec(PCG_R)[c] = b;
    x.vec(FV_Y)[c] = 0.0;
    b2[0] += b * b;
  }
  wide_slot_put(wide_slots(a, par ^ 1), g, 0, b2, lds);
}

// ---- the four GEMMs of z = L+ r: W1 = Qy^T R, W2 = W1 Qx / Lambda, W1 = Qy W2, Z = W1 Qx^T
__host__ __device__ inline FvWideGemm wide_pcg_gemm_of(const FvDesc& d, int which) {
  const int nx = d.nx, ny = d.ny;
  const int64_t n = (int64_t)nx * ny;
  double* w = d.work;
  double *R = w + PCG_R * n, *W1 = w + FV_W1 * n, *W2 = w + FV_W2 * n, *Z = w + PCG_Z * n;
  if (which == 0) return {d.Qy, R, W1, 1, ny, nx, 1, ny, nx, ny};
  if (which == 1) return {W1, d.Qx, W2, nx, 1, nx, 1, ny, nx, nx};
  if (which == 2) return {d.Qy, W2, W1, ny, 1, nx, 1, ny, nx, ny};
  return {W1, d.Qx, Z, nx, 1, 1, nx, ny, nx, nx};
}

// HEAD: the first GEMM of iteration `it` reads the sums of the launch before, decides and writes the scalars (copy
// par ^ 1); the three others read that copy as their `par`.
template <bool HEAD, bool SCALE>
__device__ __forceinline__ void wide_pcg_gemm(const FvWideArgs& a, const FvWidePcg& P, int gb, const FvWideGemm& g, int it,
                                              int par, double* lds) {
  if (wide_pcg_gate(a)) return;
  WidePcgScalars s;
  if (HEAD) {
    if (it == 0) {
      double b2[1];
      wide_slot_sum(wide_slots(a, par), a.G, 0, b2, lds);
      s.bb = b2[0]; s.rr = b2[0]; s.rz = 0.0; s.alpha = 0.0; s.beta = 0.0; s.its = 0;
      s.act = b2[0] != 0.0;
    } else {
      wide_pcg_load(wide_kry(a, par), s);
      if (s.act) {
        double r2[1];
        wide_slot_sum(wide_slots(a, par), a.G, 0, r2, lds);
        s.rr = r2[0]; s.its = it;
      }
    }
    if (s.act && wide_pcg_done(s, P.tol)) s.act = false;
    wide_pcg_store(wide_kry(a, par ^ 1), gb, s);
  } else {
    wide_pcg_load(wide_kry(a, par), s);
  }
  if (!s.act) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int tn = (g.N + 15) >> 4, tiles = ((g.M + 15) >> 4) * tn;
  const int t = gb * kWW + w;
  if (t >= tiles) return;
  fv_gemm_tile<SCALE, false>(g.A, g.sar, g.sak, g.B, g.sbk, g.sbc, g.C, g.M, g.N, g.K, (t / tn) * 16, (t % tn) * 16, lane,
                             a.d.lamx, a.d.lamy, a.d.dy / a.d.dx, a.d.dx / a.d.dy, 0.0);
}

// ---- rz; slot: r . z
__device__ __forceinline__ void wide_pcg_rz(const FvWideArgs& a, int g, int par, double* lds) {
  if (wide_pcg_gate(a)) return;
  const FvCtx x(a.d);
  WidePcgScalars s;
  wide_pcg_load(wide_kry(a, par), s);
  wide_pcg_store(wide_kry(a, par ^ 1), g, s);
  if (!s.act) return;
  double rz[1] = {0.0};
  const double *r = x.vec(PCG_R), *z = x.vec(PCG_Z);
  for (int c = g * kWT + threadIdx.x; c < x.n; c += a.G * kWT) rz[0] += r[c] * z[c];
  wide_slot_put(wide_slots(a, par ^ 1), g, 0, rz, lds);
}

// ---- ap: beta, p = z + beta p_prev (into copy it & 1, from copy (it & 1) ^ 1), q = A p; slot: p . q
__device__ __forceinline__ void wide_pcg_ap(const FvWideArgs& a, int g, int it, int par, double* lds) {
  if (wide_pcg_gate(a)) return;
  const FvCtx x(a.d);
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
    const double y = wide_pcg_row(x, c, i, j, pc, [&](int k) { return PCG_PV(k); });
#undef PCG_PV
    pnew[c] = pc; q[c] = y;
    pq[0] += pc * y;
  }
  wide_slot_put(wide_slots(a, par ^ 1), g, 0, pq, lds);
}

// ---- xr: alpha, x += alpha p, r -= alpha q; slot: |r|^2
__device__ __forceinline__ void wide_pcg_xr(const FvWideArgs& a, int g, int it, int par, double* lds) {
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
  const double *p = x.vec(PCG_P, it & 1), *q = x.vec(PCG_Q);
  double *xs = x.vec(FV_Y), *r = x.vec(PCG_R);
  double r2[1] = {0.0};
  for (int c = g * kWT + threadIdx.x; c < x.n; c += a.G * kWT) {
    xs[c] += alpha * p[c];
    const double rn = r[c] - alpha * q[c];
    r[c] = rn;
    r2[0] += rn * rn;
  }
  wide_slot_put(wide_slots(a, par ^ 1), g, 0, r2, lds);
}

// ---- pfinish (one work-group), after `nb` = min(pressure budget, pmax) iterations
__device__ __forceinline__ void wide_pcg_finish(const FvWideArgs& a, const FvWidePcg& P, int nb, int par, double* lds) {
  if (wide_pcg_gate(a)) return;
  WidePcgScalars s;
  wide_pcg_load(wide_kry(a, par), s);
  if (s.act) {
    double r2[1];
    wide_slot_sum(wide_slots(a, par), a.G, 0, r2, lds);
    s.rr = r2[0]; s.its = nb;
    if (wide_pcg_done(s, P.tol)) s.act = false;
  }
  const bool overflow = s.act && nb < a.pmax;
  if (threadIdx.x == 0) {
    if (overflow) wide_words(a)[WW_OVF] = 2;
    else {
      P.stats[0] += s.its; P.stats[1] += 1; P.stats[2] += s.act ? 1 : 0; P.stats[3] = s.its;
    }
  }
}

// ---- mdot = mdot* - w_f (p'_N - p'_P) on the inner faces, 0.0 on the walls; the vorticity with ghost cells; record sum 8.
__device__ __forceinline__ void wide_pcg_fluxvort(const FvWideArgs& a, int g, double* lds) {
  if (wide_pcg_gate(a)) return;
  const FvCtx x(a.d);
  const double *pp = x.vec(FV_Y), *sx = x.vec(PCG_MS), *sy = x.vec(PCG_MS) + x.ny * x.ldx;
  double part[1] = {0.0};
  for (int c = g * kWT + threadIdx.x; c < x.n; c += a.G * kWT) wide_pcg_cell_fluxvort(x, c, pp, sx, sy, part[0]);
  wide_slot_put(wide_rec_slots(a), g, 8, part, lds);
}
