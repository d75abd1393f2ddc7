// ldc_fv_cu_solve.inc -- what the one-CU kernels with a pressure solve of their own share beside the phases: the four-GEMM
// fast diagonalisation (fv_fastdiag), the conjugate-gradient loop of the consistent pressure equation (fv_pcg, FvPcgRun)
// and the kernel frame (the descriptor fetch, the write-back of the control and statistics words, the host launch loop).
// Included INSIDE the anonymous namespace of its unit, behind ldc_fv_cu_phases.inc and ahead of
// ldc_fv_stretched_phases.inc, by ldc_fv_cu_pressure.hip, ldc_fv_stretched.hip and ldc_fv_stretched_sep.hip.  Each unit
// contributes a policy: its preconditioner, its row of A and, in the separable kernel, three pointwise factors.
// fv_kernel (ldc_fv_kernel.inc) keeps its own frame and fv_pressure_correction: its code object shares a layout with the
// spectral kernels' and is not to move.  The chip chain's CG (ldc_fv_wide_pressure.inc) has launch boundaries where this
// loop has barriers and stays a program of its own.

// this launch's increments of the caller's statistics words (last: the last solve's count)
struct FvPcgRun {
  long long iters, solves, caps, last;
};

// out = Qy ((Qy^T rhs Qx) / Lambda) Qx^T with Lambda = ax lamx_i + ay lamy_j, the zero mode dropped (wide_pcg_gemm_of):
// the exact solve of a separable operator with the eigenpairs (Qx, lamx), (Qy, lamy).  W1 and W2 are its scratch.
// The four table pointers are bound by reference: each is read where its GEMM uses it.  Read up front they stay live
// across the four GEMMs, and the kernels that take them from the descriptor park 7 to 13 more scalar registers in
// vector lanes (profiles/fv_cu_pcg.md).
__device__ __forceinline__ void fv_fastdiag(const FvCtx& x, const double* const& Qx, const double* const& lamx,
                                            const double* const& Qy, const double* const& lamy, double ax, double ay,
                                            const double* rhs, double* out) {
  const int nx = x.nx, ny = x.ny;
  fv_gemm<false>(Qy, 1, ny, rhs, nx, 1, x.vec(FV_W1), ny, nx, ny, nullptr, nullptr, 0, 0);          // W1 = Qy^T rhs
  __syncthreads();
  fv_gemm<true>(x.vec(FV_W1), nx, 1, Qx, nx, 1, x.vec(FV_W2), ny, nx, nx, lamx, lamy, ax, ay);      // W2 = W1 Qx / Lambda
  __syncthreads();
  fv_gemm<false>(Qy, ny, 1, x.vec(FV_W2), nx, 1, x.vec(FV_W1), ny, nx, ny, nullptr, nullptr, 0, 0); // W1 = Qy W2
  __syncthreads();
  fv_gemm<false>(x.vec(FV_W1), nx, 1, Qx, 1, nx, out, ny, nx, nx, nullptr, nullptr, 0, 0);          // out = W1 Qx^T
  __syncthreads();
}

// A x = b by preconditioned conjugate gradients from x = 0 (tests/fv_consistent_numpy.py::FVConsistentState.pcg), the loop
// of the chip chain (ldc_fv_wide_pressure.inc) between barriers: b, |b|^2; then per iteration the stop test, z' = M+ r',
// r'.z', p = z + beta p, q = A p and p.q, x += alpha p, r -= alpha q and |r|^2.  One copy of p: the barrier between its
// update and the product does what the chip chain's two alternating copies do.  b is FV_C with b00 in entry 0; x is FV_Y.
// The policy supplies what differs between the kernels:
//   start(c, b)       what else the start loop writes for cell c (the separable kernel: s and s . b)
//   precondition()    PCG_Z = M+ src(), ending on a barrier (fv_fastdiag)
//   src()             r', the vector the preconditioner reads and r'.z' sums: PCG_R, or s . r
//   z(c)              z_c from z' = PCG_Z: z'_c, or s_c z'_c
//   row(c, i, j, pc, p)   (A p)_c
//   residual(c, rn)   what else is written beside r_c = rn (the separable kernel: s_c rn)
template <class Policy>
__device__ __forceinline__ void fv_pcg(const FvCtx& x, const Policy& pol, const FvCuPcg& P, FvRed& red, double b00,
                                       FvPcgRun& st) {
  const int nx = x.nx, n = x.n, tid = threadIdx.x;
  double bb[1] = {0.0};
  for (int c = tid; c < n; c += kFvThreads) {
    const double b = c == 0 ? b00 : x.vec(FV_C)[c];
    x.vec(PCG_R)[c] = b;
    pol.start(c, b);
    x.vec(FV_Y)[c] = 0.0;
    bb[0] += b * b;
  }
  red.sum(bb);
  double rr = bb[0], rz_prev = 0.0;
  bool act = bb[0] != 0.0;
  int its = 0;
  for (int it = 0; it < P.max_iters && act; ++it) {
    if (sqrt(rr) <= P.tol * sqrt(bb[0])) { act = false; break; }
    pol.precondition();
    double rz[1] = {0.0};
    for (int c = tid; c < n; c += kFvThreads) rz[0] += pol.src()[c] * x.vec(PCG_Z)[c];
    red.sum(rz);
    const double beta = it > 0 ? rz[0] / rz_prev : 0.0;
    rz_prev = rz[0];
    for (int c = tid; c < n; c += kFvThreads) {
      double* p = x.vec(PCG_P);
      const double z = pol.z(c);
      p[c] = it > 0 ? fma(beta, p[c], z) : z;
    }
    __syncthreads();
    double pq[1] = {0.0};
    for (int c = tid; c < n; c += kFvThreads) {
      const double* p = x.vec(PCG_P);
      const double pc = p[c];
      const double y = pol.row(c, c % nx, c / nx, pc, p);
      x.vec(PCG_Q)[c] = y;
      pq[0] += pc * y;
    }
    red.sum(pq);
    const double alpha = rz[0] / pq[0];
    double r2[1] = {0.0};
    for (int c = tid; c < n; c += kFvThreads) {
      double* r = x.vec(PCG_R);
      x.vec(FV_Y)[c] += alpha * x.vec(PCG_P)[c];
      const double rn = r[c] - alpha * x.vec(PCG_Q)[c];
      r[c] = rn;
      pol.residual(c, rn);
      r2[0] += rn * rn;
    }
    red.sum(r2);
    rr = r2[0];
    its = it + 1;
  }
  if (act && sqrt(rr) <= P.tol * sqrt(bb[0])) act = false;      // (converged with the last iteration the cap allows)
  st.iters += its; st.solves += 1; st.caps += act ? 1 : 0; st.last = its;
  __syncthreads();
}

// ---- the kernel frame

// the work-group's descriptor.  The pointer is read straight from the kernarg segment: indexing the by-value array with
// blockIdx.x would make the compiler materialise all LDC_FV_LAUNCH_MAX pointers in registers (fv_kernel does the same)
__device__ __forceinline__ const FvDesc& fv_block_desc() {
  typedef const FvDesc* FvDescPtr;
  return **(const __attribute__((address_space(4))) FvDescPtr*)((kernarg_ptr)__builtin_amdgcn_kernarg_segment_ptr() +
                                                                __builtin_offsetof(FvLaunch, d) + blockIdx.x * sizeof(FvDescPtr));
}

// a block of the descriptor slot behind FvDesc (ldc_fv_common.inc lists them): FvCuPcg, FvGridBlk, FvPrecondBlk
template <class Blk>
__device__ __forceinline__ const Blk& fv_slot_block(const FvDesc& d, int offset) {
  return *reinterpret_cast<const Blk*>(reinterpret_cast<const char*>(&d) + offset);
}

// thread 0, at the end of a launch: the control words ctrl[0 .. 5] (the three counters are this launch's increments)
__device__ __forceinline__ void fv_store_run(const FvDesc& d, const FvRun& run) {
  d.ctrl[0] = run.done; d.ctrl[1] = run.iter; d.ctrl[2] = run.nan_seen ? 1 : 0;
  d.ctrl[3] += run.giveups; d.ctrl[4] += run.lin_iters; d.ctrl[5] += run.solves;
}

// thread 0, at the end of a launch: the caller's four pressure statistics words
__device__ __forceinline__ void fv_store_stats(const FvCuPcg& P, const FvPcgRun& st) {
  P.stats[0] += st.iters; P.stats[1] += st.solves; P.stats[2] += st.caps;
  if (st.solves) P.stats[3] = st.last;
}

// host: the handles hs[0 .. n), LDC_FV_LAUNCH_MAX per launch of `kernel`, one work-group each.  ok(h): the handle is in
// the modes this kernel advances; every handle must belong to the current device.
template <class Ok>
int fv_launch_chunks(void (*kernel)(FvLaunch), ldc_fv* const* hs, int n, int n_iters, void* stream, Ok ok) {
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) return LDC_E_NODEVICE;
  for (int lo = 0; lo < n; lo += LDC_FV_LAUNCH_MAX) {
    FvLaunch L;
    const int b = n - lo < LDC_FV_LAUNCH_MAX ? n - lo : LDC_FV_LAUNCH_MAX;
    for (int q = 0; q < b; ++q) {
      const ldc_fv* h = hs[lo + q];
      if (h->device != dev || !ok(h)) return LDC_E_STATE;
      L.d[q] = h->dev;
    }
    for (int q = b; q < LDC_FV_LAUNCH_MAX; ++q) L.d[q] = nullptr;
    L.n_iters = n_iters;
    hipLaunchKernelGGL(kernel, dim3(b), dim3(kFvThreads), 0, as_stream(stream), L);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  return 0;
}
