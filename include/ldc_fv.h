/* ldc_fv.h -- C ABI of the finite-volume SIMPLE solver in libldc_hip.so (csrc/ldc_fv_kernel.inc, csrc/ldc_fv_post.hip,
 * csrc/ldc_fv_prolong.hip, csrc/ldc_fv_anderson.hip, csrc/ldc_fv_wide.hip with csrc/ldc_fv_wide_anderson.inc and
 * csrc/ldc_fv_wide_pressure.inc and csrc/ldc_fv_wide_stretched.inc and csrc/ldc_fv_wide_separable.inc, csrc/ldc_fv_sample.hip, csrc/ldc_fv_cu_pressure.hip, csrc/ldc_fv_wall_post.hip,
 * csrc/ldc_fv_stretched.hip, csrc/ldc_fv_stretched_sep.hip, csrc/ldc_fv_wall_post_stretched.hip,
 * csrc/ldc_fv_prolong_tables.hip, csrc/ldc_fv_wide_prolong_tables.hip with csrc/ldc_fv_prolong_tables_cells.inc).
 *
 * The reference's other solver (src/solvers/fv/ and src/shared/meshing/): a collocated finite-volume SIMPLE
 * iteration on a uniform nx x ny Cartesian grid of the lid-driven cavity.  One work-group advances one trial for a
 * whole chunk of iterations; a launch of B trials is B independent work-groups (no inter-group waits).
 *
 * Conventions (all arrays are device memory owned by the caller, doubles unless stated):
 *  - cells  c = j*nx + i  (y outer, x inner; simple_structured.py:197-200), n = nx*ny;
 *  - face fluxes  mdot = [ fx | fy ]:  fx[j*(nx+1) + i], i = 0..nx, the flux in +x through the face at x = i*dx;
 *    fy[j*nx + i], j = 0..ny, the flux in +y through the face at y = j*dy  (length LDC_FV_FACES(nx, ny));
 *  - Qx (nx x nx, row-major, column k = k-th eigenvector) and lamx (nx): numpy.linalg.eigh of the 1-D Neumann
 *    second difference (diagonal 1, 2, ..., 2, 1; off-diagonals -1), eigenvalues ascending, so the zero mode is
 *    index 0; Qy, lamy likewise for ny.  The pressure correction is solved with them exactly (fast diagonalisation).
 *  - rec: rec_cap rows of LDC_FV_REC_LEN doubles, row k = iteration k of the last enqueue:
 *    rel_change, |u'|, |v'|, |div mdot|, E, Z, P, 0   (the record of include/ldc_hip.h with DT = 0);
 *  - ctrl: LDC_FV_CTRL_LEN int64: [0] converged latch, [1] iterations done, [2] NaN seen (the trial stopped),
 *    [3] momentum solves that hit max_lin_iters (accepted, as the reference does), [4] BiCGSTAB iterations of all
 *    momentum solves, [5] momentum solves.  Zero ALL of it to start a solve, before the first enqueue and again
 *    before every later solve on the same handle: the kernel counts on from ctrl[1], tests the latch only once
 *    ctrl[1] >= warmup and adds to [3..5], so words left from a finished solve would skip the warm-up and report
 *    running totals.  The state (u, v, p, mdot) is not touched by that: a new solve continues from the fields.
 *    Between the enqueues of ONE solve leave ctrl alone.
 *  - functions return 0, a negative LDC_E_* code of ldc_hip.h, LDC_FV_E_NAN, or a positive hipError_t.
 *
 * Post-processing (version 2, csrc/ldc_fv_post.hip): the vorticity, the streamfunction and the vortex extrema of a
 * trial that is NOT in flight, one work-group per trial, as the solver's host code computes them (base.py:569-760):
 *  - omega (ny x nx) by ghost cells from u and v: -f at the walls, 2 lid_velocity - u at the lid;
 *  - psi (ny x nx): the 5-point Dirichlet problem (cx Tx + cy Ty) psi = omega on the (nx-2) x (ny-2) interior cells,
 *    T = tridiag(-1, 2, -1), cx = 1/dx^2, cy = 1/dy^2, solved exactly with the sine vectors
 *    S_m[k][j] = sqrt(2/(m+1)) sin(pi (k+1)(j+1)/(m+1)), lam_m[k] = 2 - 2 cos(pi (k+1)/(m+1)), m = nx-2 and ny-2
 *    (S row-major m x m; symmetric); the boundary ring of psi is exactly 0.0;
 *  - the extrema are (value, cell) pairs, ties to the LOWEST cell c = j*nx + i (numpy.argmin / argmax); the three
 *    corner regions are BR: i >= ix_gt and j < jy_lt, BL: i < ix_lt and j < jy_lt, TL: i < ix_lt and j >= jy_gt.
 *    The caller derives the four bounds from its own cell-centre coordinates (x < 0.5: i < ix_lt; x > 0.5:
 *    i >= ix_gt; likewise y), so the kernel compares no coordinates;
 *  - result: LDC_FV_POST_RESULT_LEN doubles, the LDC_FV_POST_* slots below; cells are stored as doubles, -1 = none;
 *  - scratch: two of the trial's work vectors and 72 bytes of the descriptor slot behind the descriptor.  The state,
 *    rec and ctrl are only read, so a solve goes on afterwards as if nothing had happened.
 *
 * Prolongation (csrc/ldc_fv_prolong.hip): the state of a FINE trial from the state of a COARSE one on the same domain,
 * of any two sizes (coarse-to-fine sequencing, continuation in Re at equal size), one work-group per pair, neither
 * trial in flight.  Read: the coarse trial's u, v, p, ulid and sizes.  Written: the fine trial's u, v, p, mdot and
 * nothing else (no ctrl, no rec, no work vector), so the caller zeroes ctrl as before any new solve.
 *  - per axis the coarse field is extended by a ring on the domain boundary: nodes e_0 = 0, e_k = (k - 1/2) h_c
 *    (k = 1..n_c, the cell centres), e_{n_c+1} = n_c h_c.  u and v on the ring are 0.0, except u above cell i on the
 *    lid (the y ring, j = ny_c + 1), which is the coarse ulid[i]; the four corners are 0.0.  The ring of p repeats
 *    the nearest cell (zero normal gradient);
 *  - a fine centre x = (i + 1/2) h_f takes the left node k = the largest node with e_k <= x, at most n_c, and the
 *    weight t = (x - e_k) / (e_{k+1} - e_k); the value is bilinear, x first: lo = a + tx (b - a) on row ky,
 *    hi likewise on row ky + 1, then lo + ty (hi - lo).  No multiply-add is contracted;
 *  - p: the interpolated value at fine cell 0 is subtracted from every cell, so p[0] is exactly 0.0 (the pinned cell);
 *  - mdot from the new u, v as the solver's face rule: interior faces rho (1/2 f_N + 1/2 f_P) |S|, the faces on the
 *    four walls exactly 0.0.
 *
 * Anderson acceleration (csrc/ldc_fv_anderson.hip, ldc_fv_anderson_enqueue): the outer iteration as the fixed-point map
 * x -> g = SIMPLE(x) on the concatenation [u | v | p | mdot] (L = 3n + faces entries), mixed after every iteration by a
 * kernel of its own, one work-group of 512 threads per trial; the solve kernel is not touched.  Per trial and iteration,
 * with it = ctrl[1] after the SIMPLE launch:
 *  - it equals astate[2] (the trial was latched, NaN or capped: the launch did nothing): nothing happens;
 *  - otherwise rec row 0 (where a launch of one iteration writes) is copied to rec row j, the iteration's place in the
 *    enqueue; the row of iteration 0 waits in the last LDC_FV_REC_LEN doubles of the descriptor slot in the tail of
 *    `work` and goes back to row 0 with the trial's last iteration of the enqueue (the last one, or the one that set
 *    ctrl[0] or ctrl[2]), so rec reads as after ldc_fv_batch_enqueue.  With ctrl[0] or ctrl[2] set, or depth 0, that
 *    is all;
 *  - x is the state the SIMPLE launch started from, which the kernel keeps in hist.  After a zeroed astate it has none:
 *    the first iteration of a solve only keeps g as the next x.  From the second on f = g - x, and from the third on
 *    the differences dG = g - g_prev, dF = f - f_prev replace the oldest of `depth` columns (a ring; slot astate[1]);
 *  - it < start, or no column yet: the next state is g.  Otherwise, over the m valid columns in SLOT order, A = dF^T dF
 *    and b = dF^T f over the u, v, p entries (the first 3n), A += 1e-12 trace(A) / m on the diagonal, A gamma = b by
 *    Cholesky (one thread), and the next state is g - sum_i gamma_i dG_i over all L entries.  The weights of the g's sum
 *    to 1, so the mixed mdot is a combination of mass-conserving fluxes and p[0] stays 0; it is WRITTEN as 0.0;
 *  - a pivot <= 0 (or NaN) or a gamma that is not finite: the fallback.  The next state is g, the ring is emptied
 *    (g_prev and f_prev stay) and astate[3] counts it;
 *  - hist: x, g_prev, f_prev, dG[depth], dF[depth], L doubles each: (2 depth + 3) L.  The Gram matrix is recomputed in
 *    full every iteration, sums in a fixed order (per thread in increasing index, wave shuffles, LDS), so lone runs,
 *    batches and repeats agree bit for bit.
 *  Between the enqueues of ONE solve an accelerated trial is advanced by ldc_fv_anderson_enqueue only.
 *
 * A lone trial on the whole chip (csrc/ldc_fv_wide.hip, ldc_fv_wide_*): the same iteration on the same arrays, with the
 * same meaning of u, v, p, mdot, work, rec and ctrl, for LDC_FV_MIN_N .. LDC_FV_WIDE_MAX_N cells per axis.  One kernel
 * launch per phase of the iteration, up to 256 work-groups each; the launch boundary is the only barrier, so no
 * work-group waits for another.  The work vectors keep the layout of the one-CU kernel: after one iteration `work`
 * holds the intermediates of ldc_fv_step_debug (vector k at work + k n, in the order grad p x / y, aP aW aE aS aN, u*,
 * v*, ..., rhs_p at 23 with entry 0 = 0, p' + const at 26, u' and v' at 27 and 28, b_u and b_v at 30 and 31).
 *  - sums: every work-group leaves its partial in a slot of `scratch`, the next launch adds the slots in a fixed
 *    order, so runs repeat bit for bit (the order differs from the one-CU kernel's: the two agree to rounding);
 *  - an enqueue carries lin_budget BiCGSTAB iterations per SIMPLE iteration (min(lin_budget, max_lin_iters) times five
 *    launches).  A momentum solve still active after lin_budget < max_lin_iters iterations sets the overflow word
 *    before u, v, p or mdot are touched: ctrl stays as it was, the rest of the enqueue does nothing, ldc_fv_wide_status
 *    returns LDC_FV_WIDE_E_BUDGET and the caller enqueues the remaining iterations again with a larger budget (every
 *    enqueue clears the word).  With lin_budget >= max_lin_iters a solve still active is the accepted give-up of
 *    ctrl[3].  So the result does not depend on the budget;
 *  - scratch: LDC_FV_WIDE_SCRATCH_LEN doubles owned by the caller, the library's between two enqueues of one solve too.
 *
 * Several such trials in the same launches (ldc_fv_wide_batch_*): a batch object over 1 .. LDC_FV_WIDE_BATCH_MAX
 * ldc_fv_wide handles of any sizes and parameters (one max_lin_iters, one device).  Every phase is then ONE launch that
 * carries the work-groups of all trials -- the sum of LDC_FV_WIDE_GROUPS for a cell sweep, the sum of
 * LDC_FV_WIDE_GEMM_GROUPS for a GEMM, one per trial for begin, linfinish and record -- and a work-group finds its trial
 * and its index within it in a table in a device buffer of the caller's (LDC_FV_WIDE_BATCH_TABLE_LEN bytes, written once
 * by create).  Per trial nothing changes: the same kernels' bodies, the same G, slots and order of every sum, so a trial's
 * u, v, p, mdot, rec and ctrl are bit-identical to those of ldc_fv_wide_enqueue on its own handle.
 *  - an enqueue hands every trial its own number of iterations (its quota, 0 .. its rec_cap; a scratch word that
 *    `begin` writes) and runs max(quota) iteration chains; a trial stops at its quota, its latch, a NaN or its overflow,
 *    and the launches after that cost it empty work-groups.  A trial with quota 0 is not touched at all;
 *  - overflow and NaN are per trial: ldc_fv_wide_status of the trial's own handle.  The caller enqueues the trials that
 *    overflowed again with a larger budget and quota 0 for everyone else;
 *  - the table is never rebuilt: finished trials stay in the batch object.
 *
 * Anderson acceleration of such a trial (ldc_fv_wide_set_anderson; csrc/ldc_fv_wide_anderson.inc, part of the same unit):
 * the algorithm above, word for word -- the same map, hist, A and b over the first 3n entries with the columns in slot
 * order, lambda, Cholesky by one thread, x_next over all L entries with p[0] written as 0.0, the same fallback and the same
 * four astate words -- by the chip mapping's rules.  A handle with a mixing block attached ends every iteration on three
 * more launches behind `record` (LDC_FV_WIDE_ANDERSON_LAUNCHES), part of the captured iteration like the others:
 *  - push (LDC_FV_WIDE_GROUPS work-groups, grid-stride over the entries): f, the new columns dG and dF, g_prev and f_prev
 *    (an iteration that is not mixed keeps g as the next x here); then the work-group's partial sums of b and of the lower
 *    triangle of A into its own slot of the mixing scratch;
 *  - mix (the same grid): every work-group adds the slots in one fixed order (thread t takes slot t), solves the m x m
 *    system itself -- the same numbers by the same instructions everywhere -- and mixes its entries; work-group 0 leaves
 *    the fell flag in the scratch;
 *  - close (one work-group): astate.
 *  - the gate: every one of the three returns at once when ctrl[1] == astate[2], that is when `record` has counted no
 *    iteration since the last close: the trial latched or met a NaN earlier, the iteration overflowed (it changed nothing
 *    and is enqueued again), the quota is done, or it is 0.  The quota word is NOT read: the last iteration of a quota is
 *    mixed like any other, so a solve does not depend on where its enqueues end.  With ctrl[0] or ctrl[2] set by this
 *    iteration only astate[2] moves.  push and mix write neither ctrl nor astate; close, one work-group per trial, is
 *    the only launch that writes astate.  The record rows are in place already: nothing is moved;
 *  - mixing scratch: LDC_FV_WIDE_ANDERSON_SCRATCH_LEN doubles owned by the caller, the library's between two enqueues of
 *    one solve: 8 int64 words (word 0: the last mix took the fallback), then one slot per work-group of
 *    depth (depth + 3) / 2 doubles: b[depth], then the lower triangle of A by rows.  hist takes (2 depth + 3) L doubles
 *    (LDC_FV_ANDERSON_HIST_LEN): 0.55 GB at 1024 x 1024 with depth 5, 1.5 GB with depth 16;
 *  - in a batch the block travels in the trial's table entry (ldc_fv_wide_batch_create copies it: attach first), the
 *    three launches carry the work-groups of all trials, and a trial without a block returns from them before it reads
 *    anything: it is bit-identical to its plain run.  A batch without any block runs the plain chain, launch for launch.
 *  Sums run in a fixed order (per thread in increasing index, wave shuffles, the waves in order from LDS, the slots by
 *  thread), so lone runs, batches, graphs and repeats agree bit for bit, whatever the budget and the enqueues' lengths.
 *  The order differs from the one-CU mixing kernel's: the two agree to rounding.
 *
 * The consistent pressure equation of such a trial (ldc_fv_wide_set_pressure; csrc/ldc_fv_wide_pressure.inc, part of the
 * same unit).  The reference corrects the pressure with the constant-coefficient Laplacian rho |S| / d and the velocities
 * with u' = -D grad p', D = V / a_P: two operators, so the corrected face fluxes never conserve mass.  A handle in mode
 * LDC_FV_PRESSURE_CONSISTENT solves, per SIMPLE iteration,
 *    (A x)_P = sum over the inner faces f of P of w_f (x_P - x_N) = b,  w_f = rho (D_P / 2 + D_N / 2) |S_f| / d_f,
 * D_c = V / (a_P + 1e-14) from the unrelaxed diagonal, |S| / d = dy / dx on x faces and dx / dy on y faces, b = rhs_p with
 * entry 0 replaced by minus the sum of the others, by conjugate gradients from x = 0 with the preconditioner z = L+ r (the
 * four GEMMs of the fast diagonalisation, zero mode dropped, no entry-0 insertion, no shift).  It stops at
 * |r|_2 <= tol |b|_2; after max_iters iterations the iterate is accepted and the cap hit counted; |b| = 0 gives x = 0 without
 * an iteration.  p' = x - x_0, u' = -D grad p' and p += alpha_p p' as before; the inner faces take
 * mdot = mdot* - w_f (p'_N - p'_P) and the wall faces stay exactly 0.0 (DESIGN.md FV-Q4 does not apply in this mode).
 *  - the chain: faces | init | np x (gemm x 4 | rz | ap | xr) | pfinish stand where faces | gemm x 4 stood, and a fluxvort
 *    of the mode where fluxvort stood: 9 + 5 nb + 7 np launches per iteration (ldc_fv_wide_launches), np = min(pressure
 *    budget, max_iters), by the chip mapping's rules -- grids of (nx, ny) alone, partial sums through the slots of the solve's
 *    scratch in the one fixed order, the CG scalars in two copies that alternate by launch (where the BiCGSTAB scalars
 *    lived), the search direction in two alternating copies because its update is fused with the matrix-vector product,
 *    no waits, no atomics.  The CG vectors and mdot* live in BiCGSTAB's work vectors 9 .. 16, dead after linfinish; x is
 *    vector 26, where p' + const stands in the reference mode too;
 *  - the budget (ldc_fv_wide_set_pressure_budget, LDC_FV_WIDE_PRESSURE_BUDGET_DEFAULT) follows the protocol of lin_budget: a
 *    solve still active after np < max_iters iterations sets the overflow word -- to 2, where BiCGSTAB's overflow writes 1 --
 *    before u, v, p or mdot are touched (mdot* waits in work vectors), ctrl stays, ldc_fv_wide_status returns
 *    LDC_FV_WIDE_E_BUDGET and the caller enqueues again with a larger budget.  Results do not depend on either budget; the
 *    captured graphs are keyed on both;
 *  - statistics: LDC_FV_WIDE_PRESSURE_SCRATCH_LEN int64 words of the caller's, written by pfinish for every completed
 *    iteration: [0] CG iterations in all, [1] solves, [2] cap hits, [3] the last solve's count.  Zero them with ctrl;
 *  - in a batch the block (tolerance, statistics pointer: 16 bytes) travels in the trial's table entry behind the mixing
 *    block -- FvWideArgs 208 bytes with max_iters in its last four, the mixing block 32, this one 16: the entry's 256 bytes
 *    are full -- so ldc_fv_wide_set_pressure comes before ldc_fv_wide_batch_create.  A batch may mix both modes (one
 *    max_iters among the consistent trials): its chain then carries the launches of both, 13 + 5 nb + 7 np, a reference
 *    trial returns from the new ones before it reads anything and is bit-identical to its plain run, and a consistent trial
 *    returns from the exact solve's GEMMs.  A batch without a consistent trial runs the plain chain, launch for launch.
 *  The mixing chain of ldc_fv_wide_set_anderson follows `record` as before.
 *
 * The consistent pressure equation of a one-CU trial (ldc_fv_set_pressure; csrc/ldc_fv_cu_pressure.hip, a unit of its own so
 * that the code object of the reference kernel stays what it was).  The same equation, operator, right-hand side,
 * preconditioner, stop rule, cap, p' = x - x_0 and face correction as above, for an ldc_fv handle: one work-group of 512
 * threads advances the trial for the whole chunk, as the reference kernel does, and ldc_fv_enqueue / ldc_fv_batch_enqueue
 * send each handle to the kernel of its mode (a list of both modes is two launch groups; ldc_fv_anderson_enqueue reaches the
 * solve through ldc_fv_batch_enqueue, so the mixing kernel follows either).
 *  - the CG loop runs inside the work-group, between barriers where the chip chain has launch boundaries: b and |b|^2; per
 *    iteration the stop test, the four GEMMs of z = L+ r, r.z, p = z + beta p (one copy of p: the barrier does what the two
 *    alternating copies do), q = A p and p.q, x += alpha p, r -= alpha q and |r|^2.  There is no budget and no overflow: the
 *    loop ends inside the kernel, as BiCGSTAB does on this mapping;
 *  - every stop decision is taken from totals that every thread holds identically, every loop is bounded (a NaN runs to
 *    max_iters and the record's NaN then stops the trial, ctrl[2]), and the sums run in one fixed order (per thread in
 *    increasing cell, wave shuffles, the waves in order from LDS; no atomics): lone runs, batches and repeats agree bit
 *    for bit, whatever the chunks.  The order differs from the chip chain's: the two agree to rounding;
 *  - the work vectors are the chip chain's (mdot* in 9 .. 11, r 12, z 13, p 14, q 16, x 26): after one iteration `work`
 *    reads as after a chip iteration, rhs_p at 23 with entry 0 = 0 and x at 26;
 *  - statistics: LDC_FV_PRESSURE_STATS_LEN int64 words of the caller's, to which thread 0 adds the launch's increments
 *    when it writes ctrl back: [0] CG iterations in all, [1] solves, [2] cap hits, [3] the last solve's count.  Zero them
 *    with ctrl;
 *  - the block (tolerance, cap, mode, statistics pointer: 24 bytes) lives at byte 384 of the descriptor slot in the tail of
 *    `work`, clear of the descriptor (< 256), the post block (256 .. 327) and the mixing kernel's kept row (448 .. 511);
 *  - ldc_fv_step_debug on such a handle returns LDC_E_ARG: the debug kernel is the reference iteration.  The work vectors
 *    hold the intermediates.  ldc_fv_post_enqueue and ldc_fv_prolong_enqueue take the handle as any other.
 *
 * Stretched grids of a one-CU trial (ldc_fv_set_grid; csrc/ldc_fv_stretched.hip, a unit of its own so that the code objects
 * of the kernels above stay what they were).  A handle with geometry tables attached runs the same iteration on a tensor
 * grid with any spacing per axis (the solver builds tanh-clustered vertices, cell centres at their midpoints), with the
 * reference's own rules on such a mesh (tests/fv_stretched_numpy.py states them array by array), by either pressure
 * equation (ldc_fv_set_pressure), one work-group of 512 threads per trial as before.  ldc_fv_enqueue / ldc_fv_batch_enqueue
 * send such handles to fv_stretched_kernel, one launch group per pressure mode, so a list may mix uniform and stretched
 * trials of any sizes.
 *  - per axis ONE table of LDC_FV_GRID_TABLE_LEN(n) = 3 n + 2 doubles, [h | d | g]: h[i], i = 0 .. n-1, the cell widths; then
 *    per face k = 0 .. n (face k lies between cells k-1 and k) d[k], the distance between the two centres, h[0] / 2 and
 *    h[n-1] / 2 on the walls, and g[k] = (face - centre of cell k-1) / d[k], the weight of cell k in
 *    phi_f = g phi_N + (1 - g) phi_P (the walls' g is not read).  V = hx[i] hy[j]; |S| = hy[j] on x faces, hx[i] on y faces;
 *  - the gradient is the mean of the one-sided slopes (f_N - f_P) / d a cell has, with the pinned-cell exclusions; inner
 *    diffusion mu |S| / d, wall diffusion mu |S| / (h / 2); u*, v*, grad p, D = V / (a_P + 1e-14) and u', v' go to the
 *    faces with g; `ulid` is the caller's lid profile at the stretched face centres; dx, dy of the problem are not read;
 *  - reference mode: the operator with the weights rho |S| / d is Hy (x) Kx + Ky (x) Hx, so Qx, lamx (Qy, lamy) are the
 *    generalised eigenpairs Kx q = lam Hx q with Q^T Hx Q = I (Kx: the 1-D Neumann stiffness with the weights rho / d,
 *    Hx = diag(h); ascending, index 0 the zero mode), and the exact solve is the same four GEMMs with the divisor
 *    lamy[a] + lamx[b]; the c_0 and y - y_0 rules and FV-Q4 (wall faces of mdot') are kept;
 *  - consistent mode: w_f = rho (g D_N + (1 - g) D_P) |S| / d, CG preconditioned by the operator above, the loop, the stop
 *    rule, the work vectors and the statistics words of ldc_fv_cu_pressure.hip; walls exactly 0.0;
 *  - omega, E, Z, P: d f / dx at a cell is (f_e - f_w) / hx[i] with g-weighted face values and the wall's own value on a
 *    wall face (0; ulid[i] for u on the lid; 0 for omega); the sums carry the weight V.  With equal widths and a constant lid
 *    this is algebraically the ghost-cell rule above;
 *  - the block (two pointers) lives at byte 328 of the descriptor slot, clear of the post block (256 .. 327) and the pressure
 *    block (384 .. 407); the descriptor itself does not change;
 *  - ldc_fv_step_debug on such a handle returns LDC_E_ARG.  ldc_fv_post_enqueue, ldc_fv_prolong_enqueue, ldc_fv_wall_post_enqueue,
 *    the sampling and the mixing kernel's callers assume equal spacing: the solver refuses those combinations.  The wall rule
 *    of such a trial is ldc_fv_wall_stretched_post_enqueue, its coarse-to-fine transfer ldc_fv_prolong_tables_enqueue (both
 *    below).
 *
 * The separable scaled preconditioner of such a trial (ldc_fv_set_preconditioner; csrc/ldc_fv_stretched_sep.hip, a unit of
 * its own so that fv_stretched_kernel stays what it was).  In consistent mode the CG above is preconditioned by the operator
 * with D left out; on a stretched mesh D = V / a_P varies with V, and the count per solve grows several times.  A handle with
 * preconditioner tables attached runs the same iteration with another z in the CG loop, and nothing else changed: the
 * operator, b, the start x = 0, the stop rule and the cap, the statistics words, p', the face correction, walls exactly 0.0.
 *  - the caller fits D by a product a[i] b[j] on the host (the solver: a least-squares fit of log G, G = V / a_P of pure
 *    diffusion with mu left out) and builds L_s = My (x) Kx^a + Ky^b (x) Mx: Kx^a the 1-D Neumann stiffness with the weights
 *    rho a_f / d, a_f[k] = g[k] a[k] + (1 - g[k]) a[k-1] on the inner faces, Mx = diag(hx a); y likewise with b;
 *  - per axis ONE table of LDC_FV_PRECOND_TABLE_LEN(n) = n (n + 2) doubles, [a (n) | lam (n) | Q (n x n, row-major, column k
 *    the k-th vector)]: the generalised eigenpairs Kx^a q = lam Mx q with Q^T Mx Q = I, ascending, index 0 the zero mode;
 *  - L_s+ R = Qy ((Qy^T R Qx) / (lamy[a] + lamx[b])) Qx^T with entry (0, 0) set to 0: the four GEMMs of the exact solve with
 *    these tables; per solve s_c = sqrt(a[i] b[j] / D_c), D_c = V / (a_P + 1e-14), and z = s . L_s+ (s . r).  z . r > 0 for
 *    every r != 0 of zero sum, so CG is defined on the range of A; a constant in z is harmless, p' = x - x_0;
 *  - s and s . r live in the work vectors 15 and 17, which are dead during the pressure solve; the loop has the sweeps and
 *    barriers of the other, LDC_FV_NWORK is unchanged;
 *  - the block (two pointers) lives at byte 344 of the descriptor slot, behind the grid block; the descriptor itself does
 *    not change.  ldc_fv_enqueue / ldc_fv_batch_enqueue send consistent handles with both kinds of tables to
 *    fv_stretched_sep_kernel as one more launch group, in list order within it.  A handle in reference mode keeps the
 *    setting and does not read the block.
 *
 * Stretched grids of a chip trial (ldc_fv_wide_set_grid; csrc/ldc_fv_wide_stretched.inc, inside the wide unit).  A LONE
 * ldc_fv_wide handle with geometry tables attached runs the iteration described under "Stretched grids of a one-CU trial" --
 * the same tables [h | d | g], the same rules, either pressure equation, Qx, lamx, Qy, lamy the generalised eigenpairs, ulid at
 * the stretched face centres, dx and dy not read -- as the launch-per-phase chain above, LDC_FV_MIN_N .. LDC_FV_WIDE_MAX_N
 * cells per axis.
 *  - the phases that read the geometry (assemble, faces, correct, fluxvort, sums; consistent mode: its faces, ap and
 *    fluxvort) are twins that take the two table pointers by value beside the trial's arguments; their cell bodies are those
 *    of the one-CU stretched kernels (csrc/ldc_fv_stretched_cells.inc: one definition for both mappings).  The BiCGSTAB
 *    sweeps, linfinish, init, rz, xr, pfinish and the GEMMs are the uniform chain's kernels; the scaled GEMM and `record` are
 *    launched with dx = dy = 1 in their copy of the arguments (the divisor is lamy[a] + lamx[b], and the sums of E, Z, P carry
 *    each cell's volume already);
 *  - the chain has the uniform chain's launches one for one, in the same grids: ldc_fv_wide_launches, the scratch, both
 *    budgets and their overflow protocol, the statistics words and the graphs are unchanged, and the chip mapping's rules
 *    hold (grids of (nx, ny) alone, slots added in one fixed order, `par` alternating, every kernel behind the gate, no
 *    work-group reading what another of the same launch writes: ap recomputes p at the neighbours as before);
 *  - the sums go through the slots in the chip mapping's order, not the one-CU kernel's: the two agree to rounding;
 *  - not for such a handle, each LDC_E_ARG before any device call: Anderson mixing (ldc_fv_wide_set_anderson, in either
 *    order), a batch (ldc_fv_wide_batch_create: the 256-byte table entry is full, and a stretched trial must never run the
 *    uniform kernels unnoticed), ldc_fv_wide_post_enqueue and ldc_fv_wide_prolong_enqueue (equal spacing).  The wall rule of
 *    such a trial is ldc_fv_wall_stretched_post_enqueue, its coarse-to-fine transfer ldc_fv_wide_prolong_tables_enqueue (below);
 *    both take raw pointers and every size.
 *
 * The separable scaled preconditioner of a chip trial (ldc_fv_wide_set_preconditioner; csrc/ldc_fv_wide_separable.inc, inside
 * the wide unit).  A lone ldc_fv_wide handle with geometry tables takes the tables of "The separable scaled preconditioner"
 * above -- the same struct, per axis [a | lam | Q] of LDC_FV_PRECOND_TABLE_LEN(n) doubles, LDC_FV_MIN_N .. LDC_FV_WIDE_MAX_N
 * cells per axis -- and its consistent chain then preconditions the CG by z = s . L_s+ (s . r), s_c = sqrt(a[i] b[j] / D_c):
 * the same operator, b, start x = 0, stop rule on |r|, cap, budget protocol, statistics words, p' and face correction, so
 * the result differs from the laplacian run's at the level of the pressure tolerance.
 *  - the chain is launch for launch the stretched consistent one, in the same grids, with the same `par`, slots and scratch:
 *      faces | init* | np x (gemm x 4* | rz* | ap* | xr*) | pfinish.
 *    init* also writes s and s . b, xr* also s . r (work vectors 18 and 19, dead after linfinish; vector 15 of the one-CU
 *    kernel is the second copy of p here); the GEMMs are the chain's own kernels on a copy of the arguments whose descriptor
 *    carries Qx, lamx, Qy, lamy of these tables and dx = dy = 1, the first one reading s . r; rz* sums (s . r) . z'; ap* is
 *    the stretched ap with s . z' for z at the cell and at its four neighbours.  The scaling factor has one definition for
 *    both mappings (csrc/ldc_fv_stretched_cells.inc).  ldc_fv_wide_launches is unchanged;
 *  - the block (two pointers and the mode) stands at the end of the handle, behind the grid block, and travels by value in
 *    the kernel arguments: nothing is copied.  The mode is kept in either pressure mode and read only in consistent mode; a
 *    handle without the block enqueues exactly the launches of before;
 *  - ldc_fv_wide_set_grid resets it to LDC_FV_PRECOND_LAPLACIAN whenever it attaches or detaches geometry tables: the tables
 *    belong to the mesh they were fitted to.
 *
 * Post-processing and prolongation of such a trial (ldc_fv_wide_post_enqueue, ldc_fv_wide_prolong_enqueue; the same
 * unit): what ldc_fv_post_enqueue and ldc_fv_prolong_enqueue do for a trial of up to LDC_FV_MAX_N cells per axis, by the
 * chip mapping's rules for LDC_FV_MIN_N .. LDC_FV_WIDE_MAX_N: one launch per phase, a grid that depends on (nx, ny) alone,
 * the launch boundary the only barrier, no work-group reading what another of the same launch writes.
 *  - post: omega | W1 = Sy^T F | W2 = W1 Sx / Lambda | W1 = Sy W2 | psi = W1 Sx^T | extrema | result, seven launches
 *    (ldc_fv_wide_post_launches).  The cell sweeps take LDC_FV_WIDE_GROUPS work-groups, a GEMM
 *    LDC_FV_WIDE_GEMM_GROUPS(nx - 2, ny - 2); every work-group leaves its five (key, cell) candidates and its not-finite
 *    flags in a slot of the caller's scratch (LDC_FV_WIDE_POST_SCRATCH_LEN doubles) and `result`, one work-group, merges
 *    them by (larger key, then lower cell), which does not depend on the grouping.  The arithmetic, the operands and the
 *    order of every sum are those of ldc_fv_post_enqueue: psi, omega and the result block are its bits.  Read: u, v, the
 *    sizes.  Written: psi, omega, result, work vectors 24 and 25, the scratch; not ctrl, rec, the state or the scratch of
 *    the solve;
 *  - prolong: a launch for u, v, p at the fine cells (every thread recomputes the interpolated p at fine cell 0, so
 *    p[0] is exactly 0.0) and one for mdot, LDC_FV_WIDE_GROUPS of the fine trial each; the arithmetic of
 *    ldc_fv_prolong_enqueue with no multiply-add contracted, so the fine u, v, p, mdot are its bits.  It is the transfer of
 *    two EQUALLY SPACED chip trials; a chip trial on either grid is also served by ldc_fv_wide_prolong_tables_enqueue (below),
 *    which reads both grids from tables.
 *
 * Sampling at the nodes of a tensor grid (csrc/ldc_fv_sample.hip, ldc_fv_sample_nodes): the initial guess of a spectral
 * trial from a finite-volume state of the same cavity.  A job holds raw device pointers only, no handle, so a trial of any
 * mapping can be the source, LDC_FV_MIN_N .. LDC_FV_WIDE_MAX_N cells per axis; nothing of the source is written.
 *  - interior nodes (0 < ix < Mx - 1 and 0 < iy < My - 1) take the bilinear interpolant of the ring-extended field of the
 *    prolongation above at (x[ix], y[iy]): the same nodes e_k, the same left node and weight, x first, no multiply-add
 *    contracted.  U and V take the ring of walls and lid (the SOURCE's ulid above the cells), P the zero-gradient ring,
 *    and P is not shifted: only grad p enters the spectral residual;
 *  - boundary nodes take the TARGET's own values, bit for bit: U = V = 0.0 on ix = 0, ix = Mx - 1 and iy = 0; V = 0.0 and
 *    U = ulid_nodes[ix] on iy = My - 1, the two top corners included;
 *  - U and V are dense Mx x My, element (ix, iy) at ix My + iy; P is dense (Mx - 2) x (My - 2) over the inner nodes,
 *    element (ix, iy) at (ix - 1)(My - 2) + (iy - 1);
 *  - blockIdx.y is the job and the work-groups of a job stride over its nodes: no waits, no atomics, no LDS, so a job's
 *    result does not depend on what else is in the call, bit for bit.
 *
 * Wall-anchored streamfunction and sub-cell vortex centres (csrc/ldc_fv_wall_post.hip, ldc_fv_wall_post_enqueue): a second
 * post-processing rule beside the reference's above, whose psi = 0 at the CENTRES of the boundary ring is an O(h) error
 * under the lid and whose centres are cell centres.  A job holds raw device pointers only, no handle, so a trial of any
 * mapping is served, LDC_FV_MIN_N .. LDC_FV_WIDE_MAX_N cells per axis; the state is only read.
 *  - omega (ny x nx): as above, but the ghost above the top row is 2 ulid[i] - u, the lid PROFILE, not the scalar
 *    lid_velocity (second order for the smoothed lids too).  Nothing writes psi in this phase;
 *  - psi (ny x nx): (cx Tx + cy Ty) psi = omega on ALL nx x ny cells, T_n = tridiag(-1, 2, -1) with T[0][0] = T[n-1][n-1] = 3
 *    (the ghost is -psi: psi = 0 on the wall face), cx = 1/dx^2, cy = 1/dy^2, solved exactly with T_n = C Lam C^T,
 *    lam[k] = 2 - 2 cos(pi (k+1)/n), C[j][k] = sqrt(2/n) sin(pi (k+1)(j+1/2)/n) for k = 0 .. n-1 with the last column
 *    (k = n-1) divided by sqrt(2) (C row-major n x n, column k the k-th vector; NOT symmetric):
 *    psi = Cy ((Cy^T Omega Cx) / (cy lamy[a] + cx lamx[b])) Cx^T, four GEMMs, the second with the division in its epilogue;
 *  - the extrema: the five candidates, the four index bounds and the tie rule (lowest cell) of ldc_fv_post_enqueue;
 *  - result: LDC_FV_WALL_RESULT_LEN doubles.  Slots 0 .. 15 are the LDC_FV_POST_* slots.  Then four groups of
 *    LDC_FV_WALL_GROUP_LEN doubles for the primary minimum, BR, BL and TL: x, y, psi, omega, status, sx, sy, 0
 *    (LDC_FV_WALL_X ..).  With refine = 0 a group carries the cell's own values (x = (i + 1/2) dx, y = (j + 1/2) dy) and
 *    status -1; a group without a cell (-1) is all zeros but for its status;
 *  - refine = 1: per extremum the 3 x 3 stencil of psi around its cell (i, j), cells outside the grid filled by odd
 *    reflection (the mirror cell's -psi, +psi across a corner).  In index units
 *      gx = (E - W)/2, gy = (N - S)/2, Hxx = E - 2C + W, Hyy = N - 2C + S, Hxy = (NE - NW - SE + SW)/4,
 *      det = Hxx Hyy - Hxy^2, sx = -(Hyy gx - Hxy gy)/det, sy = -(Hxx gy - Hxy gx)/det,
 *      x = (i + 1/2 + sx) dx, y = (j + 1/2 + sy) dy, psi* = C + (gx sx + gy sy)/2,
 *    and omega* is the same six-term quadratic of omega, C + gx sx + gy sy + Hxx sx^2/2 + Hyy sy^2/2 + Hxy sx sy with the
 *    stencil of omega, where the cell is not on the boundary ring; on the ring it is the cell's omega.  Definiteness is
 *    judged against rounding, with eps = 2^-52 and the floors Fxx = 4 eps (|E| + 2|C| + |W|), Fyy = 4 eps (|N| + 2|C| + |S|),
 *    Fxy = eps (|NE| + |NW| + |SE| + |SW|): a fit counts only if |Hxx| > Fxx, |Hyy| > Fyy,
 *    det > Fxx |Hyy| + Fyy |Hxx| + 2 Fxy |Hxy| and Hxx > 0 for the minimum, < 0 for the three maxima.  No multiply-add of
 *    this part is contracted (tests/fv_wall_post_numpy.py states it with the same roundings);
 *  - status: 0 refined; 1 no candidate (cell -1, a corner value <= 0, or the not-finite flag); 2 flat or indefinite;
 *    3 a result that is not finite, |sx| > 1, |sy| > 1, or a point outside [0, nx dx] x [0, ny dy].  Any status but 0
 *    reports the cell's own x, y, psi and omega, and sx = sy = 0;
 *  - the mapping: seven launches per group of up to LDC_FV_WALL_LAUNCH_MAX jobs (omega | gemm x 4 | extrema | result), the
 *    launch boundary the only barrier, no waits, no atomics, every sum and merge in a fixed order.  blockIdx.y is the job
 *    and blockIdx.x the work-group within it; the x extent is the largest count among the group's jobs and a work-group
 *    beyond its own job's count returns at once.  Per job LDC_FV_WIDE_GROUPS(nx, ny) work-groups for the cell sweeps,
 *    LDC_FV_WIDE_GEMM_GROUPS(nx, ny) for a GEMM, one for `result`; the job structs travel as kernel arguments.  A job's
 *    psi, omega and block do not depend on what else is in the call, bit for bit;
 *  - scratch: LDC_FV_WALL_SCRATCH_LEN(nx, ny) doubles per job, the caller's: two fields of n, then one slot of 12 doubles
 *    per work-group of a sweep (five keys, five cells, two not-finite flags).  No two jobs of a call may share scratch,
 *    psi, omega or result.
 *
 * The same reading on a stretched tensor grid (csrc/ldc_fv_wall_post_stretched.hip, ldc_fv_wall_stretched_post_enqueue; a
 * unit of its own, every other code object stays what it was): the wall-anchored psi and the sub-cell centres of a trial
 * whose geometry comes from the per-axis tables of ldc_fv_set_grid.  A job holds raw device pointers only, no handle,
 * LDC_FV_MIN_N .. LDC_FV_WIDE_MAX_N cells per axis; the state is only read.  tests/fv_wall_stretched_numpy.py states every
 * array of it.
 *  - tables: per axis the geometry table [h (n) | d (n + 1) | g (n + 1)] above, and ONE post table of
 *    LDC_FV_WALL_STRETCHED_TABLE_LEN(n) = n (n + 2) doubles, [xc (n) | lam (n) | Q (n x n, row-major, column k the k-th
 *    vector)]: the cell centres and the generalised eigenpairs K^D q = lam H q with Q^T H Q = I, H = diag(h), K^D the 1-D
 *    stiffness with the weights 1 / d[k] on ALL n + 1 faces (the walls carry 1 / (h / 2): psi = 0 on the wall face).  Every
 *    lam > 0, there is no zero mode;
 *  - omega (ny x nx): the Gauss rule of the stretched kernels' record, (v_e - v_w) / hx[i] - (u_n - u_s) / hy[j] with the face
 *    values g[k] f_k + (1 - g[k]) f_(k-1) on inner faces, 0 on the walls and ulid[i] for u on the lid;
 *  - psi (ny x nx): (Hy (x) Kx^D + Ky^D (x) Hx) psi = (Hy (x) Hx) omega on ALL cells, solved exactly:
 *    psi = Qy ((Qy^T B Qx) / (lamy[a] + lamx[b])) Qx^T with B = V . omega, V = hx[i] hy[j] -- the four GEMMs of the uniform
 *    rule with cx = cy = 1; the omega launch leaves B in the second scratch field.  With equal widths this is
 *    (cx Tx + cy Ty) psi = omega of ldc_fv_wall_post_enqueue;
 *  - the extrema, slots 0 .. 15 and the layout of the four groups are those of ldc_fv_wall_post_enqueue; a group's own
 *    values are x = xc[i], y = yc[j], psi and omega of the cell;
 *  - refine = 1: the 3 x 3 stencil with odd reflection as above, in PHYSICAL coordinates.  With dw = dx[i], de = dx[i+1],
 *    ds = dy[j], dn = dy[j+1] the distances to the neighbours' centres (d of the geometry table; beyond a wall the mirror
 *    cell lies at 2 d_wall = h),
 *      gx  = ((E - C) dw / de + (C - W) de / dw) / (dw + de),      Hxx = 2 ((E - C) / de - (C - W) / dw) / (dw + de),
 *      gy, Hyy likewise with N, S, ds, dn,                          Hxy = (NE - NW - SE + SW) / ((dw + de) (ds + dn)),
 *      det = Hxx Hyy - Hxy^2, sx = -(Hyy gx - Hxy gy) / det, sy = -(Hxx gy - Hxy gx) / det   (lengths),
 *      x = xc[i] + sx, y = yc[j] + sy, psi* = C + (gx sx + gy sy) / 2,
 *    exact for a six-term quadratic on any spacing; omega* is the same quadratic of omega off the boundary ring, the cell's
 *    omega on it.  The floors are those of the uniform rule carried through the same divisions, every |term| divided as its
 *    value is: Fxx = 4 eps 2 ((|E| + |C|) / de + (|C| + |W|) / dw) / (dw + de), Fyy likewise,
 *    Fxy = 4 eps (|NE| + |NW| + |SE| + |SW|) / ((dw + de) (ds + dn)); the definiteness rule and its signs are unchanged.  No
 *    multiply-add of omega, B or the refinement is contracted;
 *  - status: as above, with 3 for a result that is not finite, sx outside [-dw, de], sy outside [-ds, dn] (the step leaves
 *    the stencil) or a point outside [0, xc[nx-1] + d[nx]] x [0, yc[ny-1] + d[ny]].  LDC_FV_WALL_SX / SY hold the step as a
 *    fraction of the distance to the neighbour on its side: sx / dw for sx < 0, else sx / de (the uniform value with equal
 *    widths).  Any status but 0 reports the cell's own values and sx = sy = 0;
 *  - the mapping and the scratch (LDC_FV_WALL_SCRATCH_LEN) are those of ldc_fv_wall_post_enqueue, seven launches per group of
 *    up to LDC_FV_WALL_STRETCHED_LAUNCH_MAX jobs; a job's psi, omega and block do not depend on what else is in the call,
 *    bit for bit.  Two jobs may share tables, never scratch, psi, omega or result.
 *
 * The coarse-to-fine transfer on tensor grids with any spacing per axis (csrc/ldc_fv_prolong_tables.hip,
 * ldc_fv_prolong_tables_enqueue; a unit of its own, every other code object stays what it was): what ldc_fv_prolong_enqueue
 * does for two equally spaced trials, with the geometry of both read from tables, so that a stretched trial can start from a
 * coarser one, from a trial of its own size at another Re, or from a uniform one (and the other way round).  A job holds raw
 * device pointers only, no handle (a uniform source has no tables on its handle), LDC_FV_MIN_N .. LDC_FV_MAX_N cells per
 * axis on both sides; the coarse state is only read.  tests/fv_prolong_tables_numpy.py states it operation by operation.
 *  - tables: per coarse axis ONE table of its n cell centres, ascending inside (0, L); per fine axis the same, and the
 *    geometry table [h (n) | d (n + 1) | g (n + 1)] of ldc_fv_set_grid (for an equally spaced trial the table of its vertices
 *    k L / n); Lx, Ly are the domain lengths of BOTH trials;
 *  - the extended coarse axis has the nodes e_0 = 0, e_k = xc[k-1] (k = 1 .. n), e_(n+1) = L; the ring values are those of
 *    ldc_fv_prolong_enqueue: u and v 0.0 on the walls and corners, u above cell i on the lid the COARSE ulid[i], p repeats the
 *    nearest cell;
 *  - a fine centre x takes the largest k <= n with e_k <= x (k = 0 when there is none), found by bisection, and the weight
 *    t = (x - e_k) / (e_(k+1) - e_k); the value is bilinear with x first, lo = a + tx (b - a), hi likewise on the row above,
 *    then lo + ty (hi - lo); every thread subtracts from p the interpolated p at fine cell 0, so p[0] is exactly 0.0;
 *  - mdot from the new u and v by the face rule of the stretched kernels: x face i of row j, 0 < i < nx, is
 *    rho ((g_x[i] u[j][i] + (1 - g_x[i]) u[j][i-1]) hy[j]), the y faces likewise with g_y and hx; the faces on the four walls
 *    are exactly 0.0.  No multiply-add is contracted;
 *  - the mapping: one work-group of 512 threads per job, LDC_FV_PROLONG_TABLES_LAUNCH_MAX jobs per launch, the job structs
 *    travelling as kernel arguments, no waits between work-groups, no reduction, no scratch.  (k, t) of the nx + ny fine
 *    centres go to LDS first, one bisection per thread; then the cells; then the faces, a barrier between the phases.  A job's
 *    result does not depend on what else is in the call, bit for bit;
 *  - written: the fine u, v, p (ny x nx each) and mdot (LDC_FV_FACES), nothing else: no ctrl, no rec, no work vector.
 *
 * The same transfer over the whole chip (csrc/ldc_fv_wide_prolong_tables.hip, ldc_fv_wide_prolong_tables_enqueue; a unit of its
 * own, every other code object stays what it was): the job struct, the tables, the checks and the arithmetic above -- one
 * definition for both units, csrc/ldc_fv_prolong_tables_cells.inc, no multiply-add contracted -- for LDC_FV_MIN_N ..
 * LDC_FV_WIDE_MAX_N cells per axis on both sides, so a pair that both entries take gets the same bits from either.  The
 * source may be a trial of any mapping and grid; the coarse state is only read.
 *  - the mapping is the chip mapping's: LDC_FV_WIDE_PROLONG_TABLES_LAUNCHES = 2 launches per job, `cells` and `faces`, of
 *    LDC_FV_WIDE_GROUPS(fine_nx, fine_ny) work-groups of 256 threads each (a grid that depends on the fine sizes alone), the
 *    launch boundary the only barrier between work-groups, no work-group reading what another of the same launch writes, no
 *    scratch in global memory, no atomics, no waits.  The jobs of a call are launched one after another, each job travelling
 *    by value in the kernel arguments;
 *  - `cells`: every work-group fills its own LDS with (k, t) of all fine_nx + fine_ny fine centres (at most 2048 entries,
 *    24 KB, eight bisections per thread) and, after one work-group barrier, strides over the fine cells; every thread forms
 *    the interpolated p at fine cell 0 for itself.  `faces` strides over the x faces, then the y faces.  (k, t) of a centre
 *    does not depend on who computes it: a job's result does not depend on the grouping or on the other jobs, bit for bit;
 *  - written: the fine u, v, p and mdot, nothing else: no ctrl, no rec, no work vector, no scratch of the solve, no table.
 */
#ifndef LDC_FV_H
#define LDC_FV_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LDC_FV_VERSION 2
#define LDC_FV_MIN_N 8
#define LDC_FV_MAX_N 256
#define LDC_FV_REC_LEN 8
#define LDC_FV_CTRL_LEN 8
#define LDC_FV_NWORK 32            /* work vectors of n doubles */
#define LDC_FV_DESC_DOUBLES 64     /* + the trial's device-side descriptor */
#define LDC_FV_WORK_LEN(nx, ny) (LDC_FV_NWORK * (int64_t)(nx) * (ny) + LDC_FV_DESC_DOUBLES)
#define LDC_FV_FACES(nx, ny) ((int64_t)(ny) * ((nx) + 1) + (int64_t)((ny) + 1) * (nx))
#define LDC_FV_LAUNCH_MAX 256      /* trials per launch of ldc_fv_batch_enqueue (more: several launches) */
#define LDC_FV_PROLONG_LAUNCH_MAX 128 /* pairs per launch of ldc_fv_prolong_enqueue: two descriptors per pair in the arguments */
#define LDC_FV_SAMPLE_LAUNCH_MAX 32  /* jobs per launch of ldc_fv_sample_nodes: 112 bytes per job in the arguments */
#define LDC_FV_ANDERSON_LAUNCH_MAX 96 /* trials per launch of the mixing kernel: 32 bytes per trial in the arguments */
#define LDC_FV_ANDERSON_MAX_DEPTH 16
#define LDC_FV_ANDERSON_STATE_LEN 4
#define LDC_FV_ANDERSON_HIST_LEN(nx, ny, depth) ((2 * (int64_t)(depth) + 3) * (3 * (int64_t)(nx) * (ny) + LDC_FV_FACES(nx, ny)))
#define LDC_FV_E_NAN (-5)          /* ldc_fv_status: the trial produced a NaN and stopped */
#define LDC_FV_WIDE_MAX_N 1024     /* cells per axis of a trial on the whole chip */
#define LDC_FV_WIDE_GRAPH_DEFAULT 0 /* ldc_fv_wide_set_graph of a new handle (profiles/fv_wide.md) */
#define LDC_FV_WIDE_E_BUDGET (-6)  /* ldc_fv_wide_status: the last enqueue stopped for want of BiCGSTAB launches */
/* work-groups of a sweep over the cells (one slot of partial sums each) and the caller's scratch, in doubles */
#define LDC_FV_WIDE_GROUPS(nx, ny) ((((int64_t)(nx) * (ny) + 255) / 256) < 256 ? (((int64_t)(nx) * (ny) + 255) / 256) : 256)
#define LDC_FV_WIDE_SCRATCH_LEN(nx, ny) (80 + 30 * LDC_FV_WIDE_GROUPS(nx, ny))
/* several trials in the same launches (ldc_fv_wide_batch_*): trials per batch, work-groups of one trial's GEMM launches,   */
/* and the BYTES of the caller's device buffer for the batch's table: n entries, then one word per work-group of a cell  */
/* sweep (sweep_groups: the sum of LDC_FV_WIDE_GROUPS over the trials) and of a GEMM launch (gemm_groups: likewise)      */
#define LDC_FV_WIDE_BATCH_MAX 256
#define LDC_FV_WIDE_BATCH_ENTRY_BYTES 256
#define LDC_FV_WIDE_GEMM_GROUPS(nx, ny) ((((int64_t)(ny) + 15) / 16 * (((nx) + 15) / 16) + 3) / 4)
#define LDC_FV_WIDE_BATCH_TABLE_LEN(n, sweep_groups, gemm_groups) (LDC_FV_WIDE_BATCH_ENTRY_BYTES * (int64_t)(n) + 4 * ((int64_t)(sweep_groups) + (int64_t)(gemm_groups)))
/* the caller's scratch of ldc_fv_wide_post_enqueue, in doubles: one slot per work-group of a cell sweep (five keys, five  */
/* cells, two not-finite flags)                                                                                           */
#define LDC_FV_WIDE_POST_SCRATCH_LEN(nx, ny) (12 * LDC_FV_WIDE_GROUPS(nx, ny))
/* Anderson mixing of a chip or shared trial (ldc_fv_wide_set_anderson): the launches it adds to an iteration, and the     */
/* caller's mixing scratch in doubles: 8 words, then per work-group of a sweep b[depth] and the lower triangle of A        */
#define LDC_FV_WIDE_ANDERSON_LAUNCHES 3
#define LDC_FV_WIDE_ANDERSON_SCRATCH_LEN(nx, ny, depth) (8 + LDC_FV_WIDE_GROUPS(nx, ny) * ((int64_t)(depth) * ((depth) + 3) / 2))

/* The consistent pressure equation of a chip or shared trial (ldc_fv_wide_set_pressure): the modes, the launches of one   */
/* CG iteration, the CG iterations a new handle's enqueue carries per SIMPLE iteration, the caller's statistics words       */
#define LDC_FV_PRESSURE_REFERENCE 0
#define LDC_FV_PRESSURE_CONSISTENT 1
#define LDC_FV_WIDE_PRESSURE_LAUNCHES 7
#define LDC_FV_WIDE_PRESSURE_BUDGET_DEFAULT 12
#define LDC_FV_WIDE_PRESSURE_SCRATCH_LEN 4
#define LDC_FV_PRESSURE_STATS_LEN 4 /* the statistics words of ldc_fv_set_pressure (a one-CU trial) */
/* ldc_fv_set_grid: the modes and the doubles of one axis' table [h (n) | d (n + 1) | g (n + 1)] */
#define LDC_FV_GRID_UNIFORM 0
#define LDC_FV_GRID_TABLES 1
#define LDC_FV_GRID_TABLE_LEN(n) (3 * (int64_t)(n) + 2)
/* ldc_fv_set_preconditioner: the modes and the doubles of one axis' table [a (n) | lam (n) | Q (n x n)] */
#define LDC_FV_PRECOND_LAPLACIAN 0
#define LDC_FV_PRECOND_SEPARABLE 1
#define LDC_FV_PRECOND_TABLE_LEN(n) ((int64_t)(n) * ((int64_t)(n) + 2))
/* ldc_fv_wall_post_enqueue: jobs per launch (136 bytes per job in the arguments), the caller's scratch per job in doubles, */
/* the result block (the LDC_FV_POST_* slots, then four groups) and the slots of a group                                   */
#define LDC_FV_WALL_LAUNCH_MAX 24
#define LDC_FV_WALL_SCRATCH_LEN(nx, ny) (2 * (int64_t)(nx) * (ny) + 12 * LDC_FV_WIDE_GROUPS(nx, ny))
#define LDC_FV_WALL_GROUP_LEN 8
#define LDC_FV_WALL_RESULT_LEN 48  /* LDC_FV_POST_RESULT_LEN + 4 groups: the primary minimum, BR, BL, TL */
#define LDC_FV_WALL_X 0
#define LDC_FV_WALL_Y 1
#define LDC_FV_WALL_PSI 2
#define LDC_FV_WALL_OMEGA 3
#define LDC_FV_WALL_STATUS 4       /* -1 not asked for, 0 refined, 1 no candidate, 2 flat or indefinite, 3 rejected */
#define LDC_FV_WALL_SX 5           /* the step from the cell centre, in cells */
#define LDC_FV_WALL_SY 6
/* ldc_fv_wall_stretched_post_enqueue: jobs per launch (120 bytes per job in the arguments) and the doubles of one axis'    */
/* post table [xc (n) | lam (n) | Q (n x n)]; the scratch, the result block and the slots of a group are those above, with   */
/* LDC_FV_WALL_SX / SY as fractions of the distance to the neighbour on the step's side                                    */
#define LDC_FV_WALL_STRETCHED_LAUNCH_MAX 32
#define LDC_FV_WALL_STRETCHED_TABLE_LEN(n) ((int64_t)(n) * ((int64_t)(n) + 2))
/* ldc_fv_prolong_tables_enqueue: jobs per launch (152 bytes per job in the arguments) */
#define LDC_FV_PROLONG_TABLES_LAUNCH_MAX 23
/* ldc_fv_wide_prolong_tables_enqueue: launches per job (cells | faces) */
#define LDC_FV_WIDE_PROLONG_TABLES_LAUNCHES 2

/* intermediates of ldc_fv_step_debug (bit k of `which` selects out[k]) and their lengths */
#define LDC_FV_DBG_GRAD_P 0        /* 2n: d/dx p, then d/dy p                                    */
#define LDC_FV_DBG_DIAG 1          /* 5n: aP (unrelaxed), aW, aE, aS, aN                          */
#define LDC_FV_DBG_B 2             /* 2n: b_u, b_v of the assembly (boundary + deferred correction) */
#define LDC_FV_DBG_USTAR 3         /* n */
#define LDC_FV_DBG_VSTAR 4         /* n */
#define LDC_FV_DBG_MDOT_STAR 5     /* faces */
#define LDC_FV_DBG_RHS_P 6         /* n: -div mdot*, entry 0 = 0 */
#define LDC_FV_DBG_P_PRIME 7       /* n */
#define LDC_FV_DBG_U_PRIME 8       /* n */
#define LDC_FV_DBG_V_PRIME 9       /* n */
#define LDC_FV_DBG_MDOT 10         /* faces */
#define LDC_FV_DBG_COUNT 11

struct ldc_fv_problem {
  int32_t nx, ny;                 /* LDC_FV_MIN_N .. LDC_FV_MAX_N each */
  int32_t scheme;                 /* 0 = Upwind, 1 = TVD (MUSCL; DESIGN.md FV-Q1) */
  int32_t rec_cap;                /* rows of rec: the most iterations one enqueue may run */
  int32_t warmup;                 /* no convergence test before this many iterations (10) */
  int32_t max_lin_iters;          /* BiCGSTAB iterations per momentum solve (1000) */
  double dx, dy;                  /* Lx / nx, Ly / ny */
  double rho, mu;                 /* density, viscosity rho * U * Lx / Re */
  double alpha_uv, alpha_p;       /* under-relaxation, each in (0, 1] */
  double lin_tol;                 /* BiCGSTAB rtol relative to |b| (atol = 0) */
  double tol;                     /* outer latch on the relative change of u, v */
  double lid_velocity;            /* u on the lid in E/Z/P's ghost cells (base.py:424-425) */
  const double *ulid;             /* nx: u on the lid faces (the lid profile of the mesh) */
  const double *Qx, *lamx, *Qy, *lamy;
  double *u, *v, *p, *mdot;       /* state: n, n, n, faces */
  double *work;                   /* LDC_FV_WORK_LEN(nx, ny) */
  double *rec;                    /* rec_cap * LDC_FV_REC_LEN */
  int64_t *ctrl;                  /* LDC_FV_CTRL_LEN */
};

/* slots of a result block of ldc_fv_post_enqueue */
#define LDC_FV_POST_PSI_MIN 0          /* min psi */
#define LDC_FV_POST_OMEGA_CENTER 1     /* omega at the cell of min psi */
#define LDC_FV_POST_OMEGA_MAX 2        /* the signed omega at the cell of max |omega| */
#define LDC_FV_POST_PSI_BR 3           /* max psi inside BR, BL, TL (-inf for a region without cells); the caller */
#define LDC_FV_POST_PSI_BL 4           /* keeps one that is > 0 */
#define LDC_FV_POST_PSI_TL 5
#define LDC_FV_POST_PSI_MIN_CELL 6     /* their cells c = j*nx + i, in the same order */
#define LDC_FV_POST_OMEGA_MAX_CELL 7
#define LDC_FV_POST_PSI_BR_CELL 8
#define LDC_FV_POST_PSI_BL_CELL 9
#define LDC_FV_POST_PSI_TL_CELL 10
#define LDC_FV_POST_NONFINITE 11       /* non-zero: some omega or psi is not finite, the other slots mean nothing */
#define LDC_FV_POST_RESULT_LEN 16      /* (the rest is written as 0) */

struct ldc_fv_post {
  const double *Sx, *lamx;        /* sine eigenvectors (nx-2)^2 and eigenvalues (nx-2) */
  const double *Sy, *lamy;        /* the same for ny-2 */
  int32_t ix_lt, ix_gt;           /* cells with x < 0.5: i < ix_lt; with x > 0.5: i >= ix_gt */
  int32_t jy_lt, jy_gt;           /* cells with y < 0.5: j < jy_lt; with y > 0.5: j >= jy_gt */
  double *psi, *omega;            /* out: n each */
  double *result;                 /* out: LDC_FV_POST_RESULT_LEN */
};

struct ldc_fv_anderson {
  int32_t depth;                  /* 0 .. LDC_FV_ANDERSON_MAX_DEPTH columns; 0: no mixing (a plain trial in the same call) */
  int32_t start;                  /* mixing from this iteration count on (>= 1) */
  double *hist;                   /* LDC_FV_ANDERSON_HIST_LEN(nx, ny, depth) device doubles (depth 0: may be NULL) */
  int64_t hist_len;               /* the length of hist */
  int64_t *astate;                /* device int64[LDC_FV_ANDERSON_STATE_LEN]: valid columns, ring position, the iteration */
                                  /* count seen last, fallbacks taken.  Zero it exactly when ctrl is zeroed. */
};

struct ldc_fv_pressure {
  int32_t mode;                   /* LDC_FV_PRESSURE_REFERENCE (the exact solve of the constant-coefficient Laplacian) or */
                                  /* LDC_FV_PRESSURE_CONSISTENT (CG on the a_P-weighted operator)                          */
  int32_t max_iters;              /* CG iterations per solve (>= 1); the iterate is accepted after that many              */
  double tol;                     /* CG stops at |r|_2 <= tol |b|_2 (0 < tol < 1)                                          */
};

struct ldc_fv_grid {
  int32_t mode;                   /* LDC_FV_GRID_UNIFORM (dx, dy of the problem) or LDC_FV_GRID_TABLES */
  int32_t pad;
  const double *x_tables;         /* device: LDC_FV_GRID_TABLE_LEN(nx) doubles, [h | d | g] of the x axis */
  const double *y_tables;         /* device: LDC_FV_GRID_TABLE_LEN(ny) doubles, the same for y */
  int64_t x_len, y_len;           /* the lengths of the two buffers */
};

struct ldc_fv_precond {
  int32_t mode;                   /* LDC_FV_PRECOND_LAPLACIAN (the operator with D left out) or LDC_FV_PRECOND_SEPARABLE */
  int32_t pad;
  const double *x_table;          /* device: LDC_FV_PRECOND_TABLE_LEN(nx) doubles, [a | lam | Q] of the x axis */
  const double *y_table;          /* device: LDC_FV_PRECOND_TABLE_LEN(ny) doubles, the same for y (b in place of a) */
  int64_t x_len, y_len;           /* the lengths of the two buffers */
};

struct ldc_fv_sample_job {
  const double *u, *v, *p;        /* source: the FV state at the cells c = j*nx + i (n each) */
  const double *ulid;             /* source: the FV lid profile (nx) */
  int32_t nx, ny;                 /* LDC_FV_MIN_N .. LDC_FV_WIDE_MAX_N each */
  double dx, dy;                  /* > 0 */
  const double *x, *y;            /* target: node coordinates, ascending, Mx inside [0, nx dx] and My inside [0, ny dy] */
  const double *ulid_nodes;       /* target: its own u on the lid (Mx) */
  int32_t Mx, My;                 /* >= 3 each */
  double *U, *V;                  /* out: Mx * My each, element (ix, iy) at ix * My + iy */
  double *P;                      /* out: (Mx - 2) * (My - 2), the inner nodes */
};

struct ldc_fv_wall_job {
  const double *u, *v, *ulid;     /* cell-centred state (ny x nx, c = j*nx + i), lid profile (nx) */
  const double *Cx, *lamx, *Cy, *lamy; /* the tables above: nx x nx and ny x ny row-major, nx and ny */
  double *psi, *omega;            /* out: ny x nx each */
  double *scratch;                /* LDC_FV_WALL_SCRATCH_LEN(nx, ny) */
  double *result;                 /* out: LDC_FV_WALL_RESULT_LEN */
  double dx, dy;                  /* > 0 */
  int32_t nx, ny;                 /* LDC_FV_MIN_N .. LDC_FV_WIDE_MAX_N each */
  int32_t ix_lt, ix_gt;           /* as in ldc_fv_post: 0 .. nx */
  int32_t jy_lt, jy_gt;           /* 0 .. ny */
  int32_t refine, pad;            /* 0: the cells' own values in the groups; 1: the quadratic fit */
};

struct ldc_fv_wall_stretched_job {
  const double *u, *v, *ulid;     /* cell-centred state (ny x nx, c = j*nx + i), lid profile at the cell centres (nx) */
  const double *x_grid, *y_grid;  /* the geometry tables [h | d | g]: LDC_FV_GRID_TABLE_LEN(nx), LDC_FV_GRID_TABLE_LEN(ny) */
  const double *x_post, *y_post;  /* the post tables [xc | lam | Q]: LDC_FV_WALL_STRETCHED_TABLE_LEN(nx), .. (ny) */
  double *psi, *omega;            /* out: ny x nx each */
  double *scratch;                /* LDC_FV_WALL_SCRATCH_LEN(nx, ny) */
  double *result;                 /* out: LDC_FV_WALL_RESULT_LEN */
  int32_t nx, ny;                 /* LDC_FV_MIN_N .. LDC_FV_WIDE_MAX_N each */
  int32_t ix_lt, ix_gt;           /* as in ldc_fv_post: 0 .. nx */
  int32_t jy_lt, jy_gt;           /* 0 .. ny */
  int32_t refine, pad;            /* 0: the cells' own values in the groups; 1: the quadratic fit */
};

struct ldc_fv_prolong_tables_job {
  const double *coarse_u, *coarse_v, *coarse_p; /* the coarse state (coarse_ny x coarse_nx, c = j*nx + i): only read */
  const double *coarse_ulid;      /* the coarse lid profile (coarse_nx) */
  const double *coarse_xc, *coarse_yc; /* the coarse cell centres (coarse_nx), (coarse_ny) */
  double *fine_u, *fine_v, *fine_p; /* out: fine_ny x fine_nx each */
  double *fine_mdot;              /* out: LDC_FV_FACES(fine_nx, fine_ny) */
  const double *fine_x_grid, *fine_y_grid; /* the fine geometry tables [h | d | g]: LDC_FV_GRID_TABLE_LEN(fine_nx), .. (fine_ny) */
  const double *fine_xc, *fine_yc; /* the fine cell centres (fine_nx), (fine_ny) */
  double Lx, Ly;                  /* > 0: the domain of both trials */
  double rho;                     /* > 0: the fine trial's */
  int32_t coarse_nx, coarse_ny;   /* LDC_FV_MIN_N .. LDC_FV_MAX_N each (ldc_fv_wide_prolong_tables_enqueue: .. LDC_FV_WIDE_MAX_N) */
  int32_t fine_nx, fine_ny;       /* likewise */
};

typedef struct ldc_fv ldc_fv;
typedef struct ldc_fv_wide ldc_fv_wide;
typedef struct ldc_fv_wide_batch ldc_fv_wide_batch;

int ldc_fv_version(void);
/* Validate (no device needed), then write the trial's descriptor into the tail of `work` (synchronous copy on the */
/* library's own stream: work the caller has queued on `work` must have completed).                                 */
int ldc_fv_create(const struct ldc_fv_problem *prob, ldc_fv **out);
int ldc_fv_destroy(ldc_fv *h);
/* Up to n_iters SIMPLE iterations (<= rec_cap) in one launch; stops early at the latch or a NaN. */
int ldc_fv_enqueue(ldc_fv *h, int n_iters, void *stream);
/* The same for n trials (any sizes and parameters, one device): one work-group each. */
int ldc_fv_batch_enqueue(ldc_fv *const *hs, int n, int n_iters, void *stream);
/* 0, or LDC_FV_E_NAN when the trial stopped on a NaN (reads ctrl through the library's own stream: wait for the */
/* stream of the trial's launches first). */
int ldc_fv_status(ldc_fv *h);
/* One iteration, copying the intermediates selected by `which` into out[k] (device pointers).  LDC_E_ARG for a handle in */
/* mode LDC_FV_PRESSURE_CONSISTENT (its work vectors hold the intermediates).                                              */
int ldc_fv_step_debug(ldc_fv *h, int which, double *const *out, void *stream);
/* The pressure equation of a one-CU trial: cfg == NULL or mode LDC_FV_PRESSURE_REFERENCE is the kernel of a new handle;     */
/* mode LDC_FV_PRESSURE_CONSISTENT the one described above, with `stats` a device buffer of stats_len >=                      */
/* LDC_FV_PRESSURE_STATS_LEN int64 words owned by the caller.  Call it between solves, with nothing of the handle in flight   */
/* (one synchronous copy into the tail of `work` on the library's own stream).  Validation comes first and needs no device:   */
/* LDC_E_STATE for a null handle; LDC_E_ARG for another mode, max_iters < 1, tol outside (0, 1) or NaN, a null or short       */
/* stats.  A refused call leaves the handle as it was.                                                                        */
int ldc_fv_set_pressure(ldc_fv *h, const struct ldc_fv_pressure *cfg, int64_t *stats, int64_t stats_len);
/* The grid of a one-CU trial: grid == NULL or mode LDC_FV_GRID_UNIFORM is the grid of a new handle (dx, dy); mode              */
/* LDC_FV_GRID_TABLES attaches the per-axis tables described above, device buffers owned by the caller and left alone while   */
/* the handle lives in that mode; the problem's Qx, lamx, Qy, lamy and ulid must then be those of that grid.  Call it between  */
/* solves, with nothing of the handle in flight (one synchronous copy into the tail of `work` on the library's own stream).   */
/* Validation comes first and needs no device: LDC_E_STATE for a null handle; LDC_E_ARG for another mode, a null table or a   */
/* length below LDC_FV_GRID_TABLE_LEN.  A refused call leaves the handle as it was.  The pressure mode is kept either way.    */
int ldc_fv_set_grid(ldc_fv *h, const struct ldc_fv_grid *grid);
/* The preconditioner of the consistent pressure equation on a handle with geometry tables: cfg == NULL or mode                */
/* LDC_FV_PRECOND_LAPLACIAN is that of a new handle; mode LDC_FV_PRECOND_SEPARABLE attaches the per-axis tables described      */
/* above, device buffers owned by the caller and left alone while the handle lives in that mode.  Call it after                */
/* ldc_fv_set_grid, between solves, with nothing of the handle in flight (one synchronous copy into the tail of `work`).  A    */
/* call of ldc_fv_set_grid that makes the handle uniform restores the behaviour of before too: a uniform handle runs the       */
/* uniform kernels whatever this mode says, and attaching geometry tables again resets it to LDC_FV_PRECOND_LAPLACIAN (the     */
/* tables belong to the mesh they were fitted to).  Validation comes first and needs no device: LDC_E_STATE for a null handle; */
/* LDC_E_ARG for another mode, a handle without geometry tables, a null table or a length below LDC_FV_PRECOND_TABLE_LEN.  A   */
/* refused call leaves the handle as it was.                                                                                   */
int ldc_fv_set_preconditioner(ldc_fv *h, const struct ldc_fv_precond *cfg);
/* omega, psi and the result block of n trials (any sizes, one device), one work-group each; trial q takes posts[q]. */
/* Validation comes first and needs no device.  The trials must not be in flight on another stream.                  */
int ldc_fv_post_enqueue(ldc_fv *const *hs, const struct ldc_fv_post *posts, int n, void *stream);
/* fine[q] <- the prolongation of coarse[q] for n pairs (any sizes, one device), one work-group of 512 threads each and */
/* no waits between them; more than LDC_FV_PROLONG_LAUNCH_MAX pairs: several launches.  Validation comes first, and its  */
/* first part needs no device: LDC_E_ARG for a null list or n < 1, LDC_E_STATE for a null handle; then LDC_E_STATE for  */
/* a handle of another device, LDC_E_ARG for a size outside LDC_FV_MIN_N .. LDC_FV_MAX_N, for a pair whose domains      */
/* differ (nx dx or ny dy, beyond 1e-12 relative), for coarse[q] == fine[q] and for a fine trial that is also the       */
/* coarse or the fine trial of another pair of the call, however many launches it takes (its pairs are unordered).      */
/* The library keeps no record of launches: that no trial is in flight on another stream is the caller's to see to.     */
int ldc_fv_prolong_enqueue(ldc_fv *const *coarse, ldc_fv *const *fine, int n, void *stream);
/* n_iters accelerated iterations of n trials (any sizes and parameters, one device): for every iteration             */
/* ldc_fv_batch_enqueue(hs, n, 1, stream), then the mixing kernel, one work-group of 512 threads per trial and no waits */
/* between them, LDC_FV_ANDERSON_LAUNCH_MAX trials per launch; trial q takes acc[q].  All of it is enqueued; nothing    */
/* synchronises.  Validation runs as a whole before any launch, and its first part needs no device: LDC_E_ARG for a    */
/* null list, n < 1 or n_iters < 1; then per trial, in list order, LDC_E_STATE for a null handle and LDC_E_ARG for      */
/* depth outside 0 .. 16, start < 1, a null astate, n_iters > rec_cap, and with depth > 0 a null hist or a hist_len     */
/* below LDC_FV_ANDERSON_HIST_LEN.  Then LDC_E_NODEVICE, and LDC_E_STATE for a handle of another device.  A trial may    */
/* appear once in a call, and no two trials may share hist or astate: that is the caller's to see to.                   */
int ldc_fv_anderson_enqueue(ldc_fv *const *hs, const struct ldc_fv_anderson *acc, int n, int n_iters, void *stream);
/* A trial advanced by the whole chip.  Validation is ldc_fv_create's with nx, ny up to LDC_FV_WIDE_MAX_N, a non-null   */
/* scratch and scratch_len >= LDC_FV_WIDE_SCRATCH_LEN(nx, ny); it comes first and needs no device.  Nothing is copied   */
/* or launched: the arrays may be shared with an ldc_fv handle of the same problem (one of the two in flight at a time). */
int ldc_fv_wide_create(const struct ldc_fv_problem *prob, double *scratch, int64_t scratch_len, ldc_fv_wide **out);
int ldc_fv_wide_destroy(ldc_fv_wide *h);
/* Up to n_iters SIMPLE iterations (1 .. rec_cap) with lin_budget (>= 1) BiCGSTAB iterations each, all launches enqueued */
/* on `stream`; stops early at the latch, a NaN or the overflow.  LDC_E_STATE for a null handle, then LDC_E_ARG, then     */
/* the device.                                                                                                          */
int ldc_fv_wide_enqueue(ldc_fv_wide *h, int n_iters, int lin_budget, void *stream);
/* on = 1: an enqueue replays ONE captured iteration per budget value (a linear hipGraph of that iteration's launches,   */
/* captured at the first enqueue with that budget and kept until destroy; budgets above 64 are launched one by one);   */
/* on = 0: every kernel is launched on its own.  Same kernels, same order, same results.  A new handle starts with      */
/* LDC_FV_WIDE_GRAPH_DEFAULT.  destroy waits for the last replay before it frees the graphs.                            */
int ldc_fv_wide_set_graph(ldc_fv_wide *h, int on);
/* Kernel launches of ONE iteration at that budget (an enqueue adds one), LDC_FV_WIDE_ANDERSON_LAUNCHES of them the mixing */
/* chain's when the handle has one.  Needs no device. */
int ldc_fv_wide_launches(const ldc_fv_wide *h, int lin_budget);
/* Attach Anderson mixing to the handle (acc->depth 1 .. LDC_FV_ANDERSON_MAX_DEPTH), or detach it (acc == NULL or depth 0): */
/* every iteration of ldc_fv_wide_enqueue then ends on the mixing chain.  `acc` is the struct of ldc_fv_anderson_enqueue;   */
/* `scratch` is a device buffer of scratch_len >= LDC_FV_WIDE_ANDERSON_SCRATCH_LEN(nx, ny, depth) doubles owned by the       */
/* caller.  Call it between solves, with nothing of the handle in flight: zero astate exactly when ctrl is zeroed.  The      */
/* handle's captured iterations are freed (after the last replay): they are captured again with the new block.  Validation */
/* comes first and needs no device: LDC_E_STATE for a null handle; LDC_E_ARG for depth outside 0 .. 16, start < 1, a null    */
/* astate, and with depth > 0 a null hist, a hist_len below LDC_FV_ANDERSON_HIST_LEN, a null or short scratch.  A batch      */
/* copies the block at ldc_fv_wide_batch_create: attach before creating it.                                                  */
int ldc_fv_wide_set_anderson(ldc_fv_wide *h, const struct ldc_fv_anderson *acc, double *scratch, int64_t scratch_len);
/* The pressure equation of the handle: cfg == NULL or mode LDC_FV_PRESSURE_REFERENCE is the chain of a new handle; mode    */
/* LDC_FV_PRESSURE_CONSISTENT the one described above, with `scratch` a device buffer of scratch_len >=                       */
/* LDC_FV_WIDE_PRESSURE_SCRATCH_LEN int64 words owned by the caller (the statistics).  Call it between solves, with nothing   */
/* of the handle in flight, and before ldc_fv_wide_batch_create; the handle's captured iterations are freed.  Validation      */
/* needs no device: LDC_E_STATE for a null handle; LDC_E_ARG for another mode, max_iters < 1, tol outside (0, 1), a null or   */
/* short scratch.                                                                                                             */
int ldc_fv_wide_set_pressure(ldc_fv_wide *h, const struct ldc_fv_pressure *cfg, double *scratch, int64_t scratch_len);
/* The grid of the handle: grid == NULL or mode LDC_FV_GRID_UNIFORM is the grid of a new handle (dx, dy); mode                */
/* LDC_FV_GRID_TABLES attaches the per-axis tables of ldc_fv_set_grid (the same struct and layout), device buffers owned by   */
/* the caller and left alone while the handle lives in that mode; the problem's Qx, lamx, Qy, lamy and ulid must then be      */
/* those of that grid.  The two pointers travel by value in the kernel arguments: nothing is copied, and the handle's         */
/* captured iterations are freed.  Call it between solves, with nothing of the handle in flight.  Validation comes first and  */
/* needs no device: LDC_E_ARG for a null handle, another mode, a null table, a length below LDC_FV_GRID_TABLE_LEN, and for     */
/* tables on a handle with Anderson mixing attached.  A refused call leaves the handle as it was.  The pressure mode is kept  */
/* either way.  A handle with tables is refused (LDC_E_ARG) by ldc_fv_wide_set_anderson with depth > 0,                        */
/* ldc_fv_wide_batch_create, ldc_fv_wide_post_enqueue and ldc_fv_wide_prolong_enqueue.                                         */
int ldc_fv_wide_set_grid(ldc_fv_wide *h, const struct ldc_fv_grid *grid);
/* The preconditioner of the consistent pressure equation on a handle with geometry tables: cfg == NULL or mode               */
/* LDC_FV_PRECOND_LAPLACIAN is that of a new handle; mode LDC_FV_PRECOND_SEPARABLE attaches the per-axis tables of              */
/* ldc_fv_set_preconditioner (the same struct and layout), device buffers owned by the caller and left alone while the handle */
/* lives in that mode.  The two pointers travel by value in the kernel arguments: nothing is copied, and the handle's          */
/* captured iterations are freed.  Call it after ldc_fv_wide_set_grid, between solves, with nothing of the handle in flight;   */
/* ldc_fv_wide_set_grid resets the mode to LDC_FV_PRECOND_LAPLACIAN whenever it attaches or detaches tables.  Validation comes */
/* first and needs no device: LDC_E_ARG for a null handle, another mode, a handle without geometry tables, a null table or a   */
/* length below LDC_FV_PRECOND_TABLE_LEN.  A refused call leaves the handle as it was.  Either pressure mode takes the call;   */
/* the chain reads the tables in consistent mode only.                                                                         */
int ldc_fv_wide_set_preconditioner(ldc_fv_wide *h, const struct ldc_fv_precond *cfg);
/* The CG iterations the next enqueues carry per SIMPLE iteration (>= 1; min(budget, max_iters) x 7 launches).  LDC_E_ARG for */
/* a handle in the reference mode.  Graphs are kept: they are keyed on both budgets.                                          */
int ldc_fv_wide_set_pressure_budget(ldc_fv_wide *h, int budget);
/* The same for a batch (it has no effect on a batch without a consistent trial). */
int ldc_fv_wide_batch_set_pressure_budget(ldc_fv_wide_batch *b, int budget);
/* 0, LDC_FV_E_NAN, or LDC_FV_WIDE_E_BUDGET when the last enqueue overflowed (wait for its stream first). */
int ldc_fv_wide_status(ldc_fv_wide *h);
/* n (1 .. LDC_FV_WIDE_BATCH_MAX) trials of any sizes and parameters, one device, advanced by the same launches.  `table` */
/* is a device buffer of table_len >= LDC_FV_WIDE_BATCH_TABLE_LEN bytes owned by the caller and left alone until destroy. */
/* Validation comes first and needs no device: LDC_E_ARG for a null list, n out of range or a null table; LDC_E_STATE for  */
/* a null handle; LDC_E_ARG for a handle listed twice, trials whose max_lin_iters differ and a short table; LDC_E_STATE    */
/* for handles of different devices.  Then the device: LDC_E_STATE when it is not the handles', and ONE synchronous copy   */
/* of the table on the library's own stream.  The batch keeps a copy of every trial's arguments and of its mixing block    */
/* (ldc_fv_wide_set_anderson: attach before create), not the handles: each                                                  */
/* trial may still be advanced and asked for its status through its own handle (one of the two in flight at a time).        */
int ldc_fv_wide_batch_create(ldc_fv_wide *const *hs, int n, void *table, int64_t table_len, ldc_fv_wide_batch **out);
int ldc_fv_wide_batch_destroy(ldc_fv_wide_batch *b);
/* n_iters[q] (0 .. rec_cap of trial q, at least one above 0) SIMPLE iterations of trial q with lin_budget (>= 1) BiCGSTAB */
/* iterations each: one launch that hands every trial its quota, then max(n_iters) iteration chains, every launch carrying */
/* the work-groups of all trials.  A trial stops at its quota, its latch, a NaN or ITS overflow (ldc_fv_wide_status of its  */
/* own handle tells which); a trial with quota 0 is not touched: u, v, p, mdot, rec and ctrl stay as they are.  LDC_E_STATE */
/* for a null batch, then LDC_E_ARG, then the device.                                                                       */
int ldc_fv_wide_batch_enqueue(ldc_fv_wide_batch *b, const int32_t *n_iters, int lin_budget, void *stream);
/* As ldc_fv_wide_set_graph: one linear hipGraph of the batch's iteration per budget value up to 64, captured on the        */
/* library's own stream and replayed on the caller's; destroy waits for the last replay.                                    */
int ldc_fv_wide_batch_set_graph(ldc_fv_wide_batch *b, int on);
/* Kernel launches of ONE iteration chain at that budget (an enqueue adds one): those of a lone trial, with the mixing      */
/* chain's when any trial of the batch has mixing attached.  Needs no device.                                               */
int ldc_fv_wide_batch_launches(const ldc_fv_wide_batch *b, int lin_budget);
/* omega, psi and the result block of ONE trial that is not in flight, by the whole chip: the launches of                  */
/* ldc_fv_wide_post_launches on `stream`, nothing synchronises.  `post` as for ldc_fv_post_enqueue; `scratch` is a device    */
/* buffer of scratch_len >= LDC_FV_WIDE_POST_SCRATCH_LEN(nx, ny) doubles owned by the caller.  Validation comes first and  */
/* needs no device: LDC_E_STATE for a null handle; LDC_E_ARG for a null post, a null pointer in it, a negative bound, a     */
/* null or short scratch; then LDC_E_NODEVICE, or LDC_E_STATE when the current device is not the handle's.                   */
int ldc_fv_wide_post_enqueue(ldc_fv_wide *h, const struct ldc_fv_post *post, double *scratch, int64_t scratch_len, void *stream);
/* Kernel launches of that chain (7).  Needs no device; LDC_E_ARG for a null handle. */
int ldc_fv_wide_post_launches(const ldc_fv_wide *h);
/* fine <- the prolongation of coarse (any two sizes of LDC_FV_MIN_N .. LDC_FV_WIDE_MAX_N, one domain, one device, neither  */
/* in flight): two launches on `stream`.  Written: the fine trial's u, v, p and mdot, nothing else.  Validation comes first */
/* and needs no device: LDC_E_STATE for a null handle; LDC_E_ARG for coarse == fine and for two domains (nx dx or ny dy      */
/* differ beyond 1e-12 relative); then LDC_E_NODEVICE, or LDC_E_STATE for a handle of another device.                        */
int ldc_fv_wide_prolong_enqueue(ldc_fv_wide *coarse, ldc_fv_wide *fine, void *stream);
/* n jobs (a host array; every pointer inside a job is a device pointer, nothing of it in flight elsewhere): U, V, P of   */
/* every job from its u, v, p as described above, LDC_FV_SAMPLE_LAUNCH_MAX jobs per launch, nothing synchronises.         */
/* Validation comes before any launch and needs no device: LDC_E_ARG for a null list or n < 1, for a null pointer in a    */
/* job, for nx or ny outside LDC_FV_MIN_N .. LDC_FV_WIDE_MAX_N, for Mx or My < 3 and for dx or dy <= 0; then               */
/* LDC_E_NODEVICE.  That x and y lie inside the source's domain is the caller's to see to (a node outside is              */
/* extrapolated from the last interval; no read leaves the source arrays).                                                */
int ldc_fv_sample_nodes(const struct ldc_fv_sample_job *jobs, int n, void *stream);
/* n jobs (a host array; every pointer inside a job is a device pointer, nothing of it in flight elsewhere): omega, psi and */
/* the result block of every job as described above, ldc_fv_wall_post_launches(n) launches on `stream`, nothing            */
/* synchronises.  Validation comes before any launch and needs no device: LDC_E_ARG for a null list or n < 1, for a null    */
/* pointer in a job, for nx or ny outside LDC_FV_MIN_N .. LDC_FV_WIDE_MAX_N, for dx or dy not > 0, for a bound outside      */
/* 0 .. nx (0 .. ny) and for refine other than 0 or 1; then LDC_E_NODEVICE.                                                 */
int ldc_fv_wall_post_enqueue(const struct ldc_fv_wall_job *jobs, int n, void *stream);
/* Kernel launches of that call: 7 per group of LDC_FV_WALL_LAUNCH_MAX jobs.  Needs no device; LDC_E_ARG for n < 1. */
int ldc_fv_wall_post_launches(int n);
/* The same for jobs on stretched tensor grids, as described above: ldc_fv_wall_stretched_post_launches(n) launches on      */
/* `stream`, nothing synchronises.  Validation comes before any launch and needs no device: LDC_E_ARG for a null list or     */
/* n < 1, for a null pointer in a job, for nx or ny outside LDC_FV_MIN_N .. LDC_FV_WIDE_MAX_N, for a bound outside 0 .. nx     */
/* (0 .. ny) and for refine other than 0 or 1; then LDC_E_NODEVICE.  The tables are the caller's to get right.               */
int ldc_fv_wall_stretched_post_enqueue(const struct ldc_fv_wall_stretched_job *jobs, int n, void *stream);
/* Kernel launches of that call: 7 per group of LDC_FV_WALL_STRETCHED_LAUNCH_MAX jobs.  Needs no device; LDC_E_ARG for n < 1. */
int ldc_fv_wall_stretched_post_launches(int n);
/* n jobs (a host array; every pointer inside a job is a device pointer, nothing of it in flight elsewhere): the fine u, v, p */
/* and mdot of every job from its coarse state as described above, ldc_fv_prolong_tables_launches(n) launches on `stream`,     */
/* one work-group of 512 threads per job, nothing synchronises.  Validation comes before any launch and needs no device:       */
/* LDC_E_ARG for a null list or n < 1, for a null pointer in a job, for a size outside LDC_FV_MIN_N .. LDC_FV_MAX_N, for Lx, Ly */
/* or rho not > 0, and for a fine u, v, p or mdot that is also another field of its job, a coarse field of any job of the call  */
/* or a fine field of another (what a launch writes nobody else in it may touch, however many launches the call takes); then    */
/* LDC_E_NODEVICE.  A refused call launches nothing.  Several jobs may share a coarse state and tables.  The tables are the     */
/* caller's to get right.                                                                                                      */
int ldc_fv_prolong_tables_enqueue(const struct ldc_fv_prolong_tables_job *jobs, int n, void *stream);
/* Kernel launches of that call: 1 per group of LDC_FV_PROLONG_TABLES_LAUNCH_MAX jobs.  Needs no device; LDC_E_ARG for n < 1. */
int ldc_fv_prolong_tables_launches(int n);
/* The same jobs over the whole chip: sizes LDC_FV_MIN_N .. LDC_FV_WIDE_MAX_N on both sides, ldc_fv_wide_prolong_tables_launches(n) */
/* launches on `stream`, two per job (LDC_FV_WIDE_GROUPS of the fine trial work-groups of 256 threads each), job after job,     */
/* nothing synchronises.  Validation is that of ldc_fv_prolong_tables_enqueue with the larger size bound, before any launch and  */
/* without a device: every refusal is LDC_E_ARG; then LDC_E_NODEVICE.  A refused call launches nothing.  The bits of a job are   */
/* those of ldc_fv_prolong_tables_enqueue wherever both take it.                                                               */
int ldc_fv_wide_prolong_tables_enqueue(const struct ldc_fv_prolong_tables_job *jobs, int n, void *stream);
/* Kernel launches of that call: LDC_FV_WIDE_PROLONG_TABLES_LAUNCHES per job.  Needs no device; LDC_E_ARG for n < 1. */
int ldc_fv_wide_prolong_tables_launches(int n);

#ifdef __cplusplus
}
#endif

#endif /* LDC_FV_H */
