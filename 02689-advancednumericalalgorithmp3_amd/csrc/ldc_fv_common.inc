// ldc_fv_common.inc -- what all translation units of the finite-volume solver share (include/ldc_fv.h):
// ldc_kernels.hip (through ldc_fv_kernel.inc, the SIMPLE iteration with one trial per CU), ldc_fv_wide.hip (the same
// iteration by the whole chip), ldc_fv_post.hip (streamfunction and vortex metrics), ldc_fv_prolong.hip (coarse-to-fine
// transfer of the state), ldc_fv_anderson.hip (Anderson mixing), ldc_fv_cu_pressure.hip (the one-CU iteration with the
// consistent pressure equation), ldc_fv_stretched.hip (the one-CU iteration on a wall-clustered grid) and
// ldc_fv_stretched_sep.hip (the same with the separable scaled preconditioner).
// Types, constants and host-side helpers (the fill of a descriptor, as_stream) only, no device function: each unit's
// code object holds what that unit needs and depends on no other's.  The device functions that two mappings share are
// in ldc_fv_cells.inc (the SIMPLE iteration), ldc_fv_post_cells.inc, ldc_fv_prolong_cells.inc and
// ldc_fv_anderson_cells.inc, each included only by the units that call it.
#ifndef LDC_FV_COMMON_INC
#define LDC_FV_COMMON_INC

#include "ldc_hip.h"
#include "ldc_fv.h"

typedef double v4d __attribute__((ext_vector_type(4)));

#define MFMA_F64(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)

namespace {

constexpr int kFvThreads = 512;
constexpr int kFvWaves = kFvThreads / 64;

// work vectors (n doubles each), in the order of LDC_FV_NWORK
enum FvVec {
  FV_GPX, FV_GPY, FV_AP, FV_AW, FV_AE, FV_AS, FV_AN,
  FV_XU, FV_XV, FV_RU, FV_RV, FV_RTU, FV_RTV, FV_PU, FV_PV, FV_VU, FV_VV,
  FV_PHU, FV_PHV, FV_SHU, FV_SHV, FV_TU, FV_TV,
  FV_C, FV_W1, FV_W2, FV_Y, FV_UP, FV_VP, FV_OMEGA, FV_BU, FV_BV,
  FV_NVEC
};
static_assert(FV_NVEC == LDC_FV_NWORK, "work vectors");

// the trial's device-side descriptor: the first bytes of the slot in the tail of its work buffer
struct FvDesc {
  int nx, ny, scheme, rec_cap, warmup, maxit;
  double dx, dy, rho, mu, alpha_uv, alpha_p, lin_tol, tol, lid;
  const double *ulid, *Qx, *lamx, *Qy, *lamy;
  double *u, *v, *p, *mdot, *work, *rec;
  long long *ctrl;
};
static_assert(sizeof(FvDesc) <= LDC_FV_DESC_DOUBLES * sizeof(double), "descriptor slot");

// The descriptor slot (LDC_FV_DESC_DOUBLES doubles = 512 bytes in the tail of `work`), byte by byte:
//     0 .. 255  FvDesc (ldc_fv_create; it travels by value in the 256-byte table entry of a shared batch: it must not grow)
//   256 .. 327  the post block (ldc_fv_post.hip, kFvPostOffset)
//   328 .. 343  the grid block of a one-CU trial on a stretched grid (FvGridBlk below; ldc_fv_set_grid)
//   344 .. 359  the preconditioner block of such a trial (FvPrecondBlk below; ldc_fv_set_preconditioner)
//   384 .. 407  the pressure block of a one-CU trial (FvCuPcg below; ldc_fv_set_pressure)
//   448 .. 511  the mixing kernel's kept record row (ldc_fv_anderson.hip, kFvAaKeepOffset)
// The consistent pressure equation of a one-CU trial (ldc_fv_cu_pressure.hip): tolerance, cap, mode and the caller's four
// statistics words, written by ldc_fv_set_pressure with the synchronous copy of ldc_fv_create.
struct FvCuPcg {
  double tol;
  int max_iters, mode;
  long long* stats;
};
constexpr int kFvCuPcgOffset = 384;
static_assert(sizeof(FvDesc) <= 256, "the pressure block is clear of the descriptor");
static_assert(kFvCuPcgOffset >= 256 + 72, "the pressure block is clear of the post block (ldc_fv_post.hip: 72 bytes at 256)");
static_assert(kFvCuPcgOffset + sizeof(FvCuPcg) <= (LDC_FV_DESC_DOUBLES - LDC_FV_REC_LEN) * sizeof(double),
              "the pressure block is clear of the mixing kernel's kept row");

// The per-axis geometry tables of a one-CU trial on a stretched grid (ldc_fv_stretched.hip), written by ldc_fv_set_grid with the
// synchronous copy of ldc_fv_create: per axis [h (n) | d (n + 1) | g (n + 1)] (include/ldc_fv.h).
struct FvGridBlk {
  const double *ax, *ay;
};
constexpr int kFvGridOffset = 328;
static_assert(kFvGridOffset >= 256 + 72 && kFvGridOffset + sizeof(FvGridBlk) <= kFvCuPcgOffset,
              "the grid block is clear of the post block and of the pressure block");

// The per-axis tables of the separable scaled preconditioner of such a trial (ldc_fv_stretched_sep.hip), written by
// ldc_fv_set_preconditioner with the same copy: per axis [a (n) | lam (n) | Q (n x n)] (include/ldc_fv.h).
struct FvPrecondBlk {
  const double *px, *py;
};
constexpr int kFvPrecondOffset = 344;
static_assert(kFvPrecondOffset >= kFvGridOffset + (int)sizeof(FvGridBlk) && kFvPrecondOffset + sizeof(FvPrecondBlk) <= kFvCuPcgOffset,
              "the preconditioner block is clear of the grid block and of the pressure block");

// host: the caller's stream handle of the C ABI
inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// host: validate `pr` (not null) for a mapping that takes grids up to max_n x max_n and fill the descriptor from it.
// 0 or LDC_E_ARG; needs no device.
inline int fv_desc_of(const struct ldc_fv_problem* pr, int max_n, FvDesc* h) {
  if (pr->nx < LDC_FV_MIN_N || pr->nx > max_n || pr->ny < LDC_FV_MIN_N || pr->ny > max_n) return LDC_E_ARG;
  if (pr->scheme != 0 && pr->scheme != 1) return LDC_E_ARG;
  if (pr->rec_cap < 1 || pr->warmup < 0 || pr->max_lin_iters < 1) return LDC_E_ARG;
  if (!(pr->dx > 0) || !(pr->dy > 0) || !(pr->rho > 0) || !(pr->mu > 0)) return LDC_E_ARG;
  if (!(pr->alpha_uv > 0 && pr->alpha_uv <= 1) || !(pr->alpha_p > 0 && pr->alpha_p <= 1)) return LDC_E_ARG;
  if (!(pr->lin_tol > 0) || !(pr->tol >= 0)) return LDC_E_ARG;
  const void* req[] = {pr->ulid, pr->Qx, pr->lamx, pr->Qy, pr->lamy, pr->u, pr->v, pr->p, pr->mdot, pr->work,
                       pr->rec, pr->ctrl};
  for (const void* q : req) if (!q) return LDC_E_ARG;
  h->nx = pr->nx; h->ny = pr->ny; h->scheme = pr->scheme; h->rec_cap = pr->rec_cap; h->warmup = pr->warmup;
  h->maxit = pr->max_lin_iters;
  h->dx = pr->dx; h->dy = pr->dy; h->rho = pr->rho; h->mu = pr->mu; h->alpha_uv = pr->alpha_uv; h->alpha_p = pr->alpha_p;
  h->lin_tol = pr->lin_tol; h->tol = pr->tol; h->lid = pr->lid_velocity;
  h->ulid = pr->ulid; h->Qx = pr->Qx; h->lamx = pr->lamx; h->Qy = pr->Qy; h->lamy = pr->lamy;
  h->u = pr->u; h->v = pr->v; h->p = pr->p; h->mdot = pr->mdot; h->work = pr->work; h->rec = pr->rec;
  h->ctrl = reinterpret_cast<long long*>(pr->ctrl);
  return 0;
}

}  // namespace

struct ldc_fv {
  FvDesc* dev;              // the descriptor in the tail of the trial's work buffer
  long long* ctrl;
  int rec_cap;
  int device;
  int nx, ny;               // (host-side copies for validation: ldc_fv_prolong_enqueue)
  double dx, dy;
  int pressure_mode;        // LDC_FV_PRESSURE_*: the kernel that advances the trial (ldc_fv_set_pressure)
  int grid_mode;            // LDC_FV_GRID_*: tables attached (ldc_fv_set_grid): fv_stretched_kernel advances the trial
  int precond_mode;         // LDC_FV_PRECOND_*: tables attached (ldc_fv_set_preconditioner): fv_stretched_sep_kernel does
};

// host: consistent handles (pressure_mode LDC_FV_PRESSURE_CONSISTENT) of the CURRENT device go to fv_cu_pressure_kernel,
// LDC_FV_LAUNCH_MAX per launch (ldc_fv_cu_pressure.hip; called by ldc_fv_enqueue and ldc_fv_batch_enqueue only)
__attribute__((visibility("hidden"))) int ldc_fv_cu_pressure_launch(ldc_fv* const* hs, int n, int n_iters, void* stream);

// host: handles with geometry tables (grid_mode LDC_FV_GRID_TABLES) of the CURRENT device, all in the pressure mode
// `consistent` says, go to fv_stretched_kernel, LDC_FV_LAUNCH_MAX per launch (ldc_fv_stretched.hip; called by ldc_fv_enqueue and
// ldc_fv_batch_enqueue only)
__attribute__((visibility("hidden"))) int ldc_fv_stretched_launch(ldc_fv* const* hs, int n, int n_iters, int consistent, void* stream);

// host: consistent handles with geometry tables and the separable preconditioner (precond_mode LDC_FV_PRECOND_SEPARABLE) of
// the CURRENT device go to fv_stretched_sep_kernel, LDC_FV_LAUNCH_MAX per launch (ldc_fv_stretched_sep.hip; called by
// ldc_fv_enqueue and ldc_fv_batch_enqueue only)
__attribute__((visibility("hidden"))) int ldc_fv_stretched_sep_launch(ldc_fv* const* hs, int n, int n_iters, void* stream);

#endif  // LDC_FV_COMMON_INC
