// ldc_fv_common.inc -- what the translation units of the finite-volume solver share (include/ldc_fv.h):
// ldc_kernels.hip (through ldc_fv_kernel.inc, the SIMPLE iteration), ldc_fv_post.hip (streamfunction and vortex
// metrics), ldc_fv_prolong.hip (coarse-to-fine transfer of the state) and ldc_fv_anderson.hip (Anderson mixing).  Types and constants only: each unit keeps its own device functions, so neither unit's code object
// depends on the other's.
#ifndef LDC_FV_COMMON_INC
#define LDC_FV_COMMON_INC

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

}  // namespace

struct ldc_fv {
  FvDesc* dev;              // the descriptor in the tail of the trial's work buffer
  long long* ctrl;
  int rec_cap;
  int device;
  int nx, ny;               // (host-side copies for validation: ldc_fv_prolong_enqueue)
  double dx, dy;
};

#endif  // LDC_FV_COMMON_INC
