// kf_hessian_mfma.hip — K6, the Hessian correction, with the GP sums on the
// matrix cores (kf_gp_mfma.h pixel_hessian_mfma): the two kernels of
// KF_HESSIAN_ROWS (kf_device.h) and their launch table, a translation unit of
// its own so they compile in parallel with the rest (_build.py).  Which launch
// takes one of them is hessian_plan's decision (kf_plan.h); the VALU kernel
// stays in kf_kernels.hip.
#include "kf_device.h"

namespace kf {

static const LaunchRow<HessianMfmaArgs> hessian_rows[] = {KF_HESSIAN_ROWS};

hipError_t dev_hessian_mfma(const KernelPlan& plan, const HessianMfmaArgs& a, hipStream_t s) {
  if (plan.family != PLAN_HESSIAN_MFMA || a.h.n_bands < 1 || a.h.n_bands > HESS_MAX_BANDS || a.h.N > a.h.ld)
    return hipErrorInvalidValue;
  if (a.h.N <= 0) return hipSuccess;
  for (const LaunchRow<HessianMfmaArgs>& r : hessian_rows) {
    if (!(r.plan == plan)) continue;
    hipLaunchKernelGGL(r.kernel, dim3(dev_grid(a.h.N)), dim3(plan.bs), 0, s, a);
    return hipGetLastError();
  }
  return hipErrorInvalidValue;
}

void launch_table_hessian(std::vector<KernelPlan>& out) { table_plans(hessian_rows, out); }

}  // namespace kf
