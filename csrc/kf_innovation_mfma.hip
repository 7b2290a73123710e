// kf_innovation_mfma.hip — the innovation check with the GP bands on the matrix
// cores (kf_gp_mfma.h pixel_innovation_mfma): the four kernels of
// KF_INNOV_ROWS (kf_device.h) and their launch table, a translation unit of its
// own so they compile in parallel with the rest (_build.py).  Which launch
// takes one of them is innovation_plan's decision (kf_plan.h); the VALU kernel
// stays in kf_kernels.hip.  The four kernels of KF_INNOV_PROP_ROWS (the check
// at the fused forecast, pixel_innovation_prop) have a table of their own here.
#include "kf_device.h"

namespace kf {

static const LaunchRow<InnovationArgs> innov_rows[] = {KF_INNOV_ROWS};
static const LaunchRow<InnovationArgs> innov_prop_rows[] = {KF_INNOV_PROP_ROWS};

hipError_t dev_innovation_mfma(const KernelPlan& plan, const InnovationArgs& a, int grid, hipStream_t s) {
  return launch_plan(innov_rows, plan, a, grid, s);
}

hipError_t dev_innovation_prop(const KernelPlan& plan, const InnovationArgs& a, int grid, hipStream_t s) {
  return a.prop ? launch_plan(innov_prop_rows, plan, a, grid, s) : hipErrorInvalidValue;
}

void launch_table_innovation(std::vector<KernelPlan>& out) { table_plans(innov_rows, out); }
void launch_table_innovation_prop(std::vector<KernelPlan>& out) { table_plans(innov_prop_rows, out); }

}  // namespace kf
