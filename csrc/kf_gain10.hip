// kf_gain10.hip — gain-form (K1g) instantiations for 10-parameter states
// (PROSAIL / SAIL, the multi-sensor state): the global-table matrix-core
// kernel and the VALU kernels, a translation unit of its own so they compile
// in parallel with the rest (_build.py).
#include "kf_device.h"

namespace kf {

static const LaunchRow<GainArgs> k1g_rows[] = {KF_K1G_ROWS_10};

hipError_t dev_gain_np10(const GainArgs& a, int grid, hipStream_t s) {
  return launch_plan(k1g_rows, gain_plan(10, a), a, grid, s);
}

void launch_table_gain_np10(std::vector<KernelPlan>& out) { table_plans(k1g_rows, out); }

}  // namespace kf
