// kf_gain10.hip — gain-form (K1g) instantiations for 10-parameter states
// (PROSAIL / SAIL, the multi-sensor state): the global-table matrix-core
// kernel and the VALU kernels, a translation unit of its own so they compile
// in parallel with the rest (_build.py).
#include "kf_device.h"

namespace kf {

hipError_t dev_gain_np10(const GainArgs& a, int grid, hipStream_t s) {
  l_gain<10>(a, grid, s);
  return hipGetLastError();
}

}  // namespace kf
