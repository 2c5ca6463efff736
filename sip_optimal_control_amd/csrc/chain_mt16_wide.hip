// chain_mt16_wide.hip -- the fused n = 32 matrix-core chain kernel (chain_mt16.hpp) for control dimensions 12 and 16:
// the rows of sip_lqr_plan_set_wide_controls.  A translation unit of its own: compiled in parallel with the others,
// and the tuned m = 4 and m = 8 kernels of chain_mt16.hip keep the module they were tuned in.
#include "chain_mt16.hpp"
#include "mt16_launch.hpp"

namespace sipamd {

static_assert(mt16::Layout<float, 16>::WSN == kMt16SpillPerNode && mt16::Layout<double, 12>::WSN == kMt16SpillPerNode,
              "the dispatch table sizes the workspace by kMt16SpillPerNode");
static_assert(mt16::Layout<double, 12>::VM == 3 && mt16::Layout<float, 16>::VM == 4, "control registers per lane");

#define SIP_MT16_WIDE_INSTANTIATE(S, M)                                                                      \
  template hipError_t launch_mt16<S, M>(long, int, const void *, const void *, void *, void *, int32_t *,    \
                                        void *, hipStream_t, int, void *);
SIP_MT16_WIDE_INSTANTIATE(float, 16)
SIP_MT16_WIDE_INSTANTIATE(float, 12)
SIP_MT16_WIDE_INSTANTIATE(double, 16)
SIP_MT16_WIDE_INSTANTIATE(double, 12)

} // namespace sipamd
