// chain_mt16.hip -- instantiations of the n = 32 matrix-core chain kernel (chain_mt16.hpp).
#include "chain_mt16.hpp"
#include "mt16_launch.hpp"

namespace sipamd {

static_assert(mt16::Layout<float, 8>::WSN == kMt16SpillPerNode && mt16::Layout<double, 4>::WSN == kMt16SpillPerNode,
              "the dispatch table sizes the workspace by kMt16SpillPerNode");

#define SIP_MT16_INSTANTIATE(S, M)                                                                           \
  template hipError_t launch_mt16<S, M>(long, int, const void *, const void *, void *, void *, int32_t *,    \
                                        void *, hipStream_t, int, void *);
SIP_MT16_INSTANTIATE(float, 8)
SIP_MT16_INSTANTIATE(float, 4)
SIP_MT16_INSTANTIATE(double, 8)
SIP_MT16_INSTANTIATE(double, 4)

} // namespace sipamd
