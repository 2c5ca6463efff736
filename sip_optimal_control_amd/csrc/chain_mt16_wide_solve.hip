// chain_mt16_wide_solve.hip -- the separate sweeps of the n = 32 matrix-core chain kernels for control dimensions 12
// and 16 (the rows of sip_lqr_plan_set_wide_controls): the factor sweep (chain_factor_mt16, chain_mt16.hpp) and the
// solve sweep (chain_solve_mt16, chain_mt16_solve.hpp).  A translation unit of its own, as chain_mt16_solve.hip is.
#include "chain_mt16_solve.hpp"
#include "mt16_launch.hpp"

namespace sipamd {

static_assert(mt16::Layout<float, 16>::WSN == kMt16SpillPerNode, "the spill the factor sweep left");
static_assert(mt16_col_workspace_scalars(3, 16, 5) == 4 * 5 * (mt16::N + 16), "cws[node][column][g | k]");

#define SIP_MT16_WIDE_SOLVE_INSTANTIATE(S, M)                                                                \
  template hipError_t launch_mt16_solve<S, M>(long, int, const void *, const void *, void *, void *, void *, \
                                              const void *, void *, const int32_t *, int, long, hipStream_t); \
  template hipError_t launch_mt16_factor<S, M>(long, int, const void *, void *, int32_t *, void *, void *, hipStream_t);
SIP_MT16_WIDE_SOLVE_INSTANTIATE(float, 16)
SIP_MT16_WIDE_SOLVE_INSTANTIATE(float, 12)
SIP_MT16_WIDE_SOLVE_INSTANTIATE(double, 16)
SIP_MT16_WIDE_SOLVE_INSTANTIATE(double, 12)

} // namespace sipamd
