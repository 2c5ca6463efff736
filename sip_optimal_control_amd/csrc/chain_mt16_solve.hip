// chain_mt16_solve.hip -- instantiations of the separate sweeps of the n = 32 matrix-core chain kernels: the factor
// sweep (chain_factor_mt16, chain_mt16.hpp) and the solve sweep (chain_solve_mt16, chain_mt16_solve.hpp).  A translation
// unit of its own: compiled in parallel with the others, and the fused kernels of chain_mt16.hip keep the module --
// and with it the register allocation -- they were tuned in.
#include "chain_mt16_solve.hpp"
#include "mt16_launch.hpp"

namespace sipamd {

static_assert(mt16::Layout<float, 8>::WSN == kMt16SpillPerNode, "the spill the factor sweep left");
static_assert(mt16_col_workspace_scalars(3, 8, 5) == 4 * 5 * (mt16::N + 8), "cws[node][column][g | k]");

#define SIP_MT16_SOLVE_INSTANTIATE(S, M)                                                                     \
  template hipError_t launch_mt16_solve<S, M>(long, int, const void *, const void *, void *, void *, void *, \
                                              const void *, void *, const int32_t *, int, long, hipStream_t); \
  template hipError_t launch_mt16_factor<S, M>(long, int, const void *, void *, int32_t *, void *, void *, hipStream_t);
SIP_MT16_SOLVE_INSTANTIATE(float, 8)
SIP_MT16_SOLVE_INSTANTIATE(float, 4)
SIP_MT16_SOLVE_INSTANTIATE(double, 8)
SIP_MT16_SOLVE_INSTANTIATE(double, 4)

} // namespace sipamd
