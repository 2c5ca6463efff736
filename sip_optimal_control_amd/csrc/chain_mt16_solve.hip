// chain_mt16_solve.hip -- instantiations of the separate sweeps of the n = 32 matrix-core chain kernels: the factor
// sweep (chain_factor_mt16, chain_mt16.hpp) and the solve sweep (chain_solve_mt16, chain_mt16_solve.hpp).  A translation
// unit of its own: compiled in parallel with the others, and the fused kernels of chain_mt16.hip keep the module --
// and with it the register allocation -- they were tuned in.
#include "chain_mt16_solve.hpp"
#include "mt16_launch.hpp"

namespace sipamd {

template <typename S, int M>
hipError_t launch_mt16_solve(long batch, int T, const void *mats, const void *vecs_cols, void *sol_cols, void *gains,
                             void *ws, const void *gfac, void *cws, const int32_t *status, int ncols, long col_stride,
                             hipStream_t stream) {
  if (ncols < 1 || ncols > kMt16SolveColumns || (cws == nullptr && ncols != 1))
    return hipErrorInvalidValue;
  // 16-byte loads of the stage blocks (fp32, even m) and of the W dump: bases must be 16-byte aligned
  if (((uintptr_t)mats | (uintptr_t)ws) & 15)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL((mt16::chain_solve_mt16<S, M>), dim3((unsigned)batch), dim3(64), 0, stream, (const S *)mats,
                     (const S *)vecs_cols, (S *)sol_cols, (S *)gains, (S *)ws, (const S *)gfac, (S *)cws,
                     (const int *)status, batch, T, ncols, col_stride);
  return hipGetLastError();
}

template <typename S, int M>
hipError_t launch_mt16_factor(long batch, int T, const void *mats, void *gains, int32_t *status, void *ws, void *gfac,
                              hipStream_t stream) {
  if (((uintptr_t)mats | (uintptr_t)ws) & 15)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL((mt16::chain_factor_mt16<S, M>), dim3((unsigned)batch), dim3(64), 0, stream, (const S *)mats,
                     (S *)gains, (S *)ws, (S *)gfac, (int *)status, batch, T);
  return hipGetLastError();
}

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
