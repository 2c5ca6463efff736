// chain_qf32_sweeps.hip -- instantiations of the separate sweeps of the fused fp32 chain kernel
// (chain_qf32_sweeps.hpp: chain_factor_qf32, chain_solve_cols_qf32), one pair per row of qf32_launch.hpp.  A translation
// unit of its own: compiled in parallel with the others, and the fused kernels of chain_qf32.hip keep their module.
#include "chain_qf32_sweeps.hpp"

namespace sipamd {
namespace qf32 {

template <int N, int M>
hipError_t launch_qf32_factor(long batch, int T, const void *mats, void *gains, int32_t *status, void *ws, void *gfac,
                              hipStream_t stream) {
  hipLaunchKernelGGL((chain_factor_qf32<N, M>), dim3((unsigned)((batch + 3) / 4)), dim3(64), 0, stream,
                     (const float *)mats, (float *)gains, (float *)ws, (float *)gfac, (int *)status, batch, T);
  return hipGetLastError();
}

template <int N, int M>
hipError_t launch_qf32_solve(long batch, int T, const void *mats, const void *vecs_cols, void *sol_cols, void *gains,
                             void *ws, const void *gfac, void *cws, const int32_t *status, int ncols, long col_stride,
                             hipStream_t stream) {
  if (ncols < 1 || ncols > kQf32SolveColumns || (cws == nullptr && ncols != 1))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL((chain_solve_cols_qf32<N, M, kQf32SolveColumns>), dim3((unsigned)((batch + 3) / 4)), dim3(64), 0,
                     stream, (const float *)mats, (const float *)vecs_cols, (float *)sol_cols, (float *)gains,
                     (float *)ws, (const float *)gfac, (float *)cws, (const int *)status, batch, T, ncols, col_stride);
  return hipGetLastError();
}

static_assert(qf32_col_workspace_scalars(3, 12, 4, 5) == 4 * 5 * (2 * 12 + 4), "cws[node][column][g | h | k]");

#define SIP_QF32_SWEEPS_INSTANTIATE(N, M)                                                                           \
  template hipError_t launch_qf32_factor<N, M>(long, int, const void *, void *, int32_t *, void *, void *, hipStream_t); \
  template hipError_t launch_qf32_solve<N, M>(long, int, const void *, const void *, void *, void *, void *,        \
                                              const void *, void *, const int32_t *, int, long, hipStream_t);
SIP_QF32_ROWS(SIP_QF32_SWEEPS_INSTANTIATE)

} // namespace qf32
} // namespace sipamd
