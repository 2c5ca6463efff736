// chain_qf32.hip -- instantiations of the fused fp32 chain kernel (chain_qf32.hpp): the rows of qf32_launch.hpp.
#include "chain_qf32.hpp"

namespace sipamd {
namespace qf32 {

template <int N, int M>
hipError_t launch_qf32(long batch, int T, const void *mats, const void *vecs, void *sol, void *gains, int32_t *status,
                       void *ws, hipStream_t stream, int /*mode: always the full sweep*/, void * /*gfac*/) {
  hipLaunchKernelGGL((chain_factor_solve_qf32<N, M>), dim3((unsigned)((batch + 3) / 4)), dim3(64), 0, stream,
                     (const float *)mats, (const float *)vecs, (float *)sol, (float *)gains, (float *)ws,
                     (int *)status, batch, T);
  return hipGetLastError();
}

#define SIP_QF32_INSTANTIATE(N, M)                                                                           \
  template hipError_t launch_qf32<N, M>(long, int, const void *, const void *, void *, void *, int32_t *,    \
                                        void *, hipStream_t, int, void *);
SIP_QF32_ROWS(SIP_QF32_INSTANTIATE)

} // namespace qf32
} // namespace sipamd
