// kkt_chain_kernels.hip -- the rows of the Newton-KKT chain kernel table (kkt_chain_launch.hpp) and so every
// instantiation of the chain kernels.  -DSIP_KKT_CHAIN_N=0: the generic row; =<n>: the rows of the benchmark family's
// state dimension n.  The library is built from one unit per value, compiled in parallel; without the define all rows
// are in one unit (tools/kkt_ab_build.sh, tools/diag_build.sh).
#define SIP_KKT_CHAIN_UNIT
#include "kkt_chain_launch.hpp"

namespace sipamd {
namespace kkt {

template <int N, int M>
const KktChainKernels kkt_chain_row = {N, M, &condense_chain_kernel<true, true, N, M>,
                                       &condense_chain_kernel<false, true, N, M>, &condense_chain_kernel<true, false, N, M>,
                                       &condense_chain_pipe_kernel<true, N, M>, &condense_chain_pipe_kernel<false, N, M>,
                                       &recover_chain_kernel<false, N, M>, &recover_chain_kernel<true, N, M>,
                                       &apply_chain_kernel<N, M>, &apply_theta_chain_kernel<N, M>,
                                       &theta_rhs_chain_kernel<N, M>, &theta_recover_chain_kernel<N, M>,
                                       &theta_dot_chain_kernel<N, M>};

#define SIP_KKT_CHAIN_ROW(N, M) template const KktChainKernels kkt_chain_row<N, M>;
#define SIP_KKT_CHAIN_ROWS(N) SIP_KKT_FAMILY_SHAPES(SIP_KKT_CHAIN_ROW, N)
#if !defined(SIP_KKT_CHAIN_N)
SIP_KKT_CHAIN_ROW(0, 0) SIP_KKT_FAMILY_N(SIP_KKT_CHAIN_ROWS)
#elif SIP_KKT_CHAIN_N == 0
SIP_KKT_CHAIN_ROW(0, 0)
#else
SIP_KKT_CHAIN_ROWS(SIP_KKT_CHAIN_N)
#endif

} // namespace kkt
} // namespace sipamd

#ifdef SIP_KKT_STAMPS
// diagnostic build: read (and clear) the per-segment cycle sums of condense_chain_pipe_kernel (tools/kkt_stamps.py)
extern "C" void sip_kkt_debug_segments(unsigned long long *out16) {
  (void)hipDeviceSynchronize();
  (void)hipMemcpyFromSymbol(out16, HIP_SYMBOL(sipamd::kkt::g_kkt_seg), 16 * sizeof(unsigned long long));
  unsigned long long zero[16] = {0};
  (void)hipMemcpyToSymbol(HIP_SYMBOL(sipamd::kkt::g_kkt_seg), zero, sizeof(zero));
}
#endif
