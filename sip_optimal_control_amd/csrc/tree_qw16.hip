// tree_qw16.hip -- size classes of the fused tree kernel (tree_qw16.hpp) and their launcher; its
// own translation unit so that it compiles beside the others.
#include "tree_qw16_launch.hpp"

#include "tree_qw16.hpp"
#include "tree_mrhs_qw16.hpp"

namespace sipamd {

namespace {
template <int N, int M, bool EXPORT>
hipError_t launch(const TreeSchedule &ts, const double *input, double *output, double *work, double *pgains,
                  double *spill, int32_t *status, long batch, hipStream_t s) {
  if (EXPORT && work == nullptr)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL((tree_factor_solve_qw16<N, M, EXPORT>), dim3((unsigned)((batch + 3) / 4)), dim3(64), 0, s, ts,
                     input, output, work, pgains, spill, (int *)status, batch);
  return hipGetLastError();
}
// columns per wavefront of the multi-rhs solve: 8 as in chain_mrhs.hpp; 4 from 12 states on, where a step's
// operands (rows of W, A, V, K and both triangles of L, 5 N + 3 M doubles per lane) leave less room for columns
template <int N, int M>
constexpr int kMultiCols = N <= 10 ? 8 : 4;
template <int N, int M>
hipError_t launch_multi(const TreeSchedule &ts, const double *input, const double *work, const double *rhs_cols,
                        double *out_cols, double *cols, const int32_t *status, long batch, int num_rhs, hipStream_t s) {
  constexpr int P = kMultiCols<N, M>;
  hipLaunchKernelGGL((tree_solve_mrhs_qw16<N, M, P>), dim3((unsigned)((batch + 3) / 4), (unsigned)((num_rhs + P - 1) / P)),
                     dim3(64), 0, s, ts, input, work, rhs_cols, out_cols, cols, (const int *)status, batch, num_rhs);
  return hipGetLastError();
}
// the factorization alone, every factor-state field into the work arena (tree_factor_qw16: sip_lqr_tree_factor_fused)
template <int N, int M>
hipError_t launch_factor(const TreeSchedule &ts, const double *input, double *work, double *pgains, double *spill,
                         int32_t *status, long batch, hipStream_t s) {
  hipLaunchKernelGGL((tree_factor_solve_qw16<N, M, true, true>), dim3((unsigned)((batch + 3) / 4)), dim3(64), 0, s, ts,
                     input, (double *)nullptr, work, pgains, spill, (int *)status, batch);
  return hipGetLastError();
}
// one right-hand side against the factor state of the work arena, v and k into it (tree_solve_qw16:
// sip_lqr_tree_solve_fused)
template <int N, int M>
hipError_t launch_solve(const TreeSchedule &ts, const double *input, double *work, double *output,
                        const int32_t *status, long batch, hipStream_t s) {
  hipLaunchKernelGGL((tree_solve_mrhs_qw16<N, M, 1, true>), dim3((unsigned)((batch + 3) / 4)), dim3(64), 0, s, ts, input,
                     (const double *)work, input, output, work, (const int *)status, batch, 1);
  return hipGetLastError();
}
template <int N, int M>
long cols_len(const TreeSchedule &ts) {
  return TreeColLayout<N, M>::len(ts);
}
#define TREE_CLASS(N, M)                                                                                            \
  {N, M, TreeLayout<N, M>::GAIN, TreeLayout<N, M>::WS,                                                              \
   "tree_factor_solve_qw16<" #N "," #M ">/f64", &launch<N, M, false>, &launch<N, M, true>,                          \
   "tree_solve_mrhs_qw16<" #N "," #M ">/f64", &launch_multi<N, M>, &cols_len<N, M>,                                  \
   "tree_factor_qw16<" #N "," #M ">/f64 + tree_solve_qw16<" #N "," #M ">/f64", &launch_factor<N, M>, &launch_solve<N, M>}
// sorted by cost: the first class that holds the largest node and the largest control wins
// ((9, 3): the reference's variable-shape benchmark family at base dimension 8 -- states 7..9, controls 1..3,
// benchmarks/lqr_benchmark.cpp:209-310 -- padded to (10, 4) before round 3)
const TreeClass kClasses[] = {TREE_CLASS(4, 2),  TREE_CLASS(6, 3),  TREE_CLASS(8, 4),  TREE_CLASS(9, 3), TREE_CLASS(10, 4),
                              TREE_CLASS(12, 4), TREE_CLASS(15, 4), TREE_CLASS(15, 8)};
#undef TREE_CLASS
} // namespace

const TreeClass *find_tree_class(int max_n, int max_m) {
  for (const TreeClass &k : kClasses)
    if (k.n >= max_n && k.m >= max_m)
      return &k;
  return nullptr;
}

} // namespace sipamd

#ifdef SIP_TREE_STAMPS
// diagnostic build: read (and clear) the per-segment cycle sums of tree_factor_solve_qw16 (tools/tree_stamps.py)
extern "C" void sip_lqr_tree_debug_segments(unsigned long long *out8) {
  (void)hipDeviceSynchronize();
  (void)hipMemcpyFromSymbol(out8, HIP_SYMBOL(sipamd::g_tree_seg), 8 * sizeof(unsigned long long));
  unsigned long long zero[8] = {0};
  (void)hipMemcpyToSymbol(HIP_SYMBOL(sipamd::g_tree_seg), zero, sizeof(zero));
}
#endif
