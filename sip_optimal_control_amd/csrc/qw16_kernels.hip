// qw16_kernels.hip -- one slice (-DSIP_QW16_SLICE=<s>) of the fused fp64 chain kernels: every shape n <= 16,
// m <= 8 runs on an exact instantiation, each with its multi-right-hand-side solve and, where it has one, its
// split form (A | B read where the model callback left them: sip_lqr_factor_solve_split).  Which entries a
// slice holds is generated (gen_qw16_kernels.py -> qw16_kernels_gen.hpp); the slices compile in parallel.
#include "qw16_launch.hpp"

#ifndef SIP_QW16_SLICE
#error "compile with -DSIP_QW16_SLICE=<slice number>"
#endif
#define SIP_CAT2(a, b) a##b
#define SIP_CAT(a, b) SIP_CAT2(a, b)

namespace sipamd {
namespace {
const KernelEntry kSlice[] = {SIP_CAT(QW16_SLICE_ENTRIES_, SIP_QW16_SLICE)};
}
const KernelEntry *SIP_CAT(qw16_slice_, SIP_QW16_SLICE)(int *count) {
  *count = (int)(sizeof(kSlice) / sizeof(kSlice[0]));
  return kSlice;
}
} // namespace sipamd
