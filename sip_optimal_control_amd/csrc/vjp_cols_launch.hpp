// vjp_cols_launch.hpp -- the launchers of the multi-column gradient kernel of the chain KKT solve (chain_vjp_cols.hpp,
// instantiated in chain_vjp_cols.hip, a translation unit of its own).  No kernel source in here: the host code
// (sip_lqr_amd.hip) includes this header and vjp_cols_shape.hpp alone.
#pragma once
#include <hip/hip_runtime.h>

#include "vjp_cols_shape.hpp"
#include "vjp_launch.hpp" // Args: here sol and adj are column arrays, column c at c * batch * vecs_len scalars

namespace sipamd {
namespace vjp {

// grad = the sum over the num_rhs columns of the single kernel's gradient (num_rhs = 0: zeros).  The columns go in
// groups of cols_per_launch (or of SIP_LQR_VJP_MULTI_COLUMNS, where that is less), one launch per group; the groups
// after the first accumulate onto what grad holds.  hipErrorInvalidValue where nothing fits (cols_shape).
hipError_t launch_vjp_cols(const Args &a, int num_rhs, hipStream_t stream);

// vec[c][p] = 0 (`len` scalars per problem, column c at c * batch * len) where status[p] != SIP_LQR_SUCCESS
hipError_t launch_mask_cols(int num_rhs, long batch, long len, bool f32, const int32_t *status, void *vec,
                            hipStream_t stream);

} // namespace vjp
} // namespace sipamd
