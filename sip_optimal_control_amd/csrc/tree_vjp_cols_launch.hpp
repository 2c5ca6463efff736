// tree_vjp_cols_launch.hpp -- the launcher of the multi-column gradient kernel of the tree KKT solve
// (tree_vjp_cols.hpp, instantiated in tree_vjp_cols.hip, a translation unit of its own).  No kernel source in here: the
// host code (sip_lqr_tree.hip) includes this header and tree_vjp_cols_shape.hpp alone.
#pragma once
#include <hip/hip_runtime.h>

#include "tree_vjp_cols_shape.hpp"
#include "tree_vjp_launch.hpp" // Args: here sol and adj are column arrays, column c at c * batch * out_len doubles

namespace sipamd {
namespace tree_vjp {

// grad = the sum over the num_rhs columns of the single kernel's gradient off the copy entries, +0.0 on them
// (num_rhs = 0: zeros).  The columns go in groups of cols_per_launch (SIP_LQR_TREE_VJP_MULTI_COLUMNS on top), one
// launch per group; the groups after the first accumulate onto what grad holds.  An empty input arena launches
// nothing.  The measuring aids are read per call.
hipError_t launch_tree_vjp_cols(const Args &a, int num_rhs, hipStream_t stream);

} // namespace tree_vjp
} // namespace sipamd
