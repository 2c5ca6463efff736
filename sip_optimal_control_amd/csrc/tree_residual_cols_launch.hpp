// tree_residual_cols_launch.hpp -- the launcher of the KKT residual on the tree-native arenas, for one column and for
// several (tree_residual.hpp, instantiated in tree_residual_cols.hip, a translation unit of its own).  The refinement
// update is the chain's (residual_launch.hpp: launch_update_cols).  No kernel source in here: the host code
// (sip_lqr_tree.hip) includes this header and residual_launch.hpp alone.  The launch shape is host arithmetic in
// tree_residual_cols_shape.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "tree_generic.hpp"
#include "tree_residual_cols_shape.hpp"

namespace sipamd {
namespace residual {

// What one call is told.  `input` is the whole-batch input arena; rhs_cols (or nullptr: q, c, r of input for every
// column), sol_cols, res and scaled are [num_cols][batch][out_len] arrays (sip_lqr_tree_solve_multi's layout), norm and
// scale [num_cols][batch].
struct TreeColsArgs {
  long batch;
  const double *input, *rhs_cols, *sol_cols;
  // plain form (scaled == nullptr): res may be nullptr; scaled form: rho / s to scaled, s to scale
  double *res, *scaled, *scale, *norm;
};

// The columns go in groups of tree_cols_shape(dims, aligned, kTreeColsMax).columns, one launch per group, a short last
// group on the least instantiation that holds it; the single-column entry points pass num_cols = 1.  A staged plan
// whose `input` is not 16-byte aligned is served by the in-place instantiations.
hipError_t launch_tree_residual_cols(const tree::Meta &meta, const TreeColsDims &dims, const TreeColsArgs &a,
                                     int num_cols, hipStream_t stream);

} // namespace residual
} // namespace sipamd
