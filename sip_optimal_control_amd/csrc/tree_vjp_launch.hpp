// tree_vjp_launch.hpp -- the launcher of the gradient kernel of the tree KKT solve (tree_vjp.hpp, instantiated in
// tree_vjp.hip, a translation unit of its own).  No kernel source in here: the host code (sip_lqr_tree.hip) includes
// this header and tree_vjp_table.hpp alone.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "tree_vjp_table.hpp"

namespace sipamd {
namespace tree_vjp {

// What one launch is told.  Buffers are whole-batch device pointers: sol and adj in the output arena's layout, grad in
// the input arena's; table: the plan's in_len words on the device.
struct Args {
  long batch, in_len, out_len;
  const Word *table;
  const double *sol, *adj;
  const int32_t *status; // nullptr, or per problem: != 0 gets zeros
  double *grad;
};

// The shape of a launch: launch_shape() of tree_vjp_table.hpp, with SIP_LQR_TREE_VJP_SHAPE=<wavefronts>,<entries per
// run> (a measuring aid, read per call; 0 entries: the default run) in place of the defaults.
Shape shape_of_launch(long in_len, long out_len, long batch);

// An empty input arena launches nothing.
hipError_t launch_tree_vjp(const Args &a, hipStream_t stream);

} // namespace tree_vjp
} // namespace sipamd
