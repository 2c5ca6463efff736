// tree_residual_launch.hpp -- the launcher of the KKT residual on the tree-native arenas (tree_residual.hpp,
// instantiated in tree_residual.hip, a translation unit of its own) and what a tree plan decides for it on the host.
// The refinement update is the chain's (residual_launch.hpp: launch_update).  No kernel source in here: the host code
// (sip_lqr_tree.hip) includes this header and residual_launch.hpp alone.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "tree_generic.hpp"

namespace sipamd {
namespace residual {

// Waves of a workgroup and dynamic LDS bytes of one form of the kernel; split: the wavefronts take nodes and edges
// alike and rho_q is summed from per-item parts in LDS (else they take nodes, each with its child edges).
struct TreeForm {
  int waves = 0, wave_bytes = 0;
  bool split = false;
  size_t lds_bytes = 0;
};
// What the launches of one plan use; staged: the matrices of a node and of an edge go through LDS (else the largest of
// them exceeds a wavefront's share and they are read in place).  direct: the form of the in-place kernel, which also
// serves a staged plan whose input is not 16-byte aligned.
struct TreeShape {
  bool staged = false;
  TreeForm form, direct;
};
// From the host tables of a compiled topology: state_dims[N], control_dims[E], edge_parents[E], edge_children[E].
TreeShape tree_launch_shape(int num_nodes, int num_edges, const int *state_dims, const int *control_dims,
                            const int *edge_parents, const int *edge_children);

// What one launch is told.  Buffers are whole-batch device pointers: input and sol in the input / output arenas'
// layouts, rhs (or nullptr: q, c, r of input) and the results in the output arena's.
struct TreeArgs {
  long batch;
  const double *input, *rhs, *sol;
  // plain form (scaled == nullptr): res may be nullptr; scaled form: rho / s to scaled, s to scale
  double *res, *scaled, *scale, *norm;
};
// A staged plan whose `input` is not 16-byte aligned is served by the in-place kernel.
hipError_t launch_tree_residual(const tree::Meta &meta, const TreeShape &shape, const TreeArgs &a, hipStream_t stream);

} // namespace residual
} // namespace sipamd
