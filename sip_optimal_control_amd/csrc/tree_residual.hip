// tree_residual.hip -- instantiations and launcher of the tree KKT residual (tree_residual.hpp), declared in
// tree_residual_launch.hpp.  A translation unit of its own: compiled in parallel with the others, and the solve
// kernels keep their modules.
#include "tree_residual.hpp"
#include "tree_residual_launch.hpp"

#include <algorithm>
#include <vector>

namespace sipamd {
namespace residual {

namespace {
// Dynamic LDS a launch may ask for without raising the kernel's limit.
constexpr size_t kLdsBudget = 64 * 1024;

template <bool STAGED, bool SPLIT>
hipError_t launch_as(const tree::Meta &meta, const TreeForm &f, const TreeArgs &a, hipStream_t stream) {
  hipLaunchKernelGGL((tree_residual_kernel<STAGED, SPLIT>), dim3((unsigned)a.batch), dim3(kLanes * f.waves),
                     f.lds_bytes, stream, meta, a.input, a.rhs, a.sol, a.res, a.scaled, a.scale, a.norm, f.wave_bytes);
  return hipGetLastError();
}
template <bool STAGED>
hipError_t launch_form(const tree::Meta &meta, const TreeForm &f, const TreeArgs &a, hipStream_t stream) {
  return f.split ? launch_as<STAGED, true>(meta, f, a, stream) : launch_as<STAGED, false>(meta, f, a, stream);
}

// The form at `wave_bytes` per wavefront: split where it is wanted and the parts and one wavefront fit the budget;
// then as many wavefronts as fit, at most kMaxWaves and no more than items.  waves == 0: not even one fits.
TreeForm form_for(const size_t wave_bytes, const size_t parts_bytes, const int num_nodes, const int num_edges,
                  const bool want_split) {
  const size_t room = kLdsBudget - kRedBytes;
  TreeForm f;
  f.split = want_split && parts_bytes + wave_bytes <= room;
  const size_t left = f.split ? room - parts_bytes : room;
  const int fit = (int)std::min<size_t>(left / wave_bytes, (size_t)kMaxWaves);
  f.waves = std::min(fit, f.split ? num_nodes + num_edges : std::max(1, num_nodes));
  f.wave_bytes = (int)wave_bytes;
  f.lds_bytes = kRedBytes + (size_t)f.waves * wave_bytes + (f.split ? parts_bytes : 0);
  return f;
}
} // namespace

TreeShape tree_launch_shape(const int num_nodes, const int num_edges, const int *state_dims, const int *control_dims,
                            const int *edge_parents, const int *edge_children) {
  int max_n = 0, max_m = 0, max_children = 0;
  std::vector<int> children(num_nodes, 0);
  long image = 0; // scalars of the largest item: Q of a node, A | B | M | R of an edge
  for (int i = 0; i < num_nodes; ++i) {
    max_n = std::max(max_n, state_dims[i]);
    image = std::max(image, (long)state_dims[i] * state_dims[i]);
  }
  for (int e = 0; e < num_edges; ++e) {
    const long np = state_dims[edge_parents[e]], nc = state_dims[edge_children[e]], m = control_dims[e];
    max_m = std::max(max_m, control_dims[e]);
    max_children = std::max(max_children, ++children[edge_parents[e]]);
    image = std::max(image, nc * np + nc * m + np * m + m * m);
  }
  const size_t zb = std::max<size_t>(16, (size_t)tree_z_doubles(max_n, max_m) * sizeof(double));
  const size_t staged_wave = zb + (size_t)tree_image_bytes(image);
  const size_t parts = tree_parts_bytes(num_nodes, num_edges, max_n);
  // Split where one node's children alone outnumber a wavefront's even share of all items: there the nodes-in-turn
  // form leaves the other wavefronts idle (measured: 2x on a root with 63 children); elsewhere it is the faster one
  // by 14 % (no second gather of the parent's x, no barrier: DESIGN 4.10.1).
  const bool want_split = (long)max_children * kMaxWaves > (long)num_nodes + num_edges;
  TreeShape sh;
  sh.staged = staged_wave <= kLdsBudget - kRedBytes;
  sh.direct = form_for(zb, parts, num_nodes, num_edges, want_split);
  sh.form = sh.staged ? form_for(staged_wave, parts, num_nodes, num_edges, want_split) : sh.direct;
  return sh;
}

hipError_t launch_tree_residual(const tree::Meta &meta, const TreeShape &sh, const TreeArgs &a, hipStream_t stream) {
  if (sh.direct.waves < 1 || a.batch < 1 || a.batch > 0x7fffffffL || (a.scaled != nullptr && a.scale == nullptr))
    return hipErrorInvalidValue;
  // the image is copied by 16-byte pieces from the piece that holds the item's first scalar: input must be aligned
  if (sh.staged && ((uintptr_t)a.input & 15) == 0)
    return launch_form<true>(meta, sh.form, a, stream);
  return launch_form<false>(meta, sh.direct, a, stream);
}

} // namespace residual
} // namespace sipamd
