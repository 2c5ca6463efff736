// tree_residual_cols.hip -- instantiations and launcher of the tree KKT residual (tree_residual.hpp), for one column
// and for several, declared in tree_residual_cols_launch.hpp.  A translation unit of its own: compiled in parallel with
// the others, and the solve kernels keep their modules.
#include "tree_residual.hpp"
#include "tree_residual_cols_launch.hpp"

namespace sipamd {
namespace residual {

namespace {
template <bool STAGED, bool SPLIT, int NC>
hipError_t launch_cols_as(const tree::Meta &meta, const TreeColsShape &sh, const TreeColsArgs &a, int ncols,
                          hipStream_t stream) {
  const size_t fixed =
      tree_cols_red_bytes(NC) + (SPLIT ? tree_cols_parts_bytes(meta.num_nodes, meta.num_edges, meta.max_n, NC) : 0);
  const int wave_bytes = (int)((sh.lds_bytes - fixed) / sh.waves);
  hipLaunchKernelGGL((tree_residual_kernel<STAGED, SPLIT, NC>), dim3((unsigned)a.batch), dim3(kLanes * sh.waves),
                     sh.lds_bytes, stream, meta, a.input, a.rhs_cols, a.sol_cols, a.batch * meta.out_len, a.batch, ncols,
                     a.res, a.scaled, a.scale, a.norm, wave_bytes);
  return hipGetLastError();
}

template <bool STAGED, bool SPLIT>
hipError_t launch_cols_instance(const tree::Meta &meta, const TreeColsShape &sh, const TreeColsArgs &a, int ncols,
                                hipStream_t stream) {
  switch (sh.columns) {
  case 1: return launch_cols_as<STAGED, SPLIT, 1>(meta, sh, a, ncols, stream);
  case 2: return launch_cols_as<STAGED, SPLIT, 2>(meta, sh, a, ncols, stream);
  case 4: return launch_cols_as<STAGED, SPLIT, 4>(meta, sh, a, ncols, stream);
  case 8: return launch_cols_as<STAGED, SPLIT, 8>(meta, sh, a, ncols, stream);
  default: return hipErrorInvalidValue;
  }
}

template <bool STAGED>
hipError_t launch_cols_form(const tree::Meta &meta, const TreeColsShape &sh, const TreeColsArgs &a, int ncols,
                            hipStream_t stream) {
  return sh.split ? launch_cols_instance<STAGED, true>(meta, sh, a, ncols, stream)
                  : launch_cols_instance<STAGED, false>(meta, sh, a, ncols, stream);
}
} // namespace

hipError_t launch_tree_residual_cols(const tree::Meta &meta, const TreeColsDims &dims, const TreeColsArgs &a,
                                     int num_cols, hipStream_t stream) {
  if (num_cols < 1 || a.batch < 1 || a.batch > 0x7fffffffL || (a.scaled != nullptr && a.scale == nullptr))
    return hipErrorInvalidValue;
  // the image is copied by 16-byte pieces from the piece that holds the item's first scalar: input must be aligned
  const bool aligned = ((uintptr_t)a.input & 15) == 0;
  const int group = tree_cols_shape(dims, aligned, kTreeColsMax).columns; // what a full launch carries
  if (group < 1)
    return hipErrorInvalidValue;
  const size_t stride = (size_t)a.batch * (size_t)meta.out_len;
  for (int c0 = 0; c0 < num_cols; c0 += group) {
    const int nc = num_cols - c0 < group ? num_cols - c0 : group;
    TreeColsArgs g = a;
    g.rhs_cols = a.rhs_cols ? a.rhs_cols + c0 * stride : nullptr;
    g.sol_cols = a.sol_cols + c0 * stride;
    g.res = a.res ? a.res + c0 * stride : nullptr;
    g.scaled = a.scaled ? a.scaled + c0 * stride : nullptr;
    g.scale = a.scale ? a.scale + (size_t)c0 * a.batch : nullptr;
    g.norm = a.norm + (size_t)c0 * a.batch;
    const TreeColsShape sh = tree_cols_shape(dims, aligned, nc);
    if (sh.columns < nc || sh.waves < 1)
      return hipErrorInvalidValue;
    const hipError_t e =
        sh.staged ? launch_cols_form<true>(meta, sh, g, nc, stream) : launch_cols_form<false>(meta, sh, g, nc, stream);
    if (e != hipSuccess)
      return e;
  }
  return hipSuccess;
}

} // namespace residual
} // namespace sipamd
