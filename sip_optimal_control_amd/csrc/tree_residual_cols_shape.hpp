// tree_residual_cols_shape.hpp -- the launch shape of the tree residual (tree_residual.hpp), for one column and for
// several: how many columns one launch carries, how many wavefronts a workgroup has, whether the matrices of an item go
// through LDS, whether the wavefronts take nodes and edges alike (split), and the dynamic LDS that takes.  What the
// rules read of a plan, the constants and the sizes of the kernel's LDS are stated here and nowhere else.  Host
// arithmetic only: no HIP call and no kernel in here, so a host program can print the decisions
// (tests/cpp/test_tree_residual_cols_shape.cpp).  The kernel header includes it for the sizes it shares.
//
// LDS of a workgroup: NC doubles per wavefront slot for the norms (kTreeColsMaxWaves slots), then per wavefront
//   node part   x_i | y_i | q_i | acc head | acc tail        5 max_n NC doubles, z[k][c]: the NC columns of an entry adjacent
//   edge part   x_p | u | x_c | y_c | r | c_c                (4 max_n + 2 max_m) NC doubles, packed by the edge's dims
//   delta_c     max_n doubles, once: it belongs to the input arena, not to a column
// padded to 16 bytes, then, when staged, the image of the largest item: its doubles behind at most one of lead-in,
// padded likewise; behind the wavefronts, in the split form, the parts: head | tail, max_n NC doubles each, per node
// and per edge.
//
// Rules:
//   never more than 64 KiB;
//   staged needs `input` 16-byte aligned and the largest item's image plus the NC vector sets of one wavefront to fit;
//   staged with fewer columns is taken before unstaged with more;
//   the widest instantiation tried is the least of 1, 2, 4, 8 that holds the requested columns, so a short group is
//   never launched on one twice as wide as it needs;
//   split is wanted where one node's children alone outnumber a wavefront's even share of all items
//   (max_children * 4 > N + E: there nodes in turn leave the other wavefronts idle, measured 2x on a root with 63
//   children; elsewhere they are faster by 14 %, with no second gather of the parent's x and no barrier: DESIGN
//   4.10.1) and is taken at a column count only where the parts and two wavefronts fit there (with one wavefront it
//   shares nothing out);
//   where split is wanted and kTreeColsPreferSplit is set, the largest column count at which split can be taken wins
//   over a larger one with nodes in turn; where it is not set, the largest column count that fits with nodes in turn
//   wins, and runs split only if split can be taken at that very count;
//   otherwise columns come first and wavefronts second: the largest column count of which one wavefront fits, then as
//   many wavefronts as fit, at most kTreeColsMaxWaves and no more than items (N + E split, N else).
#pragma once
#include <cstddef>
#include <vector>

#if defined(__HIPCC__)
#define SIP_TREE_COLS_HD __host__ __device__
#else
#define SIP_TREE_COLS_HD
#endif

// 1: where the split form is wanted, fewer columns split are taken before more columns with nodes
// in turn.  Measured on the reference's shallow wide tree (63 children of the root, 8 columns): split
// with 2 columns a launch beats nodes in turn with 8, which a build with 0 here gives, at batch 4096 and at 1024.
#ifndef SIP_TREE_RESIDUAL_COLS_PREFER_SPLIT
#define SIP_TREE_RESIDUAL_COLS_PREFER_SPLIT 1
#endif

namespace sipamd {
namespace residual {

constexpr int kTreeColsMax = 8;      // columns of the widest instantiation; the instantiations are 1, 2, 4 and 8
constexpr int kTreeColsMaxWaves = 4; // wavefronts of a workgroup
constexpr bool kTreeColsPreferSplit = SIP_TREE_RESIDUAL_COLS_PREFER_SPLIT != 0;
constexpr size_t kTreeColsLdsBudget = 64 * 1024;

struct TreeColsShape {
  int columns = 0; // of the instantiation that is launched: 1, 2, 4 or 8 (a shorter group masks the rest); 0: nothing fits
  int waves = 0;
  bool staged = false, split = false;
  size_t lds_bytes = 0;
};

// What the rules read of a plan: from state_dims[N], control_dims[E], edge_parents[E], edge_children[E].
struct TreeColsDims {
  int num_nodes = 0, num_edges = 0, max_n = 0, max_m = 0, max_children = 0;
  long image_scalars = 0; // of the largest item: Q of a node, A | B | M | R of an edge
};

inline TreeColsDims tree_cols_dims(const int num_nodes, const int num_edges, const int *state_dims,
                                   const int *control_dims, const int *edge_parents, const int *edge_children) {
  TreeColsDims d;
  d.num_nodes = num_nodes, d.num_edges = num_edges;
  for (int i = 0; i < num_nodes; ++i) {
    const long n = state_dims[i];
    d.max_n = state_dims[i] > d.max_n ? state_dims[i] : d.max_n;
    d.image_scalars = n * n > d.image_scalars ? n * n : d.image_scalars;
  }
  std::vector<int> children(num_nodes > 0 ? num_nodes : 1, 0);
  for (int e = 0; e < num_edges; ++e) {
    const int born = ++children[edge_parents[e]];
    d.max_children = born > d.max_children ? born : d.max_children;
    const long np = state_dims[edge_parents[e]], nc = state_dims[edge_children[e]], m = control_dims[e];
    d.max_m = control_dims[e] > d.max_m ? control_dims[e] : d.max_m;
    const long image = nc * np + nc * m + np * m + m * m;
    d.image_scalars = image > d.image_scalars ? image : d.image_scalars;
  }
  return d;
}

// front of the dynamic LDS: NC doubles per wavefront slot for the norms
SIP_TREE_COLS_HD inline int tree_cols_red_bytes(const int nc) { return nc * 8 * kTreeColsMaxWaves; }
// doubles of one wavefront's vectors, padded to a whole number of 16-byte pieces (never none: a tree of empty nodes)
SIP_TREE_COLS_HD inline int tree_cols_z_doubles(const int max_n, const int max_m, const int nc) {
  const int z = (nc * (9 * max_n + 2 * max_m) + max_n + 1) & ~1;
  return z < 2 ? 2 : z;
}
// the split form's parts
SIP_TREE_COLS_HD inline size_t tree_cols_parts_bytes(const int num_nodes, const int num_edges, const int max_n,
                                                     const int nc) {
  return (size_t)(num_nodes + num_edges) * 2 * (size_t)max_n * (size_t)nc * sizeof(double);
}
// the image behind at most one scalar of lead-in, padded to whole pieces
inline size_t tree_cols_image_bytes(const long scalars) { return ((size_t)scalars * 8 + 16 + 15) & ~(size_t)15; }

// The instantiation that carries `requested` columns: the least of 1, 2, 4, 8 that holds them.
inline int tree_cols_instance(const int requested) {
  int nc = 1;
  while (nc < requested && nc < kTreeColsMax)
    nc *= 2;
  return nc;
}

// The shape at `nc` columns, staged or not, split or not; waves == 0: it does not fit (split: not with two wavefronts).
inline TreeColsShape tree_cols_shape_at(const TreeColsDims &d, const int nc, const bool staged, const bool split) {
  const size_t wave_bytes =
      (size_t)tree_cols_z_doubles(d.max_n, d.max_m, nc) * 8 + (staged ? tree_cols_image_bytes(d.image_scalars) : 0);
  const size_t fixed =
      (size_t)tree_cols_red_bytes(nc) + (split ? tree_cols_parts_bytes(d.num_nodes, d.num_edges, d.max_n, nc) : 0);
  TreeColsShape s;
  if (fixed + (split ? 2 : 1) * wave_bytes > kTreeColsLdsBudget)
    return s;
  const int items = split ? d.num_nodes + d.num_edges : (d.num_nodes > 1 ? d.num_nodes : 1);
  int waves = (int)((kTreeColsLdsBudget - fixed) / wave_bytes);
  waves = waves < kTreeColsMaxWaves ? waves : kTreeColsMaxWaves;
  waves = waves < items ? waves : items;
  if (split && waves < 2)
    return s;
  s.columns = nc, s.waves = waves, s.staged = staged, s.split = split;
  s.lds_bytes = fixed + (size_t)waves * wave_bytes;
  return s;
}

inline TreeColsShape tree_cols_shape(const TreeColsDims &d, const bool input_aligned, const int requested,
                                     const bool prefer_split = kTreeColsPreferSplit) {
  const bool want_split = (long)d.max_children * kTreeColsMaxWaves > (long)d.num_nodes + d.num_edges;
  const int top = tree_cols_instance(requested);
  for (int staged = 1; staged >= 0; --staged) {
    if (staged && !input_aligned)
      continue;
    if (want_split && prefer_split)
      for (int nc = top; nc >= 1; nc /= 2) {
        const TreeColsShape s = tree_cols_shape_at(d, nc, staged != 0, true);
        if (s.waves > 0)
          return s;
      }
    for (int nc = top; nc >= 1; nc /= 2) {
      const TreeColsShape s = tree_cols_shape_at(d, nc, staged != 0, false);
      if (s.waves < 1)
        continue;
      if (want_split) { // (not preferred, or no column count at which it can be taken: only where it costs no column)
        const TreeColsShape sp = tree_cols_shape_at(d, nc, staged != 0, true);
        if (sp.waves > 0)
          return sp;
      }
      return s;
    }
  }
  return TreeColsShape{};
}

} // namespace residual
} // namespace sipamd
