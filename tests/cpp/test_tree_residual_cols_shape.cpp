// Prints the launch shape of the multi-column tree residual (csrc/tree_residual_cols_shape.hpp) for a fixed list of
// topologies, one line each: the name, what the rules read of the topology, the alignment of the input, the requested
// columns and the split preference, then columns, waves, staged, split and dynamic LDS bytes.  Host only;
// tests/test_tree_residual_cols_shape.py recomputes every line from the rules the header states.
#include <cstdio>
#include <string>
#include <vector>

#include "tree_residual_cols_shape.hpp"

namespace {
struct Tree {
  std::string name;
  std::vector<int> parents, children, sd, cd;
};

Tree star(const std::string &name, int kids, const std::vector<int> &sd_cycle, int sd_root,
          const std::vector<int> &cd_cycle) {
  Tree t{name, {}, {}, {sd_root}, {}};
  for (int e = 0; e < kids; ++e) {
    t.parents.push_back(0), t.children.push_back(e + 1);
    t.sd.push_back(sd_cycle[(e + 1) % sd_cycle.size()]);
    t.cd.push_back(cd_cycle[e % cd_cycle.size()]);
  }
  return t;
}

std::vector<Tree> trees() {
  std::vector<Tree> out;
  // the reference's four small trees and a single node
  out.push_back({"nonuniform_delta_chain", {0, 1, 2}, {1, 2, 3}, {3, 3, 3, 3}, {2, 2, 2}});
  out.push_back({"branch", {0, 0}, {1, 2}, {2, 2, 2}, {1, 1}});
  out.push_back({"variable_branch", {0, 0}, {1, 2}, {2, 1, 3}, {2, 1}});
  out.push_back({"five_node", {0, 0, 1, 1}, {1, 2, 3, 4}, {3, 1, 2, 4, 2}, {2, 1, 3, 1}});
  out.push_back({"single_node", {}, {}, {5}, {}});
  // the random trees of the hard-input tests, 10 nodes
  out.push_back({"random<9,3>", {0, 0, 2, 1, 1, 4, 0, 0, 8}, {1, 2, 3, 4, 5, 6, 7, 8, 9},
                 {9, 1, 3, 0, 2, 4, 0, 2, 7, 3}, {1, 3, 2, 3, 3, 2, 3, 3, 1}});
  out.push_back({"random<15,8>", {0, 1, 2, 0, 2, 3, 6, 6, 2}, {1, 2, 3, 4, 5, 6, 7, 8, 9},
                 {15, 11, 8, 5, 15, 0, 2, 3, 0, 15}, {4, 4, 6, 6, 8, 7, 8, 8, 5}});
  // a root of 12 children: split, and its parts fit at 8 columns
  Tree s12{"star_of_12", {}, {}, {6, 3, 4, 5, 6, 3, 4, 5, 6, 3, 4, 5, 2}, {2, 1, 3, 2, 1, 3, 2, 1, 3, 2, 1, 3}};
  for (int e = 0; e < 12; ++e)
    s12.parents.push_back(0), s12.children.push_back(e + 1);
  out.push_back(s12);
  // the reference's shallow wide tree at T = 63: state dims 7, 8, 9 in turn, control dims 1, 2, 3
  out.push_back(star("star_of_63", 63, {7, 8, 9}, 7, {1, 2, 3}));
  // 300 nodes, 160 of them children of the root, max_n = 15: the parts exceed LDS at any column count
  Tree wide{"parts_beyond_lds", {}, {}, {15}, {}};
  for (int e = 0; e < 299; ++e) {
    wide.parents.push_back(e < 160 ? 0 : (e * 7) % (e + 1)), wide.children.push_back(e + 1);
    wide.sd.push_back(1 + (e * 5) % 15), wide.cd.push_back(1 + e % 3);
  }
  out.push_back(wide);
  // a 91 x 91 block: beyond the staging budget
  out.push_back({"n91_pair", {0}, {1}, {91, 2}, {1}});
  // a tree of empty nodes, and vectors that leave room for no second column
  out.push_back({"empty_nodes", {0, 0}, {1, 2}, {0, 0, 0}, {0, 0}});
  out.push_back({"n500_pair", {0}, {1}, {500, 1}, {1}});
  return out;
}
} // namespace

int main() {
  using namespace sipamd::residual;
  std::printf("budget %zu max_columns %d max_waves %d prefer_split %d\n", kTreeColsLdsBudget, kTreeColsMax,
              kTreeColsMaxWaves, kTreeColsPreferSplit ? 1 : 0);
  for (const Tree &t : trees()) {
    const TreeColsDims d = tree_cols_dims((int)t.sd.size(), (int)t.cd.size(), t.sd.data(), t.cd.data(),
                                          t.parents.data(), t.children.data());
    // every tree: a full group, aligned and misaligned, both preferences; short groups on the aligned input
    const int cases[][3] = {{1, 8, 1}, {1, 8, 0}, {0, 8, 1}, {0, 8, 0}, {1, 1, 1}, {1, 2, 1}, {1, 3, 1}, {1, 5, 1}, {1, 5, 0}};
    for (const auto &c : cases) {
      const TreeColsShape s = tree_cols_shape(d, c[0] != 0, c[1], c[2] != 0);
      std::printf("%s nodes %d edges %d max_n %d max_m %d max_children %d image %ld aligned %d requested %d prefer %d -> "
                  "columns %d waves %d staged %d split %d lds %zu\n",
                  t.name.c_str(), d.num_nodes, d.num_edges, d.max_n, d.max_m, d.max_children, d.image_scalars, c[0],
                  c[1], c[2], s.columns, s.waves, s.staged ? 1 : 0, s.split ? 1 : 0, s.lds_bytes);
    }
  }
  return 0;
}
