// Prints the table and the launch shape of the tree gradient kernel (csrc/tree_vjp_table.hpp) for a fixed list of
// topologies.  Per tree: a "tree" line (name, nodes, edges, input_len, output_len), the four "list" lines of its
// topology and dimensions, one "shape" line per batch and override, then input_len "w ia ib code" lines, one per
// input-arena scalar in the arena's order, and "end".  Host only; tests/test_tree_vjp_table.py checks every word and
// evaluates the gradient through the table.
#include <cstdio>
#include <string>
#include <vector>

#include "../../sip_optimal_control_amd/csrc/generic_plan.hpp"
#include "../../sip_optimal_control_amd/csrc/tree_vjp_table.hpp"

namespace {
struct Tree {
  std::string name;
  std::vector<int> parents, children, sd, cd;
};

std::vector<Tree> trees() {
  std::vector<Tree> out;
  // the reference's four small trees
  out.push_back({"nonuniform_delta_chain", {0, 1, 2}, {1, 2, 3}, {3, 3, 3, 3}, {2, 2, 2}});
  out.push_back({"branch", {0, 0}, {1, 2}, {2, 2, 2}, {1, 1}});
  out.push_back({"variable_branch", {0, 0}, {1, 2}, {2, 1, 3}, {2, 1}});
  out.push_back({"five_node", {0, 0, 1, 1}, {1, 2, 3, 4}, {3, 1, 2, 4, 2}, {2, 1, 3, 1}});
  out.push_back({"single_node", {}, {}, {5}, {}});
  out.push_back({"node_n0", {0, 1, 1}, {1, 2, 3}, {3, 0, 4, 3}, {2, 1, 1}});
  out.push_back({"edge_m0", {0, 1, 1}, {1, 2, 3}, {3, 2, 4, 3}, {2, 0, 1}});
  Tree s12{"star_of_12", {}, {}, {6, 3, 4, 5, 6, 3, 4, 5, 6, 3, 4, 5, 2}, {2, 1, 3, 2, 1, 3, 2, 1, 3, 2, 1, 3}};
  for (int e = 0; e < 12; ++e)
    s12.parents.push_back(0), s12.children.push_back(e + 1);
  out.push_back(s12);
  // 70 states of 30 and 69 controls of 4 as a chain: 16 * output_len is above 64 KiB, the <direct> form
  Tree chain{"chain_30x70", {}, {}, std::vector<int>(70, 30), std::vector<int>(69, 4)};
  for (int e = 0; e < 69; ++e)
    chain.parents.push_back(e), chain.children.push_back(e + 1);
  out.push_back(chain);
  return out;
}

void list(const char *what, const std::vector<int> &v) {
  std::printf("list %s", what);
  for (int x : v)
    std::printf(" %d", x);
  std::printf("\n");
}
} // namespace

int main() {
  using namespace sipamd;
  std::printf("budget %zu lanes %d max_waves %d compute_units %ld min_run %ld max_runs %ld\n", tree_vjp::kLdsBudget,
              tree_vjp::kLanes, tree_vjp::kMaxWaves, tree_vjp::kComputeUnits, tree_vjp::kMinRun, tree_vjp::kMaxRuns);
  for (const Tree &t : trees()) {
    GenericPlan g;
    g.set_shape((int)t.cd.size(), 0, t.sd.data(), t.cd.data());
    const int none = 0; // (a tree without edges still names its edge lists)
    if (g.compile(t.parents.empty() ? &none : t.parents.data(), t.children.empty() ? &none : t.children.data()) !=
        SIP_LQR_SUCCESS)
      return 1;
    g.layout_tree_native();
    const std::vector<tree_vjp::Word> table = tree_vjp::build_table(g);
    if ((long)table.size() != g.in0_len)
      return 2;
    std::printf("tree %s nodes %d edges %d input_len %ld output_len %ld\n", t.name.c_str(), g.N, g.E, g.in0_len,
                g.out_len);
    list("parents", t.parents), list("children", t.children), list("state_dims", t.sd), list("control_dims", t.cd);
    // (batch, wavefronts asked for, entries per run asked for): the default at three batches, then overrides
    const long cases[][3] = {{4096, 0, 0}, {3, 0, 0}, {1, 0, 0}, {3, 2, 10}, {3, 4, 1}, {3, 99, 1000000000}};
    for (const auto &c : cases) {
      const tree_vjp::Shape s = tree_vjp::launch_shape(g.in0_len, g.out_len, c[0], (int)c[1], c[2]);
      std::printf("shape batch %ld ask_waves %ld ask_run %ld -> %s staged %d waves %d run %ld runs %ld lds %zu\n", c[0],
                  c[1], c[2], tree_vjp::kernel_name(s), s.staged ? 1 : 0, s.waves, s.run, s.runs, s.lds_bytes);
    }
    for (const tree_vjp::Word w : table)
      std::printf("w %u %u %u\n", tree_vjp::word_ia(w), tree_vjp::word_ib(w), tree_vjp::word_code(w));
    std::printf("end\n");
  }
  return 0;
}
