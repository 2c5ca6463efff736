// What a tree plan decides on the host (csrc/generic_plan.hpp: the compiled topology and the offset tables of a
// layout; csrc/tree_plan.hpp: size class, flattened traversal, scratch partition), printed for a fixed list of small
// cases: tests/test_tree_plan.py holds every offset against a walk written from the arena order
// include/sip_lqr_amd.h documents and every record against a restatement of the traversal rule.  Launches nothing,
// needs no device.
//
// Build (also done by __graft_entry__.build()):
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 tests/cpp/test_tree_plan.cpp \
//     -L sip_optimal_control_amd/lib -lsip_lqr_amd -o build/test_tree_plan
#include "../../sip_optimal_control_amd/csrc/tree_plan.hpp"

#include <cstdio>

using namespace sipamd;

namespace {

constexpr long BATCH = 3; // of the scratch partition

struct Case {
  const char *name;
  int root;
  std::vector<int> parents, children, sd, cd;
};

Case chain(const char *name, int n, int m, int T) {
  Case c{name, 0, {}, {}, std::vector<int>(T + 1, n), std::vector<int>(T, m)};
  for (int e = 0; e < T; ++e)
    c.parents.push_back(e), c.children.push_back(e + 1);
  return c;
}

const Case cases[] = {
    {"single node", 0, {}, {}, {3}, {}},
    {"one-edge chain", 0, {0}, {1}, {2, 3}, {1}},
    chain("uniform four-node chain", 3, 2, 3),
    // tests/test_topology_host.py: the second child of a node is not live, a sibling subtree intervenes; a node
    // without a state and an edge without a control
    {"five-node tree", 0, {0, 0, 1, 1}, {1, 2, 3, 4}, {3, 2, 0, 4, 1}, {2, 1, 0, 3}},
    // tests/test_kkt_plan.py: the root is not node 0
    {"branching tree, root 2", 2, {2, 0, 2, 0}, {0, 3, 1, 4}, {3, 5, 4, 0, 2}, {2, 0, 3, 1}},
    chain("two-node chain, n = 16", 16, 2, 1), // fits no size class
};

// (the order of GenericPlan::kOffsetFields, which is that of tree::Meta)
const char *const kFieldNames[21] = {"oQ", "od", "oA", "oB", "oM", "oR", "oq", "oc", "orr", "ox", "oy",
                                     "ou", "oK", "ok", "oW", "oG", "oV", "oF", "osd", "osdi", "ov"};

void print_ints(const char *what, const std::vector<int> &v) {
  std::printf("ints %s", what);
  for (const int x : v)
    std::printf(" %d", x);
  std::printf("\n");
}

void print_layout(const GenericPlan &g) {
  for (int f = 0; f < 21; ++f) {
    const GenericPlan::OffsetField &field = GenericPlan::kOffsetFields[f];
    const std::vector<long> &tab = g.*field.host;
    std::printf("tab %s %s", kFieldNames[f], field.per_edge ? "edge" : "node");
    for (const long x : tab)
      std::printf(" %ld", x);
    std::printf("\n");
  }
  std::printf("len in0 %ld in1 %ld out %ld gain %ld ws %ld scratch_ws %ld cols %ld\n", g.in0_len, g.in1_len, g.out_len,
              g.gain_len, g.ws_len, g.scratch_ws, g.cols_len());
}

void print_step(const char *sweep, const TreeStep &s) {
  std::printf("step %s kind %d node %d edge %d child %d n %d nc %d m %d flags %d oQ %ld oq %ld oc %ld od %ld oA %ld "
              "oB %ld oM %ld oR %ld orr %ld odc %ld oK %ld ok %ld oW %ld oG %ld oV %ld oF %ld osd %ld osdi %ld ov %ld "
              "ou %ld oxc %ld oyc %ld oxp %ld\n",
              sweep, s.kind, s.node, s.edge, s.child, s.n, s.nc, s.m, s.flags, s.oQ, s.oq, s.oc, s.od, s.oA, s.oB, s.oM,
              s.oR, s.orr, s.odc, s.oK, s.ok, s.oW, s.oG, s.oV, s.oF, s.osd, s.osdi, s.ov, s.ou, s.oxc, s.oyc, s.oxp);
}

int print_case(const Case &c) {
  const int E = (int)c.cd.size();
  GenericPlan g;
  g.set_shape(E, c.root, c.sd.data(), c.cd.data());
  const int none = 0; // (an edge-less tree still needs non-null edge arrays)
  const int status = g.compile(E ? c.parents.data() : &none, E ? c.children.data() : &none);
  std::printf("case %s | tree-native | root %d | topology %d\n", c.name, c.root, status);
  if (status != SIP_LQR_SUCCESS)
    return 1;
  print_ints("parents", g.parents), print_ints("children", g.children);
  print_ints("sd", g.state_dims), print_ints("cd", g.control_dims);
  print_ints("child_offsets", g.child_offsets), print_ints("child_edges", g.child_edges);
  print_ints("preorder", g.preorder), print_ints("postorder", g.postorder);
  g.layout_tree_native();
  print_layout(g);
  if (const TreeClass *k = choose_tree_class(g)) {
    const TreeScratch s = partition_tree_scratch(*k, BATCH, g.N, g.E);
    std::printf("class %d %d gain %d spill %d at_spill %zu bytes %zu name %s\n", k->n, k->m, k->gain_scalars,
                k->spill_scalars, s.at_spill, s.bytes, k->name);
  } else
    std::printf("class none\n");
  const HostTreeSchedule h = build_tree_schedule(g);
  for (const TreeStep &s : h.backward)
    print_step("backward", s);
  for (const TreeStep &s : h.forward)
    print_step("forward", s);
  const TreeSchedule &t = h.sched;
  std::printf("sched n_backward %d n_forward %d Nn %d E %d root %d root_n %d root_od %ld root_ox %ld root_oy %ld "
              "in_len %ld out_len %ld ws_len %ld\n",
              t.n_backward, t.n_forward, t.Nn, t.E, t.root, t.root_n, t.root_od, t.root_ox, t.root_oy, t.in_len,
              t.out_len, t.ws_len);
  return 0;
}

int print_chain_layout(int n, int m, int T) {
  const Case c = chain("chain", n, m, T);
  GenericPlan g;
  g.set_shape(T, 0, c.sd.data(), c.cd.data());
  const int status = g.compile(c.parents.data(), c.children.data());
  std::printf("case chain (%d, %d, %d) | packed chain | root 0 | topology %d\n", n, m, T, status);
  if (status != SIP_LQR_SUCCESS)
    return 1;
  g.layout_chain(n, m, T);
  print_layout(g);
  return 0;
}

} // namespace

int main() {
  int failures = 0;
  for (const Case &c : cases)
    failures += print_case(c);
  failures += print_chain_layout(3, 2, 2);
  return failures == 0 ? 0 : 1;
}
