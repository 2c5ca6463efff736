// tree_plan.hpp -- what a tree plan decides on the host once its GenericPlan is laid out: the size class of the fused
// kernels, the flattened traversal they walk and the partition of their scratch.  No HIP call and no kernel here:
// sip_lqr_tree.hip uploads and launches, tests/cpp/test_tree_plan.cpp prints every record on the host.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "generic_plan.hpp"
#include "tree_qw16_launch.hpp"

namespace sipamd {

// The padded size class of the fused tree kernels that serves the plan; nullptr: the general engine only
// (SIP_LQR_TREE=general | global, a tree beyond the classes, or an empty input or output arena: the clamped loads of
// the fused kernels need one readable scalar in each).
inline const TreeClass *choose_tree_class(const GenericPlan &g) {
  const char *variant = std::getenv("SIP_LQR_TREE");
  const bool general_only =
      variant != nullptr && (std::strcmp(variant, "general") == 0 || std::strcmp(variant, "global") == 0);
  if (general_only || g.in0_len < 1 || g.out_len < 1)
    return nullptr;
  return find_tree_class(std::max(1, g.max_n), std::max(1, g.max_m));
}

// The flattened traversal on the host.  `sched` has every scalar field; its two pointers are set when the records
// are on the device (backward steps first, then the forward ones).
struct HostTreeSchedule {
  std::vector<TreeStep> backward, forward;
  TreeSchedule sched{};
};

// The rule of tree_schedule.hpp over the tables of a laid-out plan (tree-native arenas).  A record takes its fields
// from the step's node and edge, except where a line below says otherwise.
inline HostTreeSchedule build_tree_schedule(const GenericPlan &g) {
  auto input_of_node = [&](TreeStep &st, int j) {
    st.node = j, st.n = g.state_dims[j];
    st.oQ = g.oQ[j], st.oq = g.oq[j], st.oc = g.oc[j], st.od = g.od[j];
  };
  auto work_of_node = [&](TreeStep &st, int i) {
    st.oV = g.oV[i], st.oF = g.oF[i], st.osd = g.osd[i], st.osdi = g.osdi[i], st.ov = g.ov[i];
  };
  auto of_edge = [&](TreeStep &st, int e) {
    const int ch = g.children[e];
    st.edge = e, st.child = ch, st.nc = g.state_dims[ch], st.m = g.control_dims[e];
    st.oA = g.oA[e], st.oB = g.oB[e], st.oM = g.oM[e], st.oR = g.oR[e], st.orr = g.orr[e], st.odc = g.od[ch];
    st.oK = g.oK[e], st.ok = g.ok[e], st.oW = g.oW[e], st.oG = g.oG[e];
    st.ou = g.ou[e], st.oxc = g.ox[ch], st.oyc = g.oy[ch];
  };
  HostTreeSchedule h;
  int finished = -1; // node finished by the previous backward step
  for (int idx = 0; idx < g.N; ++idx) {
    const int j = g.postorder[idx];
    const int lo = g.child_offsets[j], hi = g.child_offsets[j + 1];
    for (int ci = lo; ci < hi; ++ci) {
      TreeStep st{};
      st.kind = 0;
      input_of_node(st, j), work_of_node(st, j), of_edge(st, g.child_edges[ci]);
      st.oxp = g.ox[j];       // edge step: x of the PARENT (j is the edge's parent)
      st.ov = g.ov[st.child]; // v of the CHILD: read back by the single-rhs solve (tree_mrhs_qw16.hpp)
      st.flags = (ci == lo ? TS_LOAD_V : 0) | (st.child == finished ? TS_CHILD_LIVE : 0);
      h.backward.push_back(st);
      finished = -1;
    }
    TreeStep st{};
    st.kind = 1;
    input_of_node(st, j), work_of_node(st, j);
    st.oxp = g.ox[j]; // node step: x of the node ITSELF
    st.flags = lo == hi ? TS_LOAD_V : 0;
    h.backward.push_back(st);
    finished = j;
  }
  int produced = g.root; // node whose x the previous forward step produced (the root's comes first)
  for (int idx = 0; idx < g.N; ++idx) {
    const int j = g.preorder[idx];
    for (int ci = g.child_offsets[j]; ci < g.child_offsets[j + 1]; ++ci) {
      TreeStep st{};
      input_of_node(st, j), of_edge(st, g.child_edges[ci]);
      work_of_node(st, st.child); // all five work fields of the CHILD (the multi-rhs rollout solves with its F)
      st.oxp = g.ox[j];           // x of the PARENT
      st.flags = j == produced ? TS_CHILD_LIVE : 0;
      h.forward.push_back(st);
      produced = st.child;
    }
  }
  TreeSchedule &t = h.sched;
  t.n_backward = (int)h.backward.size(), t.n_forward = (int)h.forward.size();
  t.Nn = g.N, t.E = g.E, t.root = g.root, t.root_n = g.state_dims[g.root];
  t.root_od = g.od[g.root], t.root_ox = g.ox[g.root], t.root_oy = g.oy[g.root];
  t.in_len = g.in0_len, t.out_len = g.out_len, t.ws_len = g.ws_len;
  return h;
}

// Scratch of the fused kernels, in bytes for the whole batch: the padded gains at 0, then the per-node spill, each
// rounded up to 256 bytes.  What an edge and a node take there is the size class's to say (TreeLayout<N, M>).
struct TreeScratch {
  size_t at_spill = 0, bytes = 0;
};
inline TreeScratch partition_tree_scratch(const TreeClass &k, int64_t batch, int num_nodes, int num_edges) {
  const size_t B = (size_t)batch * sizeof(double);
  auto up = [](size_t v) { return (v + 255) / 256 * 256; };
  TreeScratch s;
  s.at_spill = up(B * ((size_t)num_edges * (size_t)k.gain_scalars));
  s.bytes = up(s.at_spill + B * ((size_t)num_nodes * (size_t)k.spill_scalars));
  return s;
}

} // namespace sipamd
