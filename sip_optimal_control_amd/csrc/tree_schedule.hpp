// tree_schedule.hpp -- the flattened traversal the fused tree kernels walk (tree_qw16.hpp, tree_mrhs_qw16.hpp): the
// records and nothing else, so that the host code that builds them (tree_plan.hpp) needs no kernel.
#pragma once

namespace sipamd {

// One step of the flattened traversal (built on the host from the compiled topology, one table per
// plan): everything a step needs is ONE record read by scalar loads, instead of a chain of dependent
// table look-ups (postorder -> child_offsets -> child_edges -> children -> dims -> offsets) in front
// of every step.  Offsets are in doubles from the start of one problem inside its tree-native arena
// (include/sip_lqr_amd.h).
//   backward: for node in postorder { EDGE step per child edge, in CSR order; then the NODE step }
//   forward : one step per edge, parents in preorder, child edges in CSR order; its work-arena fields
//             oV, oF, osd, osdi, ov are those of the CHILD (read by the multi-rhs rollout, tree_mrhs_qw16.hpp)
struct TreeStep {
  int kind;   // backward: 0 = edge, 1 = node
  int node;   // edge steps: the parent; node steps: the node
  int edge, child;
  int n, nc, m; // dim(node), dim(child), control dim of the edge
  int flags;    // TS_*
  long oQ, oq, oc, od;             // input arena, of `node`
  long oA, oB, oM, oR, orr, odc;   // input arena, of the edge; delta of the child
  long oK, ok;                     // work arena: K, k of the edge
  long oW, oG;                     // work arena: W, G_factor of the edge (LQR::Workspace, lqr.hpp:109-135)
  long oV, oF, osd, osdi, ov;      // work arena: V, F_factor, sqrt_delta, sqrt_delta_inv, v of `node`
  long ou, oxc, oyc, oxp;          // output arena: u of the edge, x / y of the child, x of the parent (node steps: of `node`)
};
enum {
  TS_LOAD_V = 1,    // backward: [V | v] = [Q | q] of `node` first (first child edge of a node / a leaf's node step)
  TS_CHILD_LIVE = 2 // backward edge: the child was finished by the previous step: its W, t, v are still in registers
                    // forward edge: x of the parent is the x the previous step produced (still in registers)
};

struct TreeSchedule { // device tables + sizes
  const TreeStep *backward, *forward;
  int n_backward, n_forward; // Nn + E, E
  int Nn, E, root, root_n;
  long root_od, root_ox, root_oy;
  long in_len, out_len, ws_len;
};

} // namespace sipamd
