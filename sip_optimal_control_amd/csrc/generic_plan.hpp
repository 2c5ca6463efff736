// generic_plan.hpp -- host side of the general (tree_generic.hpp) engine:
// the compiled topology, the offset tables for a given arena layout, their
// upload, kernel launches.  Shared by the tree C ABI (tree-native arenas), by
// the chain C ABI (packed chain layout: shapes / dtypes without a dedicated
// kernel, and the split factor / solve entry points) and by the Newton-KKT C
// ABI (host tables only).  The 21 offset tables are named in three places: the
// members here and in tree::Meta, the field table (kOffsetFields) that pairs
// them, and the layout walks that assign them.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include <cstdlib>
#include <cstring>

#include "stream_fill.hpp"
#include "table_packer.hpp"
#include "tree_generic.hpp"
#include "tree_lds.hpp"

namespace sipamd {

// Host integer work, exactly the reference's traversal compilation
// (lqr.cpp:563-631): counting sort of the edges by parent, then an iterative
// DFS that pushes children in reverse so the lowest edge index is visited
// first; postorder is the reversed preorder.  The body of the C ABI's
// sip_lqr_compile_topology (array sizes: include/sip_lqr_amd.h).
inline int compile_topology(int num_edges, int root, const int *edge_parents, const int *edge_children,
                            int *child_offsets, int *child_edges, int *edge_parents_out, int *edge_children_out,
                            int *preorder, int *postorder, int *node_marks) {
  const int E = num_edges, N = num_edges + 1;
  if (E < 0 || edge_parents == nullptr || edge_children == nullptr)
    return SIP_LQR_INVALID_TOPOLOGY;
  if (root < 0 || root >= N)
    return SIP_LQR_INVALID_TOPOLOGY;
  std::fill(child_offsets, child_offsets + N + 1, 0);
  for (int e = 0; e < E; ++e) {
    const int p = edge_parents[e], c = edge_children[e];
    if (p < 0 || p >= N || c < 0 || c >= N || p == c)
      return SIP_LQR_INVALID_TOPOLOGY;
    edge_parents_out[e] = p;
    edge_children_out[e] = c;
    ++child_offsets[p + 1];
  }
  for (int node = 0; node < N; ++node)
    child_offsets[node + 1] += child_offsets[node];
  std::vector<int> cursor(child_offsets, child_offsets + N);
  for (int e = 0; e < E; ++e)
    child_edges[cursor[edge_parents_out[e]]++] = e;

  std::vector<int> stack;
  stack.reserve(N);
  stack.push_back(root);
  std::fill(node_marks, node_marks + N, 0);
  int visited = 0;
  while (!stack.empty()) {
    const int node = stack.back();
    stack.pop_back();
    if (visited >= N || node_marks[node] != 0)
      return SIP_LQR_INVALID_TOPOLOGY; // cycle or two parents
    node_marks[node] = 1;
    preorder[visited++] = node;
    for (int ci = child_offsets[node + 1] - 1; ci >= child_offsets[node]; --ci)
      stack.push_back(edge_children_out[child_edges[ci]]);
  }
  if (visited != N)
    return SIP_LQR_INVALID_TOPOLOGY; // disconnected
  for (int order = 0; order < N; ++order)
    postorder[order] = preorder[N - 1 - order];
  return SIP_LQR_SUCCESS;
}

struct GenericPlan {
  int E = 0, N = 0, root = 0, max_n = 0, max_m = 0;
  std::vector<int> state_dims, control_dims, parents, children;
  std::vector<int> child_offsets, child_edges, preorder, postorder;
  // per-node / per-edge offsets, see tree::Meta
  std::vector<long> oQ, od, oA, oB, oM, oR, oq, oc, orr, ox, oy, ou, oK, ok, oW, oG, oV, oF, osd,
      osdi, ov;
  long scratch_ws = 0, in0_len = 0, in1_len = 0, out_len = 0, gain_len = 0, ws_len = 0;
  void *d_ints = nullptr, *d_longs = nullptr;
  tree::Meta meta{};

  // One row per offset table: the host vector, the device pointer that is to point at its copy, and whether the
  // table has an entry per edge (else per node).  In the order of tree::Meta, which is the order of the upload.
  struct OffsetField {
    std::vector<long> GenericPlan::*host;
    const long *tree::Meta::*dev;
    bool per_edge;
  };
  static const OffsetField kOffsetFields[21];

  ~GenericPlan() {
    if (d_ints)
      (void)hipFree(d_ints);
    if (d_longs)
      (void)hipFree(d_longs);
  }

  void set_shape(int num_edges, int root_node, const int *sd, const int *cd) {
    E = num_edges, N = num_edges + 1, root = root_node;
    state_dims.assign(sd, sd + N);
    control_dims.assign(cd, cd + E);
    max_n = N ? *std::max_element(state_dims.begin(), state_dims.end()) : 0;
    max_m = E ? *std::max_element(control_dims.begin(), control_dims.end()) : 0;
    for (const OffsetField &f : kOffsetFields)
      (this->*f.host).assign(f.per_edge ? E : N, 0);
  }
  // The traversal of the shape's tree (root: set_shape) from its edge list: sizes the six topology vectors and
  // compiles them.  Returns the FactorStatus of compile_topology.
  int compile(const int *edge_parents, const int *edge_children) {
    parents.assign(E, 0), children.assign(E, 0);
    child_offsets.assign(N + 1, 0), child_edges.assign(E, 0);
    preorder.assign(N, 0), postorder.assign(N, 0);
    std::vector<int> marks(N, 0);
    return compile_topology(E, root, edge_parents, edge_children, child_offsets.data(), child_edges.data(),
                            parents.data(), children.data(), preorder.data(), postorder.data(), marks.data());
  }
  long np(int e) const { return state_dims[parents[e]]; }
  long nc(int e) const { return state_dims[children[e]]; }

  // The scratch that ends every work arena: H (max_m x max_n) | F (max_n^2), then the vectors g | h | f.
  long scratch_vec_len() const { return 2L * max_n + max_m; }
  long scratch_len() const { return (long)max_m * max_n + (long)max_n * max_n + scratch_vec_len(); }
  // Per problem and column of launch_solve_cols: the output layout (v at x, k at u), then g | h | f.
  long cols_len() const { return out_len + scratch_vec_len(); }

  // The end of every work arena: per node V | F_factor | sqrt_delta | sqrt_delta_inv | v, then the scratch.
  // `ws`: first free scalar behind the per-edge fields; sets ws_len.
  void layout_node_work(long ws) {
    for (int i = 0; i < N; ++i) {
      const long n = state_dims[i];
      oV[i] = ws, ws += n * n;
      oF[i] = ws, ws += n * n;
      osd[i] = ws, ws += n;
      osdi[i] = ws, ws += n;
      ov[i] = ws, ws += n;
    }
    scratch_ws = ws;
    ws_len = ws + scratch_len();
  }

  // Work arena of a layout that keeps its gains elsewhere: per edge W (max_n^2) | G_factor (m^2), then the
  // per-node fields and the scratch.  `start`: first free scalar of the work arena.
  void layout_work(long start) {
    long ws = start;
    for (int e = 0; e < E; ++e) {
      const long m = control_dims[e];
      oW[e] = ws, ws += (long)max_n * max_n;
      oG[e] = ws, ws += m * m;
    }
    layout_node_work(ws);
  }

  // Tree-native arenas (include/sip_lqr_amd.h, second half).  One input arena
  // (in1 == in0), gains inside the work arena with the reference's
  // LQR::Workspace field order per edge: W | K | G_factor | k.
  void layout_tree_native() {
    long in = 0, o = 0, ws = 0;
    for (int i = 0; i < N; ++i) {
      const long n = state_dims[i];
      oQ[i] = in, in += n * n;
      oq[i] = in, in += n;
      oc[i] = in, in += n;
      od[i] = in, in += n;
      ox[i] = o, o += n;
      oy[i] = o, o += n;
    }
    for (int e = 0; e < E; ++e) {
      const long m = control_dims[e];
      oA[e] = in, in += nc(e) * np(e);
      oB[e] = in, in += nc(e) * m;
      oM[e] = in, in += np(e) * m;
      oR[e] = in, in += m * m;
      orr[e] = in, in += m;
      ou[e] = o, o += m;
    }
    in0_len = in1_len = in, out_len = o;
    for (int e = 0; e < E; ++e) {
      const long m = control_dims[e];
      oW[e] = ws, ws += (long)max_n * max_n;
      oK[e] = ws, ws += m * np(e);
      oG[e] = ws, ws += m * m;
      ok[e] = ws, ws += m;
    }
    layout_node_work(ws);
    gain_len = ws_len; // the gain arena IS the work arena
  }

  // Packed chain layout (include/sip_lqr_amd.h, first half): uniform n, m,
  // chain topology; in0 = mats, in1 = vecs, out = sol, gain = gains.
  void layout_chain(int n, int m, int T) {
    const long node = (long)n * n + n, edge = (long)n * n + 2L * n * m + (long)m * m;
    const long vstg = 2L * n + m, gstg = (long)m * n + m;
    for (int i = 0; i <= T; ++i) {
      const long mb = i * (node + edge), vb = i * vstg;
      oQ[i] = mb, od[i] = mb + (long)n * n;
      oq[i] = vb, oc[i] = vb + n;
      ox[i] = vb, oy[i] = vb + n;
      if (i < T) {
        const long eb = mb + node;
        oA[i] = eb, oB[i] = eb + (long)n * n, oM[i] = oB[i] + (long)n * m, oR[i] = oM[i] + (long)n * m;
        orr[i] = vb + 2L * n;
        ou[i] = vb + 2L * n;
        oK[i] = i * gstg, ok[i] = i * gstg + (long)m * n;
      }
    }
    in0_len = (T + 1) * node + T * edge;
    in1_len = out_len = (T + 1) * 2L * n + (long)T * m;
    gain_len = T * gstg;
    layout_work(0);
  }

  // The tables on `device` (two arrays: ints, longs) and `meta` pointing into them.
  hipError_t upload(int device) {
    tree::Meta &m = meta;
    m.num_edges = E, m.num_nodes = N, m.root = root, m.max_n = max_n, m.max_m = max_m;
    m.scratch_ws = scratch_ws;
    m.in0_len = in0_len, m.in1_len = in1_len, m.out_len = out_len, m.gain_len = gain_len, m.ws_len = ws_len;
    TablePacker<int> ints;
    ints.push(state_dims, &m.state_dims), ints.push(control_dims, &m.control_dims);
    ints.push(parents, &m.edge_parents), ints.push(children, &m.edge_children);
    ints.push(child_offsets, &m.child_offsets), ints.push(child_edges, &m.child_edges);
    ints.push(preorder, &m.preorder), ints.push(postorder, &m.postorder);
    TablePacker<long> longs;
    for (const OffsetField &f : kOffsetFields)
      longs.push(this->*f.host, &(m.*f.dev));
    DeviceGuard on_device(device); // the caller's current device is restored on return
    hipError_t e = on_device.err;
    if (e == hipSuccess)
      e = ints.upload(&d_ints);
    if (e == hipSuccess)
      e = longs.upload(&d_longs);
    return e;
  }

  // LDS-resident kernels (tree_lds.hpp) when the largest node fits in 64 KB; SIP_LQR_TREE=global
  // keeps the global-memory kernels (tests, A/B).
  template <class S>
  size_t lds_bytes() const {
    const char *v = std::getenv("SIP_LQR_TREE");
    if (v != nullptr && std::strcmp(v, "global") == 0)
      return 0;
    const size_t need = (size_t)tree::lds_scalars(max_n, max_m) * sizeof(S);
    return need <= 64 * 1024 ? need : 0;
  }

  template <class S>
  hipError_t launch_factor(long batch, const void *in0, void *ws, void *gain, int32_t *status,
                           hipStream_t stream) const {
    if (const size_t lds = lds_bytes<S>())
      hipLaunchKernelGGL((tree::factor_kernel_lds<S>), dim3((unsigned)batch), dim3(tree::TPB), lds, stream, meta,
                         (const S *)in0, (S *)ws, (S *)gain, (int *)status, batch);
    else
      hipLaunchKernelGGL((tree::factor_kernel<S>), dim3((unsigned)batch), dim3(tree::TPB), 0, stream, meta,
                         (const S *)in0, (S *)ws, (S *)gain, (int *)status, batch);
    return hipGetLastError();
  }
  template <class S>
  hipError_t launch_solve(long batch, const void *in0, const void *in1, void *ws, void *gain, void *out,
                          const int32_t *status, hipStream_t stream) const {
    if (const size_t lds = lds_bytes<S>())
      hipLaunchKernelGGL((tree::solve_kernel_lds<S>), dim3((unsigned)batch), dim3(tree::TPB), lds, stream, meta,
                         (const S *)in0, (const S *)in1, (S *)ws, (S *)gain, (S *)out, (const int *)status,
                         batch);
    else
      hipLaunchKernelGGL((tree::solve_kernel<S>), dim3((unsigned)batch), dim3(tree::TPB), 0, stream, meta,
                         (const S *)in0, (const S *)in1, (S *)ws, (S *)gain, (S *)out, (const int *)status,
                         batch);
    return hipGetLastError();
  }
  // `num_rhs` right-hand sides against one factorization, one launch per column.  Columns are in the OUTPUT layout
  // (q | c where x | y are, r where u is; column k of the batch at k * batch * out_len, right-hand sides and
  // solutions alike); the work arena is only read: v / k / g | h | f of a problem go to cols_len() scalars of `cols`,
  // reused by every column.
  template <class S>
  hipError_t launch_solve_cols(long batch, const S *in0, const S *ws, const S *rhs_cols, S *out_cols, int num_rhs,
                               S *cols, const int32_t *status, hipStream_t stream) const {
    tree::Meta mt = meta;
    mt.oq = mt.ox, mt.oc = mt.oy, mt.orr = mt.ou, mt.in1_len = mt.out_len;
    const long col = batch * out_len;
    hipError_t e = hipSuccess;
    for (int k = 0; k < num_rhs && e == hipSuccess; ++k) {
      hipLaunchKernelGGL((tree::solve_cols_kernel<S>), dim3((unsigned)batch), dim3(tree::TPB), 0, stream, mt, in0,
                         rhs_cols + k * col, ws, out_cols + k * col, cols, mt.ox, mt.ou, out_len, cols_len(),
                         (const int *)status, batch);
      e = hipGetLastError();
    }
    return e;
  }
};

#define SIP_OFFSET_FIELD(name, per_edge) {&GenericPlan::name, &tree::Meta::name, per_edge}
inline const GenericPlan::OffsetField GenericPlan::kOffsetFields[21] = {
    SIP_OFFSET_FIELD(oQ, false),  SIP_OFFSET_FIELD(od, false),   SIP_OFFSET_FIELD(oA, true),
    SIP_OFFSET_FIELD(oB, true),   SIP_OFFSET_FIELD(oM, true),    SIP_OFFSET_FIELD(oR, true),
    SIP_OFFSET_FIELD(oq, false),  SIP_OFFSET_FIELD(oc, false),   SIP_OFFSET_FIELD(orr, true),
    SIP_OFFSET_FIELD(ox, false),  SIP_OFFSET_FIELD(oy, false),   SIP_OFFSET_FIELD(ou, true),
    SIP_OFFSET_FIELD(oK, true),   SIP_OFFSET_FIELD(ok, true),    SIP_OFFSET_FIELD(oW, true),
    SIP_OFFSET_FIELD(oG, true),   SIP_OFFSET_FIELD(oV, false),   SIP_OFFSET_FIELD(oF, false),
    SIP_OFFSET_FIELD(osd, false), SIP_OFFSET_FIELD(osdi, false), SIP_OFFSET_FIELD(ov, false)};
#undef SIP_OFFSET_FIELD

} // namespace sipamd
