// sip_kkt_amd.hip -- C ABI of the batched Newton-KKT step
// (include/sip_kkt_amd.h) over csrc/kkt_kernels.hpp and the library's own LQR
// entry points (include/sip_lqr_amd.h).  What a plan holds and how it is laid
// out and decided: kkt_plan.hpp; here its device tables and the launches.
#include "../../include/sip_kkt_amd.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <new>
#include <string>
#include <vector>

#include "generic_plan.hpp"
#include "stream_fill.hpp"
#include "table_packer.hpp"
#include "kkt_plan.hpp"

const sipamd::kkt::KktChainKernels *sipamd::kkt::find_kkt_chain_kernels(const int n, const int m) {
#define SIP_KKT_ROW_IF(N, M) \
  if (n == N && m == M)      \
    return &kkt_chain_row<N, M>;
#define SIP_KKT_ROWS_IF(N) SIP_KKT_FAMILY_SHAPES(SIP_KKT_ROW_IF, N)
  SIP_KKT_FAMILY_N(SIP_KKT_ROWS_IF)
#undef SIP_KKT_ROWS_IF
#undef SIP_KKT_ROW_IF
  return &kkt_chain_row<0, 0>;
}

sip_kkt_plan::~sip_kkt_plan() {
  sip_lqr_plan_destroy(chain), sip_lqr_plan_destroy(chain_sym), sip_lqr_tree_plan_destroy(tree); // (NULL: nothing)
  for (void *d : {d_ints, d_longs, d_theta_longs})
    if (d)
      (void)hipFree(d);
}

namespace {

using sipamd::report;
using sipamd::TablePacker;
using sipamd::kkt::Meta;
using sipamd::kkt::ptr;
namespace kkt = sipamd::kkt; // (the LDS descriptions next to the kernels, and what is derived from them: kkt::...)

// The preamble of a compute entry point: the plan's device is the current one while this lives, whatever the
// caller's (which is restored).  rc != SIP_LQR_OK: reported as `what`, to be returned.
struct OnPlanDevice {
  sipamd::DeviceGuard guard;
  hipStream_t s;
  int rc;
  OnPlanDevice(const sip_kkt_plan *p, void *stream, const char *what)
      : guard(p->device), s((hipStream_t)stream), rc(report(guard.err, what)) {}
};

unsigned item_grid(const sip_kkt_plan *p) { return (unsigned)(p->batch * (p->N + p->E)); }
unsigned node_grid(const sip_kkt_plan *p) { return (unsigned)(p->batch * p->N); }

// Condensation by the chain kernels.  split: mats for sip_lqr_factor_solve_split -- no A | B in it.
void condense_chain(const sip_kkt_plan *p, double *in0, double *in1, const double *inv, const double *model,
                    const double *r1, const double *b, hipStream_t s, const bool split, const bool sym) {
  kkt::ChainKkt ck = p->ck;
  if (split) { // the same chain, its mats in the split (and packed) layout
    ck.split = 1, ck.sym = sym ? 1 : 0;
    ck = kkt::chain_kkt_derive(ck);
    ck.mats_len = kkt::chain_mats_len(ck);
  }
  const size_t lds = kkt::lds_bytes(kkt::condense_lds(ck, true, 1)); // of THIS layout
  const long kkt_len = (long)p->x_dim + p->y_dim + p->z_dim, per = (long)p->y_dim + p->z_dim;
  // one-stage kernel over `nb` problems starting at problem `q0`
  auto one_stage = [&](const long q0, const long nb) {
    hipLaunchKernelGGL(b ? p->k->condense_rhs : p->k->condense, dim3((unsigned)(nb * p->N)), dim3(kkt::TPB), lds, s, ck,
                       model + q0 * ck.model_len, r1 + q0 * p->x_dim, inv + q0 * per, in0 + q0 * ck.mats_len,
                       b ? b + q0 * kkt_len : nullptr, b ? in1 + q0 * ck.vecs_len : nullptr, nb, (const int32_t *)nullptr,
                       1, 0L, 0L);
  };
  // SIP_KKT_PIPE=0, or an item longer than one pass of the pipelined walk; and the pipelined kernel copies 16-byte
  // pieces: the arena itself has to be 16-byte aligned
  if (p->chain_pipe <= 0 || ((uintptr_t)model & 7) != 0)
    return one_stage(0, (long)p->batch);
  // the last item of the arena, if of odd length: its last 16-byte piece would reach 8 bytes past the caller's array,
  // so the last problem goes to the one-stage kernel
  const bool odd_tail = (ck.n * ck.n + (ck.cT + ck.gT) * ck.n) & 1;
  const long pipe_batch = odd_tail ? (long)p->batch - 1 : (long)p->batch;
  if (pipe_batch > 0)
    hipLaunchKernelGGL(b ? p->k->condense_pipe_rhs : p->k->condense_pipe,
                       dim3((unsigned)((pipe_batch * p->N + p->chain_pipe - 1) / p->chain_pipe)), dim3(kkt::TPB), lds, s,
                       ck, model, r1, inv, in0, b, in1, pipe_batch, p->chain_pipe); // (in1: NULL without b)
  if (odd_tail)
    one_stage((long)p->batch - 1, 1);
}

// b != nullptr (fused factor+solve on the staged and chain kernels): also builds q_mod, r_mod, c_mod, from the one
// staging of the model.  split, sym: chain kernels only.
hipError_t launch_condense(const sip_kkt_plan *p, void *work, const double *model, const double *w, const double *r1,
                           const double *r2, const double *r3, const double *b, hipStream_t s,
                           const bool split = false, const bool sym = false) {
  double *in0 = ptr<double>(work, p->ws.in0), *in1 = b ? ptr<double>(work, p->ws.in1) : nullptr;
  double *inv = ptr<double>(work, p->ws.inv);
  int *reg = ptr<int>(work, p->ws.reg);
  hipError_t e = sipamd::zero_async(reg, (size_t)p->batch * sizeof(int), s); // a kernel: stream_fill.hpp
  if (e != hipSuccess)
    return e;
  const long per = (long)p->y_dim + p->z_dim;
  if (per > 0)
    hipLaunchKernelGGL(kkt::weights_kernel, dim3((unsigned)((p->batch * per + 255) / 256)), dim3(256), 0, s, p->meta, w,
                       r2, r3, inv, reg, (long)p->batch);
  if (p->chain_kernels)
    condense_chain(p, in0, in1, inv, model, r1, b, s, split, sym);
  else if (p->staged)
    hipLaunchKernelGGL(b ? kkt::condense_staged_kernel<true> : kkt::condense_staged_kernel<false>, dim3(node_grid(p)),
                       dim3(kkt::TPB), kkt::lds_bytes(kkt::condense_staged_lds(p->meta)), s, p->meta, model, r1, inv,
                       in0, b, in1, (long)p->batch);
  else
    hipLaunchKernelGGL(kkt::condense_kernel, dim3(item_grid(p)), dim3(kkt::TPB), 0, s, p->meta, model, r1, inv, in0,
                       (long)p->batch);
  return hipGetLastError();
}

hipError_t launch_merge(const sip_kkt_plan *p, void *work, int32_t *status, hipStream_t s) {
  hipLaunchKernelGGL(kkt::merge_status_kernel, dim3((unsigned)((p->batch + 255) / 256)), dim3(256), 0, s,
                     ptr<int>(work, p->ws.reg), status, (long)p->batch, (int)SIP_KKT_NONPOSITIVE_REGULARIZATION);
  return hipGetLastError();
}

// Right-hand sides of one column, into `in1`.  The generic kernels take the LQR offsets of `mt`: p->meta, or (tree
// plans) a copy that places q | c, r in the column layout of sip_lqr_tree_solve_multi.
hipError_t launch_rhs(const sip_kkt_plan *p, const Meta &mt, void *work, double *in1, const double *model,
                      const double *b, const int32_t *status, hipStream_t s) {
  double *in0 = ptr<double>(work, p->ws.in0), *inv = ptr<double>(work, p->ws.inv);
  if (p->chain_kernels)
    hipLaunchKernelGGL(p->k->rhs, dim3(node_grid(p)), dim3(kkt::TPB), kkt::lds_bytes(kkt::condense_lds(p->ck, false, 1)),
                       s, p->ck, model, (const double *)nullptr, inv, in0, b, in1, (long)p->batch, status, 1, 0L, 0L);
  else
    hipLaunchKernelGGL(p->staged ? kkt::rhs_staged_kernel : kkt::rhs_kernel, dim3(p->staged ? node_grid(p) : item_grid(p)),
                       dim3(kkt::TPB), p->staged ? kkt::lds_bytes(kkt::rhs_staged_lds(mt)) : 0, s, mt, model, b, inv, in1,
                       status, (long)p->batch);
  return hipGetLastError();
}

// The multipliers and the solution of one column from the Riccati solution `out`.
hipError_t launch_recover(const sip_kkt_plan *p, void *work, double *out, const double *model, const double *b,
                          double *sol, const int32_t *status, hipStream_t s) {
  double *inv = ptr<double>(work, p->ws.inv);
  if (p->chain_kernels)
    hipLaunchKernelGGL(p->k->recover, dim3(node_grid(p)), dim3(kkt::TPB), kkt::lds_bytes(kkt::recover_lds(p->ck, 1)), s,
                       p->ck, model, b, inv, out, sol, status, (long)p->batch, 1, 0L, 0L, 0L);
  else
    hipLaunchKernelGGL(p->staged ? kkt::recover_staged_kernel : kkt::recover_kernel,
                       dim3(p->staged ? node_grid(p) : item_grid(p)), dim3(kkt::TPB),
                       p->staged ? kkt::lds_bytes(kkt::recover_staged_lds(p->meta)) : 0, s, p->meta, model, b, inv, out,
                       sol, status, (long)p->batch);
  return hipGetLastError();
}

// [x | theta | y | z] vectors of the add_Kx_to_y entry points as an ApplyIO (all blocks).
kkt::ApplyIO kkt_vector_io(const sip_kkt_plan *p, int theta_dim, const double *d_x, double *d_y) {
  const long xt = (long)p->x_dim + theta_dim, full = xt + p->y_dim + p->z_dim;
  kkt::ApplyIO io;
  io.x_x = d_x, io.x_y = d_x + xt, io.x_z = d_x + xt + p->y_dim;
  io.y_x = d_y, io.y_y = d_y + xt, io.y_z = d_y + xt + p->y_dim;
  io.sx = io.sy = io.sz = full;
  io.parts = kkt::AP_ALL;
  return io;
}

// y += (selected blocks of K) x.  d_theta != nullptr: x-space vectors carry theta behind the
// stagewise x and the theta sections of the operators are added (apply_theta_kernel).
int apply_blocks(const sip_kkt_plan *p, const double *d_model, const double *d_theta, const double *d_w,
                 const double *d_r1, const double *d_r2, const double *d_r3, const kkt::ApplyIO &io, void *stream,
                 const char *what) {
  OnPlanDevice dev(p, stream, what);
  if (dev.rc != SIP_LQR_OK)
    return dev.rc;
  hipStream_t s = dev.s;
  const int th = d_theta != nullptr ? p->theta_dim : 0;
  if (p->chain_kernels) {
    hipLaunchKernelGGL(p->k->apply, dim3(node_grid(p)), dim3(kkt::TPB), kkt::lds_bytes(kkt::apply_lds(p->ck)), s, p->ck,
                       th, d_model, d_w, d_r1, d_r2, d_r3, io, (long)p->batch);
  } else {
    Meta wide = p->meta; // x-space = [stagewise x | theta]
    wide.theta_dim = th;
    hipLaunchKernelGGL(kkt::apply_kernel, dim3(item_grid(p)), dim3(kkt::TPB), 0, s, wide, d_model, d_w, d_r1, d_r2,
                       d_r3, io, (long)p->batch);
  }
  if (th > 0 && p->chain_theta) {
    // W wavefronts per problem, as many as 64 KiB of LDS hold (kkt_theta_chain_kernels.hpp)
    const int fit = kkt::lds_count_that_fits(kkt::apply_theta_lds(p->ck, p->ct, 1), kkt::APPLY_THETA_MAX_WAVES);
    const int waves = std::max(1, std::min(fit, p->N));
    hipLaunchKernelGGL(p->k->apply_theta, dim3((unsigned)p->batch), dim3(64 * waves),
                       kkt::lds_bytes(kkt::apply_theta_lds(p->ck, p->ct, waves)), s, p->ck, p->ct, d_theta, d_r1, io,
                       (long)p->batch);
  } else if (th > 0)
    hipLaunchKernelGGL(kkt::apply_theta_kernel, dim3((unsigned)p->batch), dim3(kkt::TPB), 0, s, p->meta, p->theta_meta,
                       d_theta, d_r1, io, (long)p->batch);
  return report(hipGetLastError(), what);
}

// One of the five block operators: xs / ys = vector space of x / y (0 x-space, 1 y-space, 2 z-space).
int block_op(const sip_kkt_plan *p, const double *d_model, const double *d_theta, int part, int xs, int ys,
             const double *d_x, double *d_y, void *stream, const char *what) {
  if (p == nullptr || p->input_status != SIP_KKT_SUCCESS)
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  const int th = d_theta != nullptr ? p->theta_dim : 0;
  const long len[3] = {(long)p->x_dim + th, (long)p->y_dim, (long)p->z_dim};
  if (len[xs] == 0 || len[ys] == 0)
    return SIP_LQR_OK; // an empty space: nothing to add
  if ((!d_model && p->model_len > 0) || !d_x || !d_y)
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  kkt::ApplyIO io{};
  io.sx = len[0], io.sy = len[1], io.sz = len[2];
  (xs == 0 ? io.x_x : xs == 1 ? io.x_y : io.x_z) = d_x;
  (ys == 0 ? io.y_x : ys == 1 ? io.y_y : io.y_z) = d_y;
  io.parts = part;
  return apply_blocks(p, d_model, d_theta, nullptr, nullptr, nullptr, nullptr, io, stream, what);
}

int fill_status(const sip_kkt_plan *p, int32_t *d_status, hipStream_t s) {
  std::vector<int32_t> st((size_t)p->batch, p->input_status);
  if (hipMemcpyAsync(d_status, st.data(), st.size() * sizeof(int32_t), hipMemcpyHostToDevice, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return SIP_LQR_ERR_HIP;
  return SIP_LQR_OK;
}

// Riccati back end of a plan with valid dimensions + the lengths and offsets of its arenas (into `g`, host tables
// only).  SIP_LQR_OK with input_status still SIP_KKT_INVALID_INPUT: go on; with another status: latched.
int create_back_end(sip_kkt_plan *p, sipamd::GenericPlan &g) {
  const int E = p->E;
  g.set_shape(E, p->root, p->sd.data(), p->cd.data());
  g.parents = p->parents, g.children = p->children;
  if (kkt::is_uniform_chain(*p)) {
    const int rc = sip_lqr_plan_create(SIP_LQR_F64, p->batch, E, p->sd[0], p->cd[0], p->device, &p->chain);
    if (rc != SIP_LQR_OK)
      return rc;
    g.layout_chain(p->sd[0], p->cd[0], E);
    p->in0_len = g.in0_len, p->in1_len = g.in1_len, p->out_len = g.out_len, p->gain_len = g.gain_len;
    p->lqr_bytes = sip_lqr_workspace_bytes(p->chain);
    return SIP_LQR_OK;
  }
  const int none = 0; // an edge-less tree still needs non-null edge arrays (lqr.cpp:566-569)
  const int rc = sip_lqr_tree_plan_create(p->batch, E, p->root, E ? p->parents.data() : &none,
                                          E ? p->children.data() : &none, p->sd.data(), E ? p->cd.data() : &none,
                                          p->device, &p->tree);
  if (rc != SIP_LQR_OK)
    return rc;
  if (sip_lqr_tree_topology_status(p->tree) != SIP_LQR_SUCCESS) {
    p->input_status = sip_lqr_tree_topology_status(p->tree); // INVALID_TOPOLOGY, latched
    p->name = "invalid topology";
    return SIP_LQR_OK;
  }
  g.layout_tree_native();
  // (in1: the tree arena holds q, r, c too -- the per-problem stride of the arena rhs_kernel writes)
  p->in0_len = p->in1_len = g.in0_len, p->out_len = g.out_len, p->gain_len = 0;
  p->lqr_bytes = sip_lqr_tree_work_len(p->tree) * sizeof(double) * (size_t)p->batch;
  return SIP_LQR_OK;
}

// The plan's tables on its device, and p->meta pointing into them.
hipError_t upload_tables(sip_kkt_plan *p, const sipamd::GenericPlan &g, const std::vector<int> &y_is_dyn,
                         const std::vector<long> (&fo_layout)[kkt::FO_NUM_BLOCKS]) {
  const int E = p->E, N = p->N;
  // incoming edge of every node (the root has none); child CSR as the LQR compiles it
  std::vector<int> in_edge(N, -1), child_offsets(N + 1, 0), child_edges(E, 0);
  for (int e = 0; e < E; ++e)
    in_edge[p->children[e]] = e, ++child_offsets[p->parents[e] + 1];
  for (int i = 0; i < N; ++i)
    child_offsets[i + 1] += child_offsets[i];
  std::vector<int> cursor(child_offsets.begin(), child_offsets.end() - 1);
  for (int e = 0; e < E; ++e)
    child_edges[cursor[p->parents[e]]++] = e; // stable in the edge index (lqr.cpp:588-598)
  Meta &m = p->meta; // (its lds_* fields are set by decide_paths)
  m.E = E, m.N = N, m.root = p->root, m.x_dim = p->x_dim, m.y_dim = p->y_dim, m.z_dim = p->z_dim;
  m.model_len = p->model_len, m.in0_len = p->in0_len, m.in1_len = p->in1_len, m.out_len = p->out_len;
  TablePacker<int> ints;
  ints.push(p->sd, &m.sd), ints.push(p->cd, &m.cd), ints.push(p->ncd, &m.ncd), ints.push(p->ngd, &m.ngd);
  ints.push(p->ecd, &m.ecd), ints.push(p->egd, &m.egd), ints.push(p->parents, &m.parent);
  ints.push(p->children, &m.child), ints.push(in_edge, &m.in_edge), ints.push(child_offsets, &m.child_offsets);
  ints.push(child_edges, &m.child_edges), ints.push(y_is_dyn, &m.y_is_dyn);
  const int **vec[7] = {&m.x_state, &m.x_control, &m.y_dyn, &m.y_node_c, &m.y_edge_c, &m.z_node, &m.z_edge};
  for (int t = 0; t < 7; ++t)
    ints.push(p->voff[t], vec[t]);
  TablePacker<long> longs;
  for (int b = 0; b < kkt::NUM_BLOCKS; ++b)
    longs.push(p->moff[b], &m.mo[b]);
  // (the twelve LQR tables this Meta has, in its own order: a walk over GenericPlan::kOffsetFields would need a second
  // table of kkt::Meta members beside it, which is these lines again)
  longs.push(g.oQ, &m.oQ), longs.push(g.od, &m.od), longs.push(g.oq, &m.oq), longs.push(g.oc, &m.oc);
  longs.push(g.ox, &m.ox), longs.push(g.oy, &m.oy), longs.push(g.oA, &m.oA), longs.push(g.oB, &m.oB);
  longs.push(g.oM, &m.oM), longs.push(g.oR, &m.oR), longs.push(g.orr, &m.orr), longs.push(g.ou, &m.ou);
  p->fo_at = longs.flat.size();
  for (const auto &block : fo_layout)
    longs.push(block);
  sipamd::DeviceGuard on_device(p->device); // the caller's current device is restored on return
  hipError_t e = on_device.err;
  if (e == hipSuccess)
    e = ints.upload(&p->d_ints);
  if (e == hipSuccess)
    e = longs.upload(&p->d_longs);
  return e;
}

} // namespace

extern "C" {

int sip_kkt_plan_create(int64_t batch, int num_edges, int root, const int *edge_parents, const int *edge_children,
                        const int *state_dims, const int *control_dims, const int *node_c_dims, const int *node_g_dims,
                        const int *edge_c_dims, const int *edge_g_dims, int device, sip_kkt_plan **out) {
  if (out == nullptr)
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  if (batch < 1 || num_edges < 0 || state_dims == nullptr || (num_edges > 0 && control_dims == nullptr))
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  sip_kkt_plan *p = new (std::nothrow) sip_kkt_plan;
  if (p == nullptr)
    return SIP_LQR_ERR_ALLOC;
  *out = p;
  // validate
  kkt::set_dims(*p, batch, num_edges, root, edge_parents, edge_children, state_dims, control_dims, node_c_dims,
                node_g_dims, edge_c_dims, edge_g_dims, device);
  if (!kkt::validate(*p, num_edges == 0 || (edge_parents != nullptr && edge_children != nullptr))) {
    p->name = "invalid input";
    return SIP_LQR_OK; // latched (helpers.cpp:24-26)
  }
  // layouts
  p->model_len = kkt::walk_arena(*p, kkt::MODEL_ARENA, 0, p->moff);
  const std::vector<int> y_is_dyn = kkt::vector_layout(*p);
  std::vector<long> fo_layout[kkt::FO_NUM_BLOCKS];
  const long fo_len = kkt::walk_arena(*p, kkt::FIRST_ORDER_ARENA, 0, fo_layout);
  // back end, workspace, paths, name
  sipamd::GenericPlan g;
  const int rc = create_back_end(p, g);
  if (rc != SIP_LQR_OK) {
    delete p;
    *out = nullptr;
    return rc;
  }
  if (p->input_status != SIP_KKT_INVALID_INPUT)
    return SIP_LQR_OK; // invalid topology, latched
  p->ws = kkt::work_offsets(*p);
  kkt::decide_paths(*p, kkt::kkt_env());
  p->name = kkt::plan_name(*p);
  // upload
  const hipError_t he = upload_tables(p, g, y_is_dyn, fo_layout);
  if (he != hipSuccess) {
    std::fprintf(stderr, "sip_kkt_plan_create: HIP error: %s\n", hipGetErrorString(he));
    delete p;
    *out = nullptr;
    return SIP_LQR_ERR_HIP;
  }
  kkt::first_order_commit(*p, 0, fo_layout, fo_len);
  p->input_status = SIP_KKT_SUCCESS;
  return SIP_LQR_OK;
}

void sip_kkt_plan_destroy(sip_kkt_plan *plan) { delete plan; }

int sip_kkt_input_status(const sip_kkt_plan *p) { return p ? p->input_status : SIP_KKT_INVALID_INPUT; }

size_t sip_kkt_len(const sip_kkt_plan *p, int which) {
  if (p == nullptr || p->input_status != SIP_KKT_SUCCESS)
    return 0;
  return which == SIP_KKT_LEN_X ? (size_t)p->x_dim : which == SIP_KKT_LEN_Y ? (size_t)p->y_dim
         : which == SIP_KKT_LEN_Z ? (size_t)p->z_dim : which == SIP_KKT_LEN_MODEL ? (size_t)p->model_len : 0;
}

size_t sip_kkt_model_offset(const sip_kkt_plan *p, int block, int index) {
  if (p == nullptr || p->input_status != SIP_KKT_SUCCESS || block < 0 || block >= SIP_KKT_NUM_BLOCKS ||
      index < 0 || index >= (block <= SIP_KKT_NODE_DG_DX ? p->N : p->E))
    return (size_t)-1;
  return (size_t)p->moff[block][index];
}

size_t sip_kkt_vector_offset(const sip_kkt_plan *p, int table, int index) {
  if (p == nullptr || p->input_status != SIP_KKT_SUCCESS || table < 0 || table > SIP_KKT_Z_EDGE || index < 0)
    return (size_t)-1;
  const bool per_edge = table == SIP_KKT_X_CONTROL || table == SIP_KKT_Y_EDGE_C || table == SIP_KKT_Z_EDGE;
  if (index >= (per_edge ? p->E : p->N))
    return (size_t)-1;
  return (size_t)p->voff[table][index];
}

size_t sip_kkt_work_bytes(const sip_kkt_plan *p) { return (p && p->input_status == SIP_KKT_SUCCESS) ? p->ws.end : 0; }

const char *sip_kkt_kernel_name(const sip_kkt_plan *p) { return p ? p->name.c_str() : ""; }

int sip_kkt_plan_set_tree_fused(sip_kkt_plan *p, int on) {
  if (p == nullptr || p->theta_dim != 0 || (on && p->tree_fused))
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  if (!on || p->input_status != SIP_KKT_SUCCESS || p->tree == nullptr)
    return SIP_LQR_OK; // chain plans (and plans without a Riccati back end): nothing to switch
  const size_t scratch = sip_lqr_tree_fused_scratch_bytes(p->tree);
  if (scratch == 0)
    return SIP_LQR_OK; // beyond the size classes, or SIP_LQR_TREE=general: the general engine stays
  p->tree_fused = true;
  p->tree_scratch_bytes = scratch; // behind the regions d_work had
  p->ws = kkt::work_offsets(*p);
  p->name = kkt::plan_name(*p);
  return SIP_LQR_OK;
}

int sip_kkt_plan_set_chain_separate_sweeps(sip_kkt_plan *p, int on) {
  if (p == nullptr || p->theta_dim != 0 || (on && p->chain != nullptr && sip_lqr_has_separate_sweeps(p->chain)))
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  if (!on || p->input_status != SIP_KKT_SUCCESS || p->chain == nullptr)
    return SIP_LQR_OK; // tree plans: nothing to switch
  const int rc = sip_lqr_plan_set_separate_sweeps(p->chain, 1);
  if (rc != SIP_LQR_OK || !sip_lqr_has_separate_sweeps(p->chain))
    return rc; // not a plan of the n = 32 matrix-core kernel: nothing changed
  // (the Riccati workspace of such a plan already holds what the separate sweeps keep; should it ever grow, the
  // arena, which ends d_work, grows with it)
  p->lqr_bytes = std::max(p->lqr_bytes, sip_lqr_workspace_bytes(p->chain));
  p->ws = kkt::work_offsets(*p);
  p->name = kkt::plan_name(*p);
  return SIP_LQR_OK;
}

int sip_kkt_plan_set_chain_wide_controls(sip_kkt_plan *p, int on) {
  if (p == nullptr || p->theta_dim != 0 || (on && p->chain != nullptr && sip_lqr_has_wide_controls(p->chain)))
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  if (!on || p->input_status != SIP_KKT_SUCCESS || p->chain == nullptr)
    return SIP_LQR_OK; // tree plans: nothing to switch
  const int rc = sip_lqr_plan_set_wide_controls(p->chain, 1);
  if (rc != SIP_LQR_OK || !sip_lqr_has_wide_controls(p->chain))
    return rc; // not a chain of 9 to 16 controls on the general engine: nothing changed
  // (the Riccati plan keeps no split form -- the general engine had none either -- so the step takes the copy path
  // n = 32 takes; its workspace, which ends d_work, is now the larger of the two layouts)
  p->lqr_bytes = std::max(p->lqr_bytes, sip_lqr_workspace_bytes(p->chain));
  p->ws = kkt::work_offsets(*p);
  p->name = kkt::plan_name(*p);
  return SIP_LQR_OK;
}

int sip_kkt_factor(const sip_kkt_plan *p, const double *d_model, const double *d_w, const double *d_r1,
                   const double *d_r2, const double *d_r3, void *d_work, int32_t *d_status, void *stream) {
  if (p == nullptr || d_status == nullptr)
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  OnPlanDevice dev(p, stream, "sip_kkt_factor(hipSetDevice)");
  if (dev.rc != SIP_LQR_OK)
    return dev.rc;
  if (p->input_status != SIP_KKT_SUCCESS)
    return fill_status(p, d_status, dev.s);
  if ((!d_model && p->model_len > 0) || (!d_w && p->z_dim > 0) || (!d_r1 && p->x_dim > 0) ||
      (!d_r2 && p->y_dim > 0) || (!d_r3 && p->z_dim > 0) || !d_work)
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  hipError_t e = launch_condense(p, d_work, d_model, d_w, d_r1, d_r2, d_r3, nullptr, dev.s);
  if (e != hipSuccess)
    return report(e, "sip_kkt_factor(condense)");
  double *in0 = ptr<double>(d_work, p->ws.in0), *lqr = ptr<double>(d_work, p->ws.lqr);
  const int rc = p->chain ? sip_lqr_factor(p->chain, in0, ptr<double>(d_work, p->ws.gain), d_status, lqr, dev.s)
                 : p->tree_fused ? sip_lqr_tree_factor_fused(p->tree, in0, lqr, d_status,
                                                             ptr<char>(d_work, p->ws.tree_scratch), dev.s)
                                 : sip_lqr_tree_factor(p->tree, in0, lqr, d_status, dev.s);
  if (rc != SIP_LQR_OK)
    return rc;
  return report(launch_merge(p, d_work, d_status, dev.s), "sip_kkt_factor(status)");
}

int sip_kkt_solve(const sip_kkt_plan *p, const double *d_model, const double *d_b, double *d_sol, void *d_work,
                  const int32_t *d_status, void *stream) {
  if (p == nullptr || d_status == nullptr)
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  if (p->input_status != SIP_KKT_SUCCESS)
    return SIP_LQR_OK; // nothing was factored; solve() after a false factor() is undefined in the reference
  const long kkt_len = (long)p->x_dim + p->y_dim + p->z_dim;
  if ((!d_model && p->model_len > 0) || (kkt_len > 0 && (!d_b || !d_sol)) || !d_work)
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  OnPlanDevice dev(p, stream, "sip_kkt_solve(hipSetDevice)");
  if (dev.rc != SIP_LQR_OK)
    return dev.rc;
  double *in0 = ptr<double>(d_work, p->ws.in0), *in1 = ptr<double>(d_work, p->ws.in1);
  double *out = ptr<double>(d_work, p->ws.out), *lqr = ptr<double>(d_work, p->ws.lqr);
  hipError_t e = launch_rhs(p, p->meta, d_work, in1, d_model, d_b, d_status, dev.s);
  if (e != hipSuccess)
    return report(e, "sip_kkt_solve(rhs)");
  const int rc = p->chain ? sip_lqr_solve(p->chain, in0, in1, out, ptr<double>(d_work, p->ws.gain), lqr, dev.s)
                 : p->tree_fused ? sip_lqr_tree_solve_fused(p->tree, in0, lqr, out, d_status,
                                                            ptr<char>(d_work, p->ws.tree_scratch), dev.s)
                                 : sip_lqr_tree_solve(p->tree, in0, lqr, out, d_status, dev.s);
  if (rc != SIP_LQR_OK)
    return rc;
  return report(launch_recover(p, d_work, out, d_model, d_b, d_sol, d_status, dev.s), "sip_kkt_solve(recover)");
}

int sip_kkt_factor_solve(const sip_kkt_plan *p, const double *d_model, const double *d_w, const double *d_r1,
                         const double *d_r2, const double *d_r3, const double *d_b, double *d_sol, void *d_work,
                         int32_t *d_status, void *stream) {
  if (p == nullptr || d_status == nullptr)
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  if (p->input_status != SIP_KKT_SUCCESS || p->chain == nullptr) {
    const int rc = sip_kkt_factor(p, d_model, d_w, d_r1, d_r2, d_r3, d_work, d_status, stream);
    return rc != SIP_LQR_OK ? rc : sip_kkt_solve(p, d_model, d_b, d_sol, d_work, d_status, stream);
  }
  const long kkt_len = (long)p->x_dim + p->y_dim + p->z_dim;
  if (!d_model || (!d_w && p->z_dim > 0) || !d_r1 || !d_r2 || (!d_r3 && p->z_dim > 0) || !d_work ||
      (kkt_len > 0 && (!d_b || !d_sol)))
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  OnPlanDevice dev(p, stream, "sip_kkt_factor_solve(hipSetDevice)");
  if (dev.rc != SIP_LQR_OK)
    return dev.rc;
  hipStream_t s = dev.s;
  double *in0 = ptr<double>(d_work, p->ws.in0), *in1 = ptr<double>(d_work, p->ws.in1);
  double *out = ptr<double>(d_work, p->ws.out), *gain = ptr<double>(d_work, p->ws.gain);
  void *lqr = ptr<void>(d_work, p->ws.lqr);
  const bool fused_rhs = p->staged || p->chain_kernels;
  // The dynamics Jacobians stay where the model callback left them: the sweep reads them in place, at whatever
  // 8-byte aligned offsets and strides the arena puts them (odd m: odd ones; launch_qw16_split)
  const long ab_off = (long)p->ck.node_len + p->ck.n * p->ck.n + p->ck.n * p->ck.m + p->ck.m * p->ck.m;
  const long ab_stage = (long)p->ck.node_len + p->ck.edge_len;
  const bool split = p->chain_split && fused_rhs && p->E > 0 && ((uintptr_t)d_model & 7) == 0;
  const bool sym = split && p->chain_sym != nullptr;
  hipError_t e = launch_condense(p, d_work, d_model, d_w, d_r1, d_r2, d_r3, fused_rhs ? d_b : nullptr, s, split, sym);
  if (e == hipSuccess && !fused_rhs)
    e = launch_rhs(p, p->meta, d_work, in1, d_model, d_b, nullptr, s);
  if (e != hipSuccess)
    return report(e, "sip_kkt_factor_solve(condense)");
  const int rc = split ? sip_lqr_factor_solve_split(sym ? p->chain_sym : p->chain, in0, d_model + ab_off,
                                                    p->ck.model_len, ab_stage, in1, out, gain, d_status, lqr, s)
                       : sip_lqr_factor_solve(p->chain, in0, in1, out, gain, d_status, lqr, s);
  if (rc != SIP_LQR_OK)
    return rc;
  e = launch_merge(p, d_work, d_status, s);
  if (e == hipSuccess)
    e = launch_recover(p, d_work, out, d_model, d_b, d_sol, d_status, s);
  return report(e, "sip_kkt_factor_solve(recover)");
}

int sip_kkt_add_Kx_to_y(const sip_kkt_plan *p, const double *d_model, const double *d_w, const double *d_r1,
                        const double *d_r2, const double *d_r3, const double *d_x, double *d_y, void *stream) {
  if (p == nullptr || p->input_status != SIP_KKT_SUCCESS)
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  const long kkt_len = (long)p->x_dim + p->y_dim + p->z_dim;
  if (kkt_len == 0)
    return SIP_LQR_OK;
  if ((!d_model && p->model_len > 0) || (!d_w && p->z_dim > 0) || (!d_r1 && p->x_dim > 0) ||
      (!d_r2 && p->y_dim > 0) || (!d_r3 && p->z_dim > 0) || !d_x || !d_y)
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  return apply_blocks(p, d_model, nullptr, d_w, d_r1, d_r2, d_r3, kkt_vector_io(p, 0, d_x, d_y), stream,
                      "sip_kkt_add_Kx_to_y");
}

// The five block operators (helpers.hpp:20-24): one bit of ApplyPart each, vectors by space.
#define SIP_KKT_BLOCK_OP(NAME, PART, XS, YS)                                                                 \
  int sip_kkt_add_##NAME##_to_y(const sip_kkt_plan *p, const double *d_model, const double *d_x, double *d_y,  \
                                void *stream) {                                                              \
    return block_op(p, d_model, nullptr, sipamd::kkt::PART, XS, YS, d_x, d_y, stream,                         \
                    "sip_kkt_add_" #NAME "_to_y");                                                           \
  }                                                                                                          \
  int sip_kkt_add_##NAME##_to_y_theta(const sip_kkt_plan *p, const double *d_model, const double *d_theta,     \
                                      const double *d_x, double *d_y, void *stream) {                        \
    if (p == nullptr || p->theta_dim < 1 || d_theta == nullptr)                                             \
      return SIP_LQR_ERR_INVALID_ARGUMENT;                                                                   \
    return block_op(p, d_model, d_theta, sipamd::kkt::PART, XS, YS, d_x, d_y, stream,                         \
                    "sip_kkt_add_" #NAME "_to_y_theta");                                                     \
  }
SIP_KKT_BLOCK_OP(Hx, AP_H, 0, 0)
SIP_KKT_BLOCK_OP(Cx, AP_C, 0, 1)
SIP_KKT_BLOCK_OP(CTx, AP_CT, 1, 0)
SIP_KKT_BLOCK_OP(Gx, AP_G, 0, 2)
SIP_KKT_BLOCK_OP(GTx, AP_GT, 2, 0)
#undef SIP_KKT_BLOCK_OP

size_t sip_kkt_first_order_len(const sip_kkt_plan *p) {
  return (p && p->input_status == SIP_KKT_SUCCESS) ? (size_t)p->first_len : 0;
}

size_t sip_kkt_first_order_offset(const sip_kkt_plan *p, int block, int index) {
  if (p == nullptr || p->input_status != SIP_KKT_SUCCESS || block < 0 || block >= SIP_KKT_FO_NUM_BLOCKS ||
      index < 0 || index >= (block <= SIP_KKT_FO_NODE_G ? p->N : p->E))
    return (size_t)-1;
  return (size_t)p->foff[block][index];
}

// Replaces the assembly of f, gradient_f, c and g in the reference's model_callback wrapper
// (sip_optimal_control.cpp:47-125); kkt_first_order_kernels.hpp.
int sip_kkt_gather_first_order(const sip_kkt_plan *p, const double *d_first, const double *d_x,
                               const double *d_initial_state, double *d_f, double *d_grad_f, double *d_c,
                               double *d_g, void *stream) {
  if (p == nullptr || p->input_status != SIP_KKT_SUCCESS || d_first == nullptr || d_f == nullptr)
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  const long xt = (long)p->x_dim + p->theta_dim;
  const bool f_only = d_grad_f == nullptr && d_c == nullptr && d_g == nullptr; // mci.new_x == false, :55
  if (!f_only) {
    if ((!d_grad_f && xt > 0) || (!d_c && p->y_dim > 0) || (!d_g && p->z_dim > 0))
      return SIP_LQR_ERR_INVALID_ARGUMENT;
    if (p->sd[p->root] > 0 && (d_x == nullptr || d_initial_state == nullptr))
      return SIP_LQR_ERR_INVALID_ARGUMENT;
  }
  OnPlanDevice dev(p, stream, "sip_kkt_gather_first_order(hipSetDevice)");
  if (dev.rc != SIP_LQR_OK)
    return dev.rc;
  using namespace sipamd::kkt;
  hipStream_t s = dev.s;
  const FoTables ft{(const long *)p->d_longs + p->fo_at, p->first_len, p->theta_dim};
  if (!f_only && p->fo_uniform)
    hipLaunchKernelGGL(gather_first_order_uniform, dim3((unsigned)((p->batch * p->N + FO_WAVES - 1) / FO_WAVES)),
                       dim3(FO_TPB), 0, s, p->fu, d_first, d_x, d_initial_state, d_grad_f, d_c, d_g, (long)p->batch);
  else if (!f_only)
    hipLaunchKernelGGL(gather_first_order_tree,
                       dim3((unsigned)((p->batch * (p->N + p->E) + FO_WAVES - 1) / FO_WAVES)), dim3(FO_TPB), 0, s,
                       p->meta, ft, d_first, d_x, d_initial_state, d_grad_f, d_c, d_g, (long)p->batch);
  // f and the theta rows: after the pass above, which has just read the same lines
  const int comps = f_only ? 1 : 1 + p->theta_dim;
  hipLaunchKernelGGL(p->fo_uniform ? gather_first_order_sums<true> : gather_first_order_sums<false>,
                     dim3((unsigned)((p->batch * comps + FO_TPB - 1) / FO_TPB)), dim3(FO_TPB), 0, s, p->fu, ft, p->N,
                     p->x_dim, comps, d_first, d_f, d_grad_f, (long)p->batch);
  return report(hipGetLastError(), "sip_kkt_gather_first_order");
}

} // extern "C"

// ---- theta (global variables): Schur complement around the stagewise solve ----
namespace {

// What the ways of forming K^-1 J_theta (helpers.cpp:387) share: the plan, the caller's arrays and the regions of
// the two workspaces.  Column c of J / KJ is at c * col_j, of vecs_cols / lsol_cols at c * col_v (the plan's).
struct ThetaFactor {
  const sip_kkt_plan *p;
  const double *model, *theta;
  void *work;
  int32_t *status;
  hipStream_t s;
  double *in0, *inv, *gain, *lqr, *J, *KJ, *vecs_cols, *lsol_cols;
  void *cws; // column workspace of sip_lqr_solve_multi (chain plans) / scratch of sip_lqr_tree_solve_multi (trees)
};

// The fused passes of kkt_theta_chain_kernels.hpp: right-hand sides of all columns straight from the theta arena, one
// multi-rhs Riccati solve, multipliers of all columns + the stage shares of the Schur complement (in J's space).
int theta_kj_fused(const ThetaFactor &t) {
  const sip_kkt_plan *p = t.p;
  hipLaunchKernelGGL(p->k->theta_rhs, dim3(node_grid(p)), dim3(kkt::TPB),
                     kkt::lds_bytes(kkt::theta_rhs_lds(p->ck, p->ct)), t.s, p->ck, p->ct, t.model, t.theta,
                     (const double *)t.inv, t.vecs_cols, p->col_v, (const int32_t *)t.status, (long)p->batch);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess)
    return report(e, "sip_kkt_factor_theta(rhs)");
  const int rc = sip_lqr_solve_multi(p->chain, t.in0, t.vecs_cols, t.lsol_cols, p->theta_dim, t.gain, t.lqr,
                                     t.cws, t.s);
  if (rc != SIP_LQR_OK)
    return rc;
  hipLaunchKernelGGL(p->k->theta_recover, dim3(node_grid(p)), dim3(kkt::TPB),
                     kkt::lds_bytes(kkt::theta_recover_lds(p->ck, p->ct)), t.s, p->ck, p->ct, t.model, t.theta,
                     (const double *)t.inv, (const double *)t.lsol_cols, p->col_v, t.KJ, p->col_j, t.J,
                     (const int32_t *)t.status, (long)p->batch);
  return report(hipGetLastError(), "sip_kkt_factor_theta(recover)");
}

// Chain kernels: the right-hand sides of all columns from one staging of the Jacobians, all columns through one
// backward / forward sweep where the shape has the multi-rhs kernel (chain_mrhs.hpp: the GEMM form of
// helpers.cpp:521-665; column by column otherwise), the multipliers of all columns from one staging.
int theta_kj_chain_columns(const ThetaFactor &t) {
  const sip_kkt_plan *p = t.p;
  const int th = p->theta_dim;
  const long colJ = p->col_j, colV = p->col_v;
  // (as many columns per launch as LDS holds)
  const int rhs_cols = kkt::lds_count_that_fits(kkt::condense_lds(p->ck, false, 1), th);
  for (int c0 = 0; c0 < th; c0 += rhs_cols) {
    const int nc = std::min(rhs_cols, th - c0);
    hipLaunchKernelGGL(p->k->rhs, dim3(node_grid(p)), dim3(kkt::TPB),
                       kkt::lds_bytes(kkt::condense_lds(p->ck, false, nc)), t.s, p->ck, t.model,
                       (const double *)nullptr, t.inv, t.in0, (const double *)t.J + (size_t)c0 * colJ,
                       t.vecs_cols + (size_t)c0 * colV, (long)p->batch, (const int32_t *)t.status, nc, colJ, colV);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess)
    return report(e, "sip_kkt_factor_theta(rhs)");
  const int rc = sip_lqr_solve_multi(p->chain, t.in0, t.vecs_cols, t.lsol_cols, th, t.gain, t.lqr, t.cws, t.s);
  if (rc != SIP_LQR_OK)
    return rc;
  const int rec_cols = kkt::lds_count_that_fits(kkt::recover_lds(p->ck, 1), th);
  for (int c0 = 0; c0 < th; c0 += rec_cols) {
    const int nc = std::min(rec_cols, th - c0);
    // (nc == 1: the single-column instantiation)
    hipLaunchKernelGGL(nc > 1 ? p->k->recover_cols : p->k->recover, dim3(node_grid(p)), dim3(kkt::TPB),
                       kkt::lds_bytes(kkt::recover_lds(p->ck, nc)), t.s, p->ck, t.model,
                       (const double *)t.J + (size_t)c0 * colJ, t.inv, (const double *)t.lsol_cols + (size_t)c0 * colV,
                       t.KJ + (size_t)c0 * colJ, (const int32_t *)t.status, (long)p->batch, nc, colJ, colV, colJ);
  }
  return report(hipGetLastError(), "sip_kkt_factor_theta(recover)");
}

// Trees: the right-hand sides of every column (the condense-rhs kernel once per column, writing q | c, r into the
// column layout of sip_lqr_tree_solve_multi instead of the LQR input arena), ONE multi-rhs Riccati solve over all
// columns against the factor state, then the multipliers of every column (the recover kernel once per column,
// reading x | y, u from the solution columns).
int theta_kj_tree_multi(const ThetaFactor &t) {
  const sip_kkt_plan *p = t.p;
  const int th = p->theta_dim;
  const long colJ = p->col_j, colV = p->col_v;
  Meta cm = p->meta; // q, c, r at the x, y, u offsets of the output layout
  cm.oq = cm.ox, cm.oc = cm.oy, cm.orr = cm.ou, cm.in1_len = cm.out_len;
  hipError_t e = hipSuccess;
  for (int col = 0; col < th && e == hipSuccess; ++col)
    e = launch_rhs(p, cm, t.work, t.vecs_cols + (size_t)col * colV, t.model, t.J + (size_t)col * colJ, t.status, t.s);
  if (e != hipSuccess)
    return report(e, "sip_kkt_factor_theta(rhs)");
  const int rc = sip_lqr_tree_solve_multi(p->tree, t.in0, (const double *)t.lqr, t.vecs_cols, t.lsol_cols, th,
                                          t.status, t.cws, t.s);
  if (rc != SIP_LQR_OK)
    return rc;
  for (int col = 0; col < th && e == hipSuccess; ++col)
    e = launch_recover(p, t.work, t.lsol_cols + (size_t)col * colV, t.model, t.J + (size_t)col * colJ,
                       t.KJ + (size_t)col * colJ, t.status, t.s);
  return report(e, "sip_kkt_factor_theta(recover)");
}

// One sip_kkt_solve per column.
int theta_kj_by_column(const ThetaFactor &t) {
  int rc = SIP_LQR_OK;
  for (int col = 0; col < t.p->theta_dim && rc == SIP_LQR_OK; ++col)
    rc = sip_kkt_solve(t.p, t.model, t.J + (size_t)col * t.p->col_j, t.KJ + (size_t)col * t.p->col_j, t.work, t.status, t.s);
  return rc;
}

} // namespace

extern "C" {

int sip_kkt_plan_set_theta(sip_kkt_plan *p, int theta_dim) {
  if (p == nullptr || theta_dim < 1 || p->theta_dim != 0 || p->input_status != SIP_KKT_SUCCESS)
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  const long theta_len = kkt::walk_arena(*p, kkt::THETA_ARENA, theta_dim, p->toff);
  TablePacker<long> longs;
  for (int b = 0; b < kkt::TH_NUM_BLOCKS; ++b)
    longs.push(p->toff[b], &p->theta_meta.to[b]);
  sipamd::DeviceGuard on_device(p->device);
  hipError_t he = on_device.err;
  if (he == hipSuccess)
    he = longs.upload(&p->d_theta_longs);
  // the first-order arena carries df_dtheta (th entries per node and edge): its table again, now, not at first use
  std::vector<long> fo_layout[kkt::FO_NUM_BLOCKS];
  const long fo_len = kkt::walk_arena(*p, kkt::FIRST_ORDER_ARENA, theta_dim, fo_layout);
  TablePacker<long> fo;
  for (const auto &block : fo_layout)
    fo.push(block);
  if (he == hipSuccess)
    he = hipMemcpy((long *)p->d_longs + p->fo_at, fo.flat.data(), fo.flat.size() * sizeof(long), hipMemcpyHostToDevice);
  if (he != hipSuccess)
    return report(he, "sip_kkt_plan_set_theta");
  kkt::first_order_commit(*p, theta_dim, fo_layout, fo_len);
  p->theta_len = theta_len, p->theta_dim = theta_dim;
  p->theta_meta.p = theta_dim, p->theta_meta.theta_len = theta_len;
  kkt::decide_theta_paths(*p, kkt::kkt_env());
  p->name = kkt::plan_name(*p);
  p->tws = kkt::theta_work_offsets(*p);
  p->col_j = (long)p->batch * ((long)p->x_dim + p->y_dim + p->z_dim);
  p->col_v = (long)p->batch * (long)kkt::theta_col_scalars(*p);
  return SIP_LQR_OK;
}

size_t sip_kkt_theta_len(const sip_kkt_plan *p) { return (p && p->theta_dim > 0) ? (size_t)p->theta_len : 0; }

size_t sip_kkt_theta_offset(const sip_kkt_plan *p, int block, int index) {
  if (p == nullptr || p->theta_dim < 1 || block < 0 || block >= SIP_KKT_TH_NUM_BLOCKS || index < 0 ||
      index >= (block <= SIP_KKT_TH_NODE_D2L_DTHETA2 ? p->N : p->E))
    return (size_t)-1;
  return (size_t)p->toff[block][index];
}

size_t sip_kkt_theta_work_bytes(const sip_kkt_plan *p) { return (p && p->theta_dim > 0) ? p->tws.end : 0; }

int sip_kkt_factor_theta(const sip_kkt_plan *p, const double *d_model, const double *d_theta, const double *d_w,
                         const double *d_r1, const double *d_r2, const double *d_r3, void *d_work,
                         void *d_theta_work, int32_t *d_status, void *stream) {
  if (p == nullptr || p->theta_dim < 1 || !d_theta || !d_theta_work || !d_r1)
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  OnPlanDevice dev(p, stream, "sip_kkt_factor_theta(hipSetDevice)");
  if (dev.rc != SIP_LQR_OK)
    return dev.rc;
  hipStream_t s = dev.s;
  const kkt::ThetaWorkOffsets &o = p->tws;
  const ThetaFactor t{p, d_model, d_theta, d_work, d_status, s, ptr<double>(d_work, p->ws.in0),
                      ptr<double>(d_work, p->ws.inv), ptr<double>(d_work, p->ws.gain), ptr<double>(d_work, p->ws.lqr),
                      ptr<double>(d_theta_work, o.J), ptr<double>(d_theta_work, o.KJ),
                      ptr<double>(d_theta_work, o.vecs_cols), ptr<double>(d_theta_work, o.lsol_cols),
                      ptr<void>(d_theta_work, o.cws)};
  double *S = ptr<double>(d_theta_work, o.S), *rhs_sw = ptr<double>(d_theta_work, o.rhs_sw);
  const int sx = p->x_dim, th = p->theta_dim;
  // r1 of problem q starts at q * (x_dim + p); the condensation kernels index r1 with the stagewise stride x_dim, so
  // they get a compacted copy (theta entries dropped) in rhs_sw's space (free until solve)
  // (a kernel, not a memcpy node: the entry points stay graph-capturable, stream_fill.hpp)
  if (sx > 0)
    hipLaunchKernelGGL(kkt::theta_strip_kernel, dim3((unsigned)((p->batch * (long)sx + 255) / 256)), dim3(256), 0, s,
                       d_r1, rhs_sw, sx, th, (long)sx, (long)p->batch);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess)
    return report(e, "sip_kkt_factor_theta(r1)");
  int rc = sip_kkt_factor(p, d_model, d_w, rhs_sw, d_r2, d_r3, d_work, d_status, stream);
  if (rc != SIP_LQR_OK)
    return rc;
  if (!p->chain_theta) {
    hipLaunchKernelGGL(kkt::theta_jacobian_kernel, dim3(node_grid(p)), dim3(kkt::TPB), 0, s, p->meta, p->theta_meta,
                       d_theta, t.J, (long)p->batch);
    if ((e = hipGetLastError()) != hipSuccess)
      return report(e, "sip_kkt_factor_theta(jacobian)");
  }
  rc = p->chain_theta        ? theta_kj_fused(t)
       : p->chain_kernels    ? theta_kj_chain_columns(t)
       : p->tree_theta_multi ? theta_kj_tree_multi(t)
                             : theta_kj_by_column(t);
  if (rc != SIP_LQR_OK)
    return rc;
  // the Schur complement and its LLT
  if (p->chain_theta) // (the sum of the stage shares)
    hipLaunchKernelGGL(kkt::theta_schur_reduce_kernel, dim3((unsigned)p->batch), dim3(kkt::TPB),
                       kkt::lds_bytes(kkt::theta_schur_lds(th)), s, p->N, th, sx, d_r1, (const double *)t.J, S, d_status,
                       (long)p->batch, (int)SIP_KKT_THETA_SCHUR_FAILURE);
  else
    hipLaunchKernelGGL(th <= 8 ? kkt::theta_schur_small_kernel<8> : kkt::theta_schur_kernel, dim3((unsigned)p->batch),
                       dim3(kkt::TPB), th <= 8 ? 0 : kkt::lds_bytes(kkt::theta_schur_lds(th)), s, p->meta, p->theta_meta,
                       d_theta, d_r1, t.J, t.KJ, S, d_status, (long)p->batch, (int)SIP_KKT_THETA_SCHUR_FAILURE);
  return report(hipGetLastError(), "sip_kkt_factor_theta(schur)");
}

int sip_kkt_solve_theta(const sip_kkt_plan *p, const double *d_model, const double *d_theta, const double *d_b,
                        double *d_sol, void *d_work, void *d_theta_work, const int32_t *d_status, void *stream) {
  if (p == nullptr || p->theta_dim < 1 || !d_theta || !d_theta_work || !d_b || !d_sol || !d_status)
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  OnPlanDevice dev(p, stream, "sip_kkt_solve_theta(hipSetDevice)");
  if (dev.rc != SIP_LQR_OK)
    return dev.rc;
  hipStream_t s = dev.s;
  const kkt::ThetaWorkOffsets &o = p->tws;
  double *J = ptr<double>(d_theta_work, o.J), *KJ = ptr<double>(d_theta_work, o.KJ), *S = ptr<double>(d_theta_work, o.S);
  double *rhs_sw = ptr<double>(d_theta_work, o.rhs_sw), *sol_sw = ptr<double>(d_theta_work, o.sol_sw);
  const int sx = p->x_dim, th = p->theta_dim;
  const long skkt = (long)sx + p->y_dim + p->z_dim;
  hipLaunchKernelGGL(kkt::theta_strip_kernel, dim3((unsigned)((p->batch * skkt + 255) / 256)), dim3(256), 0, s, d_b,
                     rhs_sw, sx, th, skkt, (long)p->batch);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess)
    return report(e, "sip_kkt_solve_theta(strip)");
  const int rc = sip_kkt_solve(p, d_model, rhs_sw, sol_sw, d_work, d_status, stream);
  if (rc != SIP_LQR_OK)
    return rc;
  if (p->chain_theta) {
    double *d_part = J + (size_t)p->batch * p->N * th * th; // behind the Schur partials (kept: solve after solve)
    hipLaunchKernelGGL(p->k->theta_dot, dim3(node_grid(p)), dim3(kkt::TPB),
                       kkt::lds_bytes(kkt::theta_dot_lds(p->ck, p->ct)), s, p->ck, p->ct, d_theta,
                       (const double *)sol_sw, d_part, d_status, (long)p->batch);
    hipLaunchKernelGGL(kkt::theta_finish_parts_kernel, dim3((unsigned)p->batch), dim3(kkt::TPB),
                       kkt::lds_bytes(kkt::theta_finish_lds(th)), s, p->N, th, sx, skkt, d_b, (const double *)d_part,
                       (const double *)KJ, (const double *)S, (const double *)sol_sw, d_sol, d_status, (long)p->batch);
  } else
    hipLaunchKernelGGL(kkt::theta_finish_kernel, dim3((unsigned)p->batch), dim3(kkt::TPB),
                       kkt::lds_bytes(kkt::theta_finish_lds(th)), s, p->meta, p->theta_meta, d_b, J, KJ, S, sol_sw,
                       d_sol, d_status, (long)p->batch);
  return report(hipGetLastError(), "sip_kkt_solve_theta(finish)");
}

int sip_kkt_add_Kx_to_y_theta(const sip_kkt_plan *p, const double *d_model, const double *d_theta,
                              const double *d_w, const double *d_r1, const double *d_r2, const double *d_r3,
                              const double *d_x, double *d_y, void *stream) {
  if (p == nullptr || p->theta_dim < 1 || !d_theta || !d_r1 || !d_x || !d_y)
    return SIP_LQR_ERR_INVALID_ARGUMENT;
  // the stagewise operator on [x | theta | y | z] vectors, then the theta terms
  return apply_blocks(p, d_model, d_theta, d_w, d_r1, d_r2, d_r3, kkt_vector_io(p, p->theta_dim, d_x, d_y), stream,
                      "sip_kkt_add_Kx_to_y_theta");
}

} // extern "C"
