// kkt_plan.hpp -- the host-side plan of the batched Newton-KKT step (include/sip_kkt_amd.h): what a plan holds
// and the functions that fill it from the dimension tables -- the arenas (tables of blocks, walk_arena), the two
// workspaces (Take), the paths (kkt_env, decide_paths, plan_name).  No kernel and no HIP call: sip_kkt_amd.hip owns
// the device side (tables, launches); tests/cpp/test_kkt_plan.cpp checks the layouts on the host.
#pragma once
#include "../../include/sip_kkt_amd.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "kkt_chain_launch.hpp"
#include "kkt_first_order_kernels.hpp"

namespace sipamd {
namespace kkt {

// Byte offsets of the regions of d_work / d_theta_work; `end` is the workspace's size.
struct WorkOffsets {
  size_t in0, in1, out, gain, inv, reg, lqr, tree_scratch, end;
};
struct ThetaWorkOffsets {
  size_t J, KJ, S, rhs_sw, sol_sw, vecs_cols, lsol_cols, cws, end; // vecs / lsol_cols, cws: the multi-rhs solves
};
// One walk over a workspace: every region starts where the one before it ends, rounded up to 256 bytes.
struct Take {
  size_t cur = 0;
  size_t operator()(const size_t bytes) {
    const size_t at = cur;
    cur = (cur + bytes + 255) / 256 * 256;
    return at;
  }
};
template <class T>
T *ptr(void *base, const size_t offset) {
  return (T *)((char *)base + offset);
}

} // namespace kkt
} // namespace sipamd

struct sip_kkt_plan {
  int64_t batch = 0;
  int device = 0;
  int E = 0, N = 0, root = 0;
  int input_status = SIP_KKT_INVALID_INPUT;
  std::vector<int> sd, cd, ncd, ngd, ecd, egd, parents, children;
  std::vector<int> voff[7];
  std::vector<long> moff[sipamd::kkt::NUM_BLOCKS];
  int x_dim = 0, y_dim = 0, z_dim = 0;
  long model_len = 0;
  // Riccati back end: packed chain plan or general tree plan
  sip_lqr_plan *chain = nullptr;
  sip_lqr_tree_plan *tree = nullptr;
  long in0_len = 0, in1_len = 0, out_len = 0, gain_len = 0;
  // d_work: the back end's arena (lqr_bytes) ends it, but for the scratch of the fused tree kernels
  size_t lqr_bytes = 0, tree_scratch_bytes = 0;
  sipamd::kkt::WorkOffsets ws{};
  void *d_ints = nullptr, *d_longs = nullptr;
  sipamd::kkt::Meta meta{};
  bool chain_kernels = false; // uniform chain: arithmetic-offset kernels (kkt_chain_kernels.hpp)
  // the fused step hands the Riccati sweep ddyn_dx | ddyn_du in the model arena instead of copying
  // them into its inputs (sip_lqr_factor_solve_split); SIP_KKT_SPLIT=0 keeps the copy
  bool chain_split = false;
  // the chain kernels the plan launches (kkt_chain_launch.hpp).  k->n > 0: the plan's dimensions are those of the
  // reference's Newton-KKT benchmark family for (k->n, k->m) -- the hot chain kernels then run as the instantiation
  // that has every dimension but the horizon as a constant (kkt_chain_kernels.hpp: family_dims); SIP_KKT_FAMILY=0
  // keeps the generic kernels
  const sipamd::kkt::KktChainKernels *k = nullptr; // (set by decide_paths)
  // ... and with Q_mod / R_mod as packed lower triangles (SIP_LQR_LAYOUT_SYMMETRIC) where the sweep has that kernel:
  // a second plan of the same shape, used by the fused step only; SIP_KKT_SYM=0 keeps the full squares
  sip_lqr_plan *chain_sym = nullptr;
  int chain_pipe = 0; // > 0: stages per wavefront of the software-pipelined condensation
  sipamd::kkt::ChainKkt ck{};
  // theta (sip_kkt_plan_set_theta)
  int theta_dim = 0;
  std::vector<long> toff[sipamd::kkt::TH_NUM_BLOCKS];
  long theta_len = 0;
  void *d_theta_longs = nullptr;
  sipamd::kkt::ThetaMeta theta_meta{};
  sipamd::kkt::ThetaWorkOffsets tws{};
  // doubles between two columns of J_theta / K^-1 J_theta, and of the right-hand sides / solutions of the multi-rhs solve
  long col_j = 0, col_v = 0;
  // uniform chains: the fused theta passes of kkt_theta_chain_kernels.hpp (J_theta never assembled);
  // SIP_KKT_THETA_FUSED=0 keeps the generic passes
  bool chain_theta = false;
  // tree plans: K^-1 J_theta through one sip_lqr_tree_solve_multi over all columns; SIP_KKT_THETA_TREE_MULTI=0
  // keeps the column-by-column sip_kkt_solve loop
  bool tree_theta_multi = false;
  // tree plans: the Riccati factor / solve on sip_lqr_tree_factor_fused / sip_lqr_tree_solve_fused, their scratch at
  // ws.tree_scratch of d_work (sip_kkt_plan_set_tree_fused)
  bool tree_fused = false;
  sipamd::kkt::ChainTheta ct{};
  // first-order arena (sip_kkt_gather_first_order): block offsets, their copy at fo_at of d_longs -- uploaded by
  // sip_kkt_plan_create and again by sip_kkt_plan_set_theta (df_dtheta then has theta_dim entries), never at first use
  std::vector<long> foff[sipamd::kkt::FO_NUM_BLOCKS];
  long first_len = 0;
  size_t fo_at = 0;
  bool fo_uniform = false; // chain_kernels plans: gather_first_order_uniform (arithmetic offsets)
  sipamd::kkt::FoUniform fu{};
  bool staged = false; // LDS-staged kernels (false: items too large for LDS, or SIP_KKT_VARIANT=direct)
  std::string name;

  ~sip_kkt_plan(); // sip_kkt_amd.hip: the back ends and the device tables
};

namespace sipamd {
namespace kkt {

inline std::vector<int> dims_or_zero(const int *src, int count) {
  return src ? std::vector<int>(src, src + count) : std::vector<int>((size_t)count, 0);
}

// The dimension tables as the caller gave them (NULL constraint tables: zeros).
inline void set_dims(sip_kkt_plan &p, int64_t batch, int E, int root, const int *parents, const int *children,
                     const int *sd, const int *cd, const int *ncd, const int *ngd, const int *ecd, const int *egd,
                     int device) {
  const int N = E + 1;
  p.batch = batch, p.device = device, p.E = E, p.N = N, p.root = root;
  p.sd.assign(sd, sd + N);
  p.cd = dims_or_zero(cd, E);
  p.ncd = dims_or_zero(ncd, N), p.ngd = dims_or_zero(ngd, N);
  p.ecd = dims_or_zero(ecd, E), p.egd = dims_or_zero(egd, E);
  p.parents = dims_or_zero(parents, E), p.children = dims_or_zero(children, E);
}

// validate_input, types.cpp:68-127 without the in-degree / reachability part,
// which the LQR traversal (lqr.cpp:563-631) latches.
inline bool validate(const sip_kkt_plan &p, bool have_topology) {
  if (!have_topology || p.root < 0 || p.root >= p.N)
    return false;
  for (int i = 0; i < p.N; ++i)
    if (p.sd[i] < 0 || p.ncd[i] < 0 || p.ngd[i] < 0)
      return false;
  for (int e = 0; e < p.E; ++e) {
    const int a = p.parents[e], c = p.children[e];
    if (p.cd[e] < 0 || p.ecd[e] < 0 || p.egd[e] < 0 || a < 0 || a >= p.N || c < 0 || c >= p.N || a == c)
      return false;
  }
  return true;
}

inline bool is_uniform_chain(const sip_kkt_plan &p) {
  if (p.E < 1 || p.root != 0 || p.sd[0] < 1 || p.cd[0] < 1)
    return false;
  for (int e = 0; e < p.E; ++e)
    if (p.parents[e] != e || p.children[e] != e + 1 || p.cd[e] != p.cd[0] || p.sd[e + 1] != p.sd[0])
      return false;
  return true;
}

// Uniform chain whose constraint dimensions are uniform too (interior nodes, terminal node, edges).
inline bool uniform_constraints(const sip_kkt_plan &p) {
  for (int i = 1; i < p.E; ++i) // (node i and edge i)
    if (p.ncd[i] != p.ncd[0] || p.ngd[i] != p.ngd[0] || p.ecd[i] != p.ecd[0] || p.egd[i] != p.egd[0])
      return false;
  return p.sd[0] <= 32 && p.cd[0] <= 32;
}

// ---- arenas: node i, then edge i; a block is rows x cols doubles ----
enum Dim { D_ONE, D_NODE, D_PARENT, D_CHILD, D_M, D_NODE_C, D_NODE_G, D_EDGE_C, D_EDGE_G, D_THETA, D_COUNT };
struct ArenaRow {
  int block;
  bool edge; // a block of edge i (false: of node i)
  Dim rows, cols;
};
struct ItemDims {
  long d[D_COUNT];
};

// include/sip_kkt_amd.h: "model arena"
constexpr ArenaRow MODEL_ARENA[] = {
    {N_Q, false, D_NODE, D_NODE},     {N_JC, false, D_NODE_C, D_NODE},  {N_JG, false, D_NODE_G, D_NODE},
    {E_Q, true, D_PARENT, D_PARENT},  {E_M, true, D_PARENT, D_M},       {E_R, true, D_M, D_M},
    {E_A, true, D_CHILD, D_PARENT},   {E_B, true, D_CHILD, D_M},        {E_JXC, true, D_EDGE_C, D_PARENT},
    {E_JUC, true, D_EDGE_C, D_M},     {E_JXG, true, D_EDGE_G, D_PARENT}, {E_JUG, true, D_EDGE_G, D_M}};
// "first-order arena" (types.hpp:48-89, first-order fields)
constexpr ArenaRow FIRST_ORDER_ARENA[] = {
    {FO_N_F, false, D_ONE, D_ONE},    {FO_N_DX, false, D_NODE, D_ONE},  {FO_N_DTH, false, D_THETA, D_ONE},
    {FO_N_C, false, D_NODE_C, D_ONE}, {FO_N_G, false, D_NODE_G, D_ONE}, {FO_E_F, true, D_ONE, D_ONE},
    {FO_E_DX, true, D_PARENT, D_ONE}, {FO_E_DU, true, D_M, D_ONE},      {FO_E_DTH, true, D_THETA, D_ONE},
    {FO_E_DYN, true, D_CHILD, D_ONE}, {FO_E_C, true, D_EDGE_C, D_ONE},  {FO_E_G, true, D_EDGE_G, D_ONE}};
// "theta arena": every block rows x theta_dim
constexpr ArenaRow THETA_ARENA[] = {
    {TH_N_X, false, D_NODE, D_THETA},   {TH_N_C, false, D_NODE_C, D_THETA}, {TH_N_G, false, D_NODE_G, D_THETA},
    {TH_N_TT, false, D_THETA, D_THETA}, {TH_E_X, true, D_PARENT, D_THETA},  {TH_E_U, true, D_M, D_THETA},
    {TH_E_DYN, true, D_CHILD, D_THETA}, {TH_E_C, true, D_EDGE_C, D_THETA},  {TH_E_G, true, D_EDGE_G, D_THETA},
    {TH_E_TT, true, D_THETA, D_THETA}};

// What the selectors stand for at node i and (i < E) edge i of the plan.
inline ItemDims item_dims(const sip_kkt_plan &p, const int i, const int th) {
  ItemDims it{};
  it.d[D_ONE] = 1, it.d[D_THETA] = th;
  it.d[D_NODE] = p.sd[i], it.d[D_NODE_C] = p.ncd[i], it.d[D_NODE_G] = p.ngd[i];
  if (i < p.E) {
    it.d[D_PARENT] = p.sd[p.parents[i]], it.d[D_CHILD] = p.sd[p.children[i]], it.d[D_M] = p.cd[i];
    it.d[D_EDGE_C] = p.ecd[i], it.d[D_EDGE_G] = p.egd[i];
  }
  return it;
}

// Lays one item out from `at`: start[block] of the node's blocks and (with_edge) the edge's; returns its end.
template <size_t R>
long walk_item(const ArenaRow (&table)[R], const ItemDims &it, const bool with_edge, long at, long *start) {
  for (const ArenaRow &r : table)
    if (!r.edge || with_edge)
      start[r.block] = at, at += it.d[r.rows] * it.d[r.cols];
  return at;
}

// off[block][i] of every block of the arena for theta_dim = th; returns the arena's length (doubles per problem).
template <size_t R, size_t B>
long walk_arena(const sip_kkt_plan &p, const ArenaRow (&table)[R], const int th, std::vector<long> (&off)[B]) {
  for (auto &v : off)
    v.assign(p.N, 0);
  long at = 0, start[B] = {};
  for (int i = 0; i < p.N; ++i) {
    at = walk_item(table, item_dims(p, i, th), i < p.E, at, start);
    for (const ArenaRow &r : table)
      if (!r.edge || i < p.E)
        off[r.block][i] = start[r.block];
  }
  return at;
}

// The arithmetic form the chain kernels address an arena by: E stages of one length (an interior node, its edge),
// the blocks of stage i at i * stage + their start within a stage, then the terminal node.  True when `off` / `len`
// is that for the chain's interior (those of node 0, edge 0: decide_paths takes ck from them) and terminal dimensions.
template <size_t R, size_t B>
bool arena_is_uniform(const sip_kkt_plan &p, const ArenaRow (&table)[R], const int th,
                      const std::vector<long> (&off)[B], const long len) {
  long in_stage[B] = {}, in_last[B] = {};
  const long stage = p.E > 0 ? walk_item(table, item_dims(p, 0, th), true, 0, in_stage) : 0;
  if (p.E < 1 || len != p.E * stage + walk_item(table, item_dims(p, p.E, th), false, 0, in_last))
    return false;
  for (int i = 0; i < p.N; ++i)
    for (const ArenaRow &r : table)
      if ((!r.edge || i < p.E) && off[r.block][i] != i * stage + (i < p.E ? in_stage : in_last)[r.block])
        return false;
  return true;
}

// populate_workspace_metadata, types.cpp:24-64: the flattened x | y | z vectors (their own order: x by stage, y and
// z nodes first).  Returns, per y row, 1 where it is a dynamics row.
inline std::vector<int> vector_layout(sip_kkt_plan &p) {
  const int E = p.E, N = p.N;
  for (auto &v : p.voff)
    v.assign(N, 0);
  int xo = 0, yo = 0, zo = 0;
  for (int i = 0; i < N; ++i) {
    p.voff[SIP_KKT_X_STATE][i] = xo, xo += p.sd[i];
    if (i < E)
      p.voff[SIP_KKT_X_CONTROL][i] = xo, xo += p.cd[i];
  }
  std::vector<int> y_is_dyn;
  for (int i = 0; i < N; ++i) {
    p.voff[SIP_KKT_Y_DYN][i] = yo, yo += p.sd[i], y_is_dyn.resize(yo, 1);
    p.voff[SIP_KKT_Y_NODE_C][i] = yo, yo += p.ncd[i], y_is_dyn.resize(yo, 0);
    p.voff[SIP_KKT_Z_NODE][i] = zo, zo += p.ngd[i];
  }
  for (int e = 0; e < E; ++e) {
    p.voff[SIP_KKT_Y_EDGE_C][e] = yo, yo += p.ecd[e];
    p.voff[SIP_KKT_Z_EDGE][e] = zo, zo += p.egd[e];
  }
  y_is_dyn.resize(yo, 0);
  p.x_dim = xo, p.y_dim = yo, p.z_dim = zo;
  return y_is_dyn;
}

// Takes over a first-order layout (walk_arena of FIRST_ORDER_ARENA for theta_dim = th) once its table is on the
// device.  chain_kernels plans get the arithmetic form of it: such a plan is a uniform chain with root 0 and uniform
// constraint dimensions (is_uniform_chain, uniform_constraints), for which the walks of this file give exactly the
// offsets gather_first_order_uniform computes, in the arena and in the x | y | z vectors -- the check cannot fail.
inline void first_order_commit(sip_kkt_plan &p, const int th, std::vector<long> (&off)[FO_NUM_BLOCKS], const long len) {
  for (int b = 0; b < FO_NUM_BLOCKS; ++b)
    p.foff[b].swap(off[b]);
  p.first_len = len;
  p.fo_uniform = p.chain_kernels && arena_is_uniform(p, FIRST_ORDER_ARENA, th, p.foff, len);
  if (!p.chain_kernels)
    return;
  const ChainKkt &ck = p.ck;
  FoUniform fu{};
  fu.n = ck.n, fu.m = ck.m, fu.T = ck.T, fu.p = th;
  fu.cn = ck.cn, fu.gn = ck.gn, fu.cT = ck.cT, fu.gT = ck.gT, fu.ce = ck.ce, fu.ge = ck.ge;
  fu.x_dim = p.x_dim, fu.y_dim = p.y_dim, fu.z_dim = p.z_dim, fu.len = len;
  p.fu = fo_uniform_derive(fu);
}

// ---- workspaces ----
inline WorkOffsets work_offsets(const sip_kkt_plan &p) {
  const size_t B = (size_t)p.batch * sizeof(double);
  Take take;
  WorkOffsets o{};
  o.in0 = take(B * (size_t)p.in0_len);
  o.in1 = p.chain ? take(B * (size_t)p.in1_len) : o.in0; // the tree arena holds q, r, c too
  o.out = take(B * (size_t)p.out_len);
  o.gain = take(B * (size_t)p.gain_len);
  o.inv = take(B * (size_t)(p.y_dim + p.z_dim));
  o.reg = take((size_t)p.batch * sizeof(int));
  o.lqr = take(p.lqr_bytes);
  o.tree_scratch = take(p.tree_scratch_bytes);
  o.end = take.cur;
  return o;
}

// doubles per problem and column of the right-hand-side / solution columns of the multi-rhs solve
inline size_t theta_col_scalars(const sip_kkt_plan &p) {
  return p.chain_kernels ? (size_t)p.in1_len : p.tree_theta_multi ? sip_lqr_tree_rhs_len(p.tree) : 0;
}

inline ThetaWorkOffsets theta_work_offsets(const sip_kkt_plan &p) {
  const size_t skkt = (size_t)p.x_dim + p.y_dim + p.z_dim, th = (size_t)p.theta_dim;
  const size_t B = (size_t)p.batch * sizeof(double);
  Take take;
  ThetaWorkOffsets o{};
  // (the fused chain passes keep stage partials here instead of J_theta: S_part (N p^2) then d_part (N p) per problem)
  o.J = take(B * (p.chain_theta ? (size_t)p.N * (th * th + th) : skkt * th));
  o.KJ = take(B * skkt * th);
  o.S = take(B * th * th);
  o.rhs_sw = take(B * skkt);
  o.sol_sw = take(B * skkt);
  o.vecs_cols = take(B * theta_col_scalars(p) * th);
  o.lsol_cols = take(B * theta_col_scalars(p) * th);
  o.cws = take(p.chain_kernels      ? sip_lqr_solve_multi_workspace_bytes(p.chain, p.theta_dim)
               : p.tree_theta_multi ? sip_lqr_tree_solve_multi_scratch_bytes(p.tree, p.theta_dim)
                                    : 0);
  o.end = take.cur;
  return o;
}

// ---- paths ----
// The environment, read whenever a plan is created or given its theta (tests change it between plans).
struct KktEnv {
  bool direct, tables; // SIP_KKT_VARIANT=direct: no LDS staging; =tables: no chain kernels
  int pipe;            // SIP_KKT_PIPE: stages per wavefront of the pipelined condensation (6), <= 0 off
  bool family, split, sym, theta_fused, theta_tree_multi; // SIP_KKT_<NAME>=0 clears it
};
inline KktEnv kkt_env() {
  auto on = [](const char *key) {
    const char *v = std::getenv(key);
    return !(v != nullptr && v[0] == '0');
  };
  const char *variant = std::getenv("SIP_KKT_VARIANT"), *pipe = std::getenv("SIP_KKT_PIPE");
  return {variant && std::strcmp(variant, "direct") == 0, variant && std::strcmp(variant, "tables") == 0,
          pipe ? std::atoi(pipe) : 6, on("SIP_KKT_FAMILY"), on("SIP_KKT_SPLIT"), on("SIP_KKT_SYM"),
          on("SIP_KKT_THETA_FUSED"), on("SIP_KKT_THETA_TREE_MULTI")};
}

// staged, chain_kernels (and ck), chain_pipe, k, chain_split, chain_sym of a plan whose layouts and back end stand.
inline void decide_paths(sip_kkt_plan &p, const KktEnv &env) {
  const int E = p.E;
  p.k = find_kkt_chain_kernels(0, 0);
  // what the LDS partitions of the staged kernels are made of (kkt_kernels.hpp: kkt::condense_staged_lds, ...)
  Meta &mt = p.meta;
  mt.lds_q = mt.lds_item = mt.lds_tail = 0, mt.lds_rows = 1;
  for (int i = 0; i < p.N; ++i) {
    const int n = p.sd[i], cg = p.ncd[i] + p.ngd[i];
    mt.lds_q = std::max(mt.lds_q, n * n), mt.lds_item = std::max(mt.lds_item, n * n + cg * n);
    mt.lds_tail = std::max(mt.lds_tail, cg * n), mt.lds_rows = std::max(mt.lds_rows, std::max(cg, n));
  }
  for (int e = 0; e < E; ++e) {
    const int n = p.sd[p.parents[e]], nc = p.sd[p.children[e]], m = p.cd[e], cg = p.ecd[e] + p.egd[e];
    mt.lds_item = std::max(mt.lds_item, n * n + n * m + m * m + nc * n + nc * m + cg * (n + m));
    mt.lds_tail = std::max(mt.lds_tail, cg * (n + m)), mt.lds_rows = std::max(mt.lds_rows, std::max(cg, m));
  }
  p.staged = lds_bytes(condense_staged_lds(p.meta)) <= 48 * 1024 && !env.direct;
  if (p.chain == nullptr || !p.staged || !uniform_constraints(p))
    return;
  ChainKkt &ck = p.ck;
  ck.n = p.sd[0], ck.m = p.cd[0], ck.T = E;
  ck.cn = p.ncd[0], ck.gn = p.ngd[0]; // (E = 1: the one interior node's)
  ck.cT = p.ncd[E], ck.gT = p.ngd[E], ck.ce = p.ecd[0], ck.ge = p.egd[0];
  ck.split = 0, ck.sym = 0;
  ck = chain_kkt_derive(ck);
  ck.model_len = p.model_len, ck.x_dim = p.x_dim, ck.y_dim = p.y_dim, ck.z_dim = p.z_dim;
  ck.mats_len = p.in0_len, ck.vecs_len = p.in1_len;
  // lane maps of the chain kernels: state rows on lanes 0..n-1, control rows on lanes 32..32+m-1
  p.chain_kernels = lds_bytes(condense_lds(ck, true, 1)) <= 48 * 1024 && ck.n <= 32 && ck.m <= 32 && !env.tables;
  if (!p.chain_kernels)
    return;
  // software-pipelined condensation (SIP_KKT_PIPE = stages per wavefront, 0 = off): the stage image must be one
  // pass of 16-byte pieces at every stage
  // (any lengths: an image of odd length takes one more piece, whose second half is the first scalar of the item
  // behind it; sources are then only 8-byte aligned, which the vector loads take.  The batch's very last item has
  // nothing behind it: launch_condense gives the last problem to the one-stage kernel when that matters.)
  const int len_mid = ck.node_len + ck.edge_len, len_last = ck.n * ck.n + (ck.cT + ck.gT) * ck.n;
  const bool fits = (len_mid + 1) / 2 <= PIPE_U * TPB && (len_last + 1) / 2 <= PIPE_U * TPB;
  p.chain_pipe = fits && env.pipe > 0 ? env.pipe : 0;
  const int fc = family_c(ck.n), fg = family_g(ck.m);
  if (ck.cn == 0 && ck.gn == 0 && ck.cT == fc && ck.gT == fg && ck.ce == fc && ck.ge == fg && env.family)
    p.k = find_kkt_chain_kernels(ck.n, ck.m);
  p.chain_split = E > 0 && sip_lqr_has_split(p.chain) == 1 && env.split;
  if (p.chain_split && env.sym &&
      (sip_lqr_plan_create_layout(SIP_LQR_F64, p.batch, E, p.sd[0], p.cd[0], p.device, SIP_LQR_LAYOUT_SYMMETRIC,
                                  &p.chain_sym) != SIP_LQR_OK ||
       sip_lqr_has_split(p.chain_sym) != 1 ||
       sip_lqr_workspace_bytes(p.chain_sym) > sip_lqr_workspace_bytes(p.chain))) { // (shares the sweep's scratch)
    sip_lqr_plan_destroy(p.chain_sym);
    p.chain_sym = nullptr;
  }
}

// chain_theta (and ct), tree_theta_multi of a plan whose theta arena stands.  (As with the first-order arena, the
// arithmetic form always holds for a chain_kernels plan; the LDS tests and the environment decide.)
inline void decide_theta_paths(sip_kkt_plan &p, const KktEnv &env) {
  if (p.chain_kernels && p.E >= 1) {
    p.ct.p = p.theta_dim, p.ct.theta_len = p.theta_len;
    p.ct = chain_theta_derive(p.ck, p.ct);
    p.chain_theta = arena_is_uniform(p, THETA_ARENA, p.theta_dim, p.toff, p.theta_len) &&
                    theta_rhs_lds(p.ck, p.ct).total() <= LDS_DOUBLES &&
                    theta_recover_lds(p.ck, p.ct).total() <= LDS_DOUBLES && env.theta_fused;
  }
  p.tree_theta_multi = p.tree != nullptr && env.theta_tree_multi;
}

// The name of a valid plan: its back end's kernel, then what the flags chose.
inline std::string plan_name(const sip_kkt_plan &p) {
  std::string name = p.chain        ? std::string("chain:") + sip_lqr_kernel_name(p.chain)
                     : p.tree_fused ? std::string("tree:fused ") + sip_lqr_tree_split_kernel_name(p.tree)
                                    : std::string("tree:general");
  // (the split form of a chain kernel is the plain kernel's: what the fused sweep of sip_lqr_factor_solve parks in
  // registers -- the ",park" at the end of its name -- says nothing about a step that runs the split form)
  const std::string park = ",park";
  if (p.chain && p.chain_split && name.size() >= park.size() && name.compare(name.size() - park.size(), park.size(), park) == 0)
    name.erase(name.size() - park.size());
  name += p.chain_kernels ? " + chain condensation" : p.staged ? " + staged condensation" : " + direct condensation";
  if (p.chain_split)
    name += p.chain_sym != nullptr ? " (A|B in place, Q|R packed)" : " (A|B in place)";
  if (p.k->n > 0)
    name += " [benchmark-family instantiation]";
  if (p.chain_theta)
    name += " + fused theta passes";
  if (p.tree_theta_multi)
    name += " + tree multi-rhs";
  return name;
}

} // namespace kkt
} // namespace sipamd
