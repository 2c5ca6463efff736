// kkt_first_order_kernels.hpp -- f, grad f, c, g from the first-order model outputs
// (sip_kkt_gather_first_order, include/sip_kkt_amd.h): what the reference's model_callback wrapper
// assembles on the host after every model evaluation, sip_optimal_control.cpp:47-125.
//
//   gather_first_order_tree     any tree, per-node dimensions: offset tables          :56-125
//   gather_first_order_uniform  uniform chains: arithmetic offsets, one stage a wave  :56-125
//   gather_first_order_sums     f and the theta rows of grad f, either form           :47-53, 65-68, 83-86
//
// Gather form, no atomics: every output entry is produced by one lane, which adds its terms in the
// reference's order (a node's df_dx, then the df_dx of its child edges in increasing edge index; nodes
// 0..N-1 then edges 0..E-1 for f and theta).  The reference accumulates into a zero-filled vector, so a
// lane starts from 0.0 too (0.0 + -0.0 is +0.0).  Plain fp64 adds and one subtraction: nothing to contract,
// the results are those of the reference bit for bit.
//
// One wavefront per work item, four items to a workgroup, items of one problem next to each other: the
// lanes of a wavefront read consecutive doubles of one first-order block and write consecutive doubles of
// the flattened vector (512 bytes per full wavefront access), and neighbouring wavefronts continue where
// the last one ended.  Blocks are only 8-byte aligned (odd dimensions), so every access is 8 bytes.
#pragma once
#include <hip/hip_runtime.h>

#include "kkt_kernels.hpp"

namespace sipamd {
namespace kkt {

enum FirstOrderBlock {
  FO_N_F = 0, FO_N_DX, FO_N_DTH, FO_N_C, FO_N_G, FO_E_F, FO_E_DX, FO_E_DU, FO_E_DTH, FO_E_DYN, FO_E_C, FO_E_G,
  FO_NUM_BLOCKS
};

constexpr int FO_TPB = 256, FO_WAVES = FO_TPB / 64;

// Table form: block b of node / edge k starts at tab[b * N + k] (N entries per block; the edge blocks use E).
struct FoTables {
  const long *tab;
  long len; // doubles per problem
  int p;    // theta_dim
};

// Uniform chain (sip_kkt_plan::chain_kernels): stage i < T is node i | edge i, the terminal node follows.
struct FoUniform {
  int n, m, T, p;
  int cn, gn, cT, gT, ce, ge; // constraint rows: interior nodes, terminal node, edges
  int node_len, edge_len;     // of an interior stage: 1 + n + p + cn + gn, 1 + 2 n + m + p + ce + ge
  int x_dim, y_dim, z_dim;    // stagewise (theta excluded)
  long len;                   // doubles per problem
};
// The fields of a FoUniform that follow from its dimensions (n, m, p, cn, gn, ce, ge): the lengths of an interior
// stage's two items.  The lengths of whole arenas (x / y / z_dim, len) are the plan's and travel as they are.
constexpr FoUniform fo_uniform_derive(FoUniform fu) {
  fu.node_len = 1 + fu.n + fu.p + fu.cn + fu.gn;
  fu.edge_len = 1 + 2 * fu.n + fu.m + fu.p + fu.ce + fu.ge;
  return fu;
}

// Work items (problem, node) and (problem, edge); item < N is a node.
__global__ void __launch_bounds__(FO_TPB)
gather_first_order_tree(const Meta mt, const FoTables ft, const double *__restrict__ first_all,
                        const double *__restrict__ x_all, const double *__restrict__ init_all,
                        double *__restrict__ grad_all, double *__restrict__ c_all, double *__restrict__ g_all,
                        const long batch) {
  const int lane = threadIdx.x & 63;
  const int items = mt.N + mt.E;
  const long at = (long)blockIdx.x * FO_WAVES + (threadIdx.x >> 6);
  if (at >= batch * items)
    return;
  const long q = at / items;
  const int item = (int)(at - q * items);
  const long xt = (long)mt.x_dim + ft.p;
  const double *fo = first_all + q * ft.len;
  double *grad = grad_all + q * xt, *c = c_all + q * mt.y_dim, *g = g_all + q * mt.z_dim;
  const long *tab = ft.tab;
  const int N = mt.N;
  if (item < N) {
    const int v = item, n = mt.sd[v];
    const double *dx = fo + tab[FO_N_DX * N + v];
    const int lo = mt.child_offsets[v], hi = mt.child_offsets[v + 1];
    double *gx = grad + mt.x_state[v];
    for (int r = lane; r < n; r += 64) {
      double acc = 0.0;
      acc += dx[r]; // :61-64
      for (int ci = lo; ci < hi; ++ci) // :75-78, the edges whose parent is v, in edge order
        acc += fo[tab[FO_E_DX * N + mt.child_edges[ci]] + r];
      gx[r] = acc;
    }
    double *cd = c + mt.y_dyn[v];
    if (v == mt.root) { // :93-97
      const double *init = init_all + q * n, *xr = x_all + q * xt + mt.x_state[v];
      for (int r = lane; r < n; r += 64)
        cd[r] = init[r] - xr[r];
    } else if (mt.in_edge[v] >= 0) { // :105-107, written by the edge that ends here
      const double *dyn = fo + tab[FO_E_DYN * N + mt.in_edge[v]];
      for (int r = lane; r < n; r += 64)
        cd[r] = dyn[r];
    }
    const double *nc = fo + tab[FO_N_C * N + v], *ng = fo + tab[FO_N_G * N + v];
    double *cc = c + mt.y_node_c[v], *gg = g + mt.z_node[v];
    for (int r = lane; r < mt.ncd[v]; r += 64) // :99-101
      cc[r] = nc[r];
    for (int r = lane; r < mt.ngd[v]; r += 64) // :116-118
      gg[r] = ng[r];
  } else {
    const int e = item - N;
    const double *du = fo + tab[FO_E_DU * N + e], *ec = fo + tab[FO_E_C * N + e], *eg = fo + tab[FO_E_G * N + e];
    double *gu = grad + mt.x_control[e], *cc = c + mt.y_edge_c[e], *gg = g + mt.z_edge[e];
    for (int r = lane; r < mt.cd[e]; r += 64) { // :79-82
      double acc = 0.0;
      acc += du[r];
      gu[r] = acc;
    }
    for (int r = lane; r < mt.ecd[e]; r += 64) // :108-110
      cc[r] = ec[r];
    for (int r = lane; r < mt.egd[e]; r += 64) // :121-123
      gg[r] = eg[r];
  }
}

// Work items (problem, stage): node i and, for i < T, edge i.  Everything a stage writes it reads from its own
// piece of the arena (the dyn rows of node i + 1 are edge i's dyn_res), except the root rows of c.  The outputs of a
// stage are numbered through -- state rows | control rows | node c | dyn rows of the child | edge c | node g |
// edge g | (stage 0) root rows of c -- and dealt to the lanes in that order: at the benchmark shapes one pass, with
// every load of the stage in flight at once.
__global__ void __launch_bounds__(FO_TPB)
gather_first_order_uniform(const FoUniform fu, const double *__restrict__ first_all,
                           const double *__restrict__ x_all, const double *__restrict__ init_all,
                           double *__restrict__ grad_all, double *__restrict__ c_all,
                           double *__restrict__ g_all, const long batch) {
  const int lane = threadIdx.x & 63;
  const int N = fu.T + 1;
  const long at = (long)blockIdx.x * FO_WAVES + (threadIdx.x >> 6);
  if (at >= batch * N)
    return;
  const long q = at / N;
  const int i = (int)(at - q * N);
  const int n = fu.n, p = fu.p, T = fu.T;
  const bool last = i == T;
  const long xt = (long)fu.x_dim + p;
  const double *node = first_all + q * fu.len + (long)i * (fu.node_len + fu.edge_len);
  // rows of this stage: the terminal node has its own constraint rows and no edge
  const int cn = last ? fu.cT : fu.cn, gn = last ? fu.gT : fu.gn;
  const int m = last ? 0 : fu.m, nd = last ? 0 : n, ce = last ? 0 : fu.ce, ge = last ? 0 : fu.ge, nr = i == 0 ? n : 0;
  const double *ndx = node + 1, *nc = ndx + n + p, *ng = nc + cn;
  const double *edx = node + fu.node_len + 1, *edu = edx + n, *edyn = edu + fu.m + p, *ec = edyn + n, *eg = ec + fu.ce;
  double *gx = grad_all + q * xt + (long)i * (n + fu.m);
  double *c = c_all + q * fu.y_dim, *g = g_all + q * fu.z_dim;
  double *cnode = c + (long)i * (n + fu.cn); // dyn_i | node_c_i
  double *cedge = c + (long)N * n + (long)T * fu.cn + fu.cT + (long)i * fu.ce;
  double *gnode = g + (long)i * fu.gn, *gedge = g + (long)T * fu.gn + fu.gT + (long)i * fu.ge;
  const int rows = n + m + cn + nd + ce + gn + ge + nr;
  enum { COPY, ADD, SUB };
  for (int t = lane; t < rows; t += 64) {
    int r = t, op = COPY;
    const double *a, *b = nullptr;
    double *out;
    if (r < n)
      a = ndx + r, b = last ? nullptr : edx + r, out = gx + r, op = ADD; // :61-64, 75-78
    else if ((r -= n) < m)
      a = edu + r, out = gx + n + r, op = ADD; // :79-82
    else if ((r -= m) < cn)
      a = nc + r, out = cnode + n + r; // :99-101
    else if ((r -= cn) < nd)
      a = edyn + r, out = cnode + (n + fu.cn) + r; // :105-107
    else if ((r -= nd) < ce)
      a = ec + r, out = cedge + r; // :108-110
    else if ((r -= ce) < gn)
      a = ng + r, out = gnode + r; // :116-118
    else if ((r -= gn) < ge)
      a = eg + r, out = gedge + r; // :121-123
    else
      r -= ge, a = init_all + q * n + r, b = x_all + q * xt + r, out = c + r, op = SUB; // :93-97
    double v = *a;
    const double w = b != nullptr ? *b : 0.0;
    if (op == ADD)
      v = (0.0 + v) + w; // (+ 0.0 where there is no second term: 0.0 + v is never -0.0, so it changes nothing)
    else if (op == SUB)
      v = v - w;
    *out = v;
  }
}

// One lane per (problem, component): component 0 is f, component k > 0 row k - 1 of theta (`comps` = 1 when only
// f is asked for).  The lane runs its 2 E + 1 dependent adds in the reference's order; its reads are 8 bytes out
// of a line each, a stage apart from one add to the next.
template <bool UNIFORM>
__global__ void __launch_bounds__(FO_TPB)
gather_first_order_sums(const FoUniform fu, const FoTables ft, const int N, const int x_dim, const int comps,
                        const double *__restrict__ first_all, double *__restrict__ f_all,
                        double *__restrict__ grad_all, const long batch) {
  const long at = (long)blockIdx.x * FO_TPB + threadIdx.x;
  if (at >= batch * comps)
    return;
  const long q = at / comps;
  const int k = (int)(at - q * comps);
  const int E = N - 1;
  double acc = 0.0;
  if (UNIFORM) {
    const long stage = fu.node_len + fu.edge_len;
    const double *node = first_all + q * fu.len + (k == 0 ? 0 : fu.n + k);
    const double *edge = first_all + q * fu.len + fu.node_len + (k == 0 ? 0 : fu.n + fu.m + k);
#pragma unroll 4
    for (int i = 0; i < N; ++i)
      acc += node[i * stage];
#pragma unroll 4
    for (int e = 0; e < E; ++e)
      acc += edge[e * stage];
  } else {
    const double *fo = first_all + q * ft.len + (k == 0 ? 0 : k - 1);
    const long *tn = ft.tab + (k == 0 ? FO_N_F : FO_N_DTH) * N, *te = ft.tab + (k == 0 ? FO_E_F : FO_E_DTH) * N;
#pragma unroll 4
    for (int i = 0; i < N; ++i)
      acc += fo[tn[i]];
#pragma unroll 4
    for (int e = 0; e < E; ++e)
      acc += fo[te[e]];
  }
  if (k == 0)
    f_all[q] = acc;
  else
    grad_all[q * ((long)x_dim + (comps - 1)) + x_dim + (k - 1)] = acc;
}

} // namespace kkt
} // namespace sipamd
