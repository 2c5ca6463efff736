// tree_residual.hpp -- the residual of the tree KKT system on the tree-native arenas (include/sip_lqr_amd.h, second
// half), in fp64, for NC right-hand sides and iterates against one `input`: the kernel of sip_lqr_tree_residual and of
// the rounds of sip_lqr_tree_refine (one column: its NC = 1 instantiation) and of sip_lqr_tree_residual_multi and
// sip_lqr_tree_refine_multi (several, laid out as sip_lqr_tree_solve_multi lays its columns out: column c of a
// whole-batch array at c * batch * out_len scalars).
//
//   rho_q[i]        = Q_i x_i - y_i + q_i + sum over the child edges e of i, in child_edges order, of
//                     (M_e u_e + A_e^T y_child(e))
//   rho_c[root]     = -x_root - delta_root o y_root + c_root
//   rho_c[child(e)] = A_e x_parent(e) + B_e u_e - x_child - delta_child o y_child + c_child
//   rho_r[e]        = M_e^T x_parent(e) + R_e u_e + B_e^T y_child + r_e
//
// in the layout of a right-hand side of sip_lqr_tree_solve_multi (the output arena's: rho_q | rho_c where x | y are,
// rho_r where u is), so a solve on rho returns d with K (z + d) + b = 0.  Q and R are taken symmetric from their lower
// triangles, as the reference's selfadjointView<Lower> does.  Dimensions are read from tree::Meta at run time; any of
// them may be 0.
//
// Shape: one workgroup per problem, its wavefronts taking nodes in turn (nothing ties the nodes).  The wavefront of
// node i computes what reads the blocks of i and of its child edges: rho_q[i], and per child edge e, in CSR order,
// rho_r[e] and rho_c[child(e)] (the root's wavefront: rho_c[root] too) -- so every block of the input arena is fetched
// once, and the sum over the children of a node has one order: no atomics, the same bits on every run.  A node with
// many children (the root of a shallow wide tree) would keep one wavefront busy with all of them while the others
// finish: for such a tree, where its parts fit LDS, the wavefronts take nodes and edges alike (SPLIT, below).
// Per item -- the node, then each child edge -- the matrices (Q; A | B | M | R, contiguous in the arena) go through LDS
// by 16-byte loads, kCopyUnroll per lane in flight, from the 16-byte piece that holds the item's first scalar (a block
// at an odd 8-byte offset has one scalar of lead-in, the odd tail goes by a scalar, as in chain_residual.hpp), so the
// transposed products A^T y, B^T y, M^T x read columns out of LDS.  Where the largest item's matrices do not fit a
// wavefront's share of LDS the host picks STAGED = false for the plan and the matrices are read in place.
// Per wavefront the LDS holds (tree_residual_cols_shape.hpp)
//   node part  x_i | y_i | q_i | acc head | acc tail   z[k][c], max_n NC doubles each
//   edge part  (SPLIT: x_p |) u | x_c | y_c | r | c_c  z[k][c], packed by the edge's dims, then delta_c[k] once
// with the NC columns of one entry adjacent: a term's NC operands are one or more 16-byte LDS reads.  The vectors are
// gathered as single doubles, kGatherUnroll per lane in flight; the gather deals (k, c) pairs to lanes with c fastest,
// so that its LDS writes are contiguous.
//
// Every row of a result is one dot product against the gathered vectors, summed as a head + tail pair (Pair, below),
// kParts lanes to a row; per lane blocks of kDotUnroll terms through the same three segments (a block's terms are
// loaded cols_tree_dot_unroll<NC>() at a time, which changes no operation and no order); a lane loads a matrix entry
// once per term and issues NC pair-FMAs into NC Pair accumulators, since what the kernel is otherwise bound by (DESIGN
// 4.10.1: gather addresses, the staging pass, row descriptors, loop control) does not depend on the right-hand side.
// The partial sums meet by two shuffle joins; a join takes the lower lane's pair first on both lanes, so after the two
// joins the kParts lanes of a row all hold the same pair, and lane `part` closes and stores the columns c with
// c % kParts == part.  rho_q[i] collects the contributions of the edges in LDS: Q x first, then the child edges in CSR
// order, in both forms.  Column c is the same bits whatever NC it is computed at.
//
// A launch of the NC instantiation may carry ncols < NC columns: a masked column reads the last real column again (in
// bounds, and no branch among the loads) and stores nothing: no residual, no norm, no scale.
// The norm and the scaled form are those of the chain kernel, whose helpers (nan_max, lds_order, pow2_scale, load_cols)
// and update kernel this one shares.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "chain_residual.hpp"
#include "tree_generic.hpp"
#include "tree_residual_cols_shape.hpp"

namespace sipamd {
namespace residual {

// Every entry of the result is summed as an unevaluated pair head + tail of doubles (Ogita, Rump, Oishi, Accurate sum
// and dot product, 2005: Dot2), so it comes out as if summed in twice the working precision and rounded once: the
// residual of a nearly solved system is all cancellation, and a refinement round can only remove the error the
// residual can see.  The transformations are exact only as written: no contraction of a * b + c inside them.
struct Pair {
  double h, l;
};
// s + e == a + b exactly (Knuth)
__device__ __forceinline__ void two_sum(const double a, const double b, double &s, double &e) {
#pragma clang fp contract(off)
  s = a + b;
  const double bb = s - a;
  e = (a - (s - bb)) + (b - bb);
}
// acc += x
__device__ __forceinline__ Pair pair_add(Pair acc, const double x) {
#pragma clang fp contract(off)
  double s, e;
  two_sum(acc.h, x, s, e);
  return {s, acc.l + e};
}
// acc += a * b, the product's rounding error (one FMA) kept
__device__ __forceinline__ Pair pair_fma(Pair acc, const double a, const double b) {
#pragma clang fp contract(off)
  const double p = a * b, pe = __builtin_fma(a, b, -p);
  double s, e;
  two_sum(acc.h, p, s, e);
  return {s, acc.l + (pe + e)};
}
// acc += other
__device__ __forceinline__ Pair pair_join(Pair acc, const Pair other) {
#pragma clang fp contract(off)
  double s, e;
  two_sum(acc.h, other.h, s, e);
  return {s, acc.l + (other.l + e)};
}
__device__ __forceinline__ double total(const Pair v) { return v.h + v.l; }
__device__ __forceinline__ Pair pair_shfl_xor(const Pair v, const int mask) {
  return {__shfl_xor(v.h, mask), __shfl_xor(v.l, mask)};
}

// Terms of a block of kDotUnroll a lane reads out of LDS before it uses the first: at NC = 8 the accumulators alone
// are 16 doubles, and every staged term brings NC more.
template <int NC>
constexpr int cols_tree_dot_unroll() {
  return NC >= 8 ? 1 : (NC >= 4 ? 2 : 4);
}

// rhs_cols, sol_cols, res and scaled point at column 0 of the launch, column c at c * col_stride scalars; norm and
// scale at column 0, column c at c * batch.  res != nullptr or scaled == nullptr: plain form (res may be nullptr: norms
// only); scaled != nullptr: rho / s_{p,c} to `scaled`, s_{p,c} to `scale`.  rhs_cols == nullptr: q, c, r are those of
// `input` for every column; else they are read from it, one column each in the output arena's layout.
// SPLIT: the wavefronts take nodes AND edges in turn, so the children of one node spread over them; an item parks its
// part of rho_q (Q x of a node, M u + A^T y_c of an edge) in LDS, max_n NC doubles per item behind the wavefronts'
// areas, and after a barrier every rho_q[i] is summed from them in the order of the other form: Q x first, then the
// child edges in CSR order -- the same additions, the same bits.  The host picks it where one node's children outnumber
// a wavefront's even share of the items and the parts fit (tree_residual_cols_shape.hpp); elsewhere nodes in turn are
// faster.
template <bool STAGED, bool SPLIT, int NC>
__global__ void __launch_bounds__(kLanes *kTreeColsMaxWaves)
    tree_residual_kernel(const tree::Meta mt, const double *__restrict__ input, const double *__restrict__ rhs_cols,
                         const double *__restrict__ sol_cols, const long launch_col_stride, const long batch,
                         const int launch_ncols, double *__restrict__ res, double *__restrict__ scaled, double *__restrict__ scale,
                         double *__restrict__ norm, const int wave_bytes) {
  static_assert(NC == 1 || NC == 2 || NC == 4 || NC == 8, "columns of an instantiation");
  static_assert(kLanes % NC == 0 && kDotUnroll % cols_tree_dot_unroll<NC>() == 0, "a lane keeps its column");
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  constexpr int LOG = NC == 1 ? 0 : (NC == 2 ? 1 : (NC == 4 ? 2 : 3));
  constexpr int DU = cols_tree_dot_unroll<NC>();
  // One column: there is one column and no stride to it, known at compile time, so the clamps to the last column, the
  // products with the stride and the tests against ncols below are folded away.
  const int ncols = NC == 1 ? 1 : launch_ncols;
  const long col_stride = NC == 1 ? 0 : launch_col_stride;
  const long p = blockIdx.x;
  const int lane = threadIdx.x & (kLanes - 1), wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kLanes);
  const int waves = blockDim.x / kLanes;
  const int part = lane & (kParts - 1);
  const int my_c = lane & (NC - 1); // the column of this lane wherever (k, c) pairs are dealt to lanes
  const int last_col = ncols - 1;
  const int stride_n = mt.max_n << LOG; // between the vectors of the node part
  double *red = (double *)lds;
  unsigned char *mine = lds + tree_cols_red_bytes(NC) + (size_t)wave * wave_bytes;
  double *xi = (double *)mine, *yi = xi + stride_n, *qi = yi + stride_n, *acc_q = qi + stride_n; // acc: head | tail
  double *ze = acc_q + 2 * stride_n;
  double *parts = (double *)(lds + tree_cols_red_bytes(NC) + (size_t)waves * wave_bytes); // SPLIT: [item][2][max_n][NC]
  double *img = (double *)(mine + tree_cols_z_doubles(mt.max_n, mt.max_m, NC) * sizeof(double));
  const double *pin = input + p * mt.in0_len, *ps = sol_cols + p * mt.out_len; // column 0
  const double *pr = rhs_cols != nullptr ? rhs_cols + p * mt.out_len : nullptr;
  const long rhs_stride = pr != nullptr ? col_stride : 0;
  const long my_col = (long)(my_c < last_col ? my_c : last_col) * col_stride; // (a masked column: the last real one)

  // `len` scalars at `src` as blk[0 .. len): through the image, or in place
  auto stage = [&](const double *src, const int len) -> const double * {
    if constexpr (STAGED) {
      if (len == 0)
        return img;
      const int lead = (int)(((uintptr_t)src & 15) / sizeof(double));
      const double *from = src - lead; // 16-byte aligned, inside the arena: the arena itself is aligned
      const int total = lead + len, pieces = total / 2;
      for (int base = 0; base < pieces; base += kLanes * kCopyUnroll) {
        // (a lane past the end loads and stores the last piece again: in bounds, the same value to the same place)
        uint4 r[kCopyUnroll];
        int k[kCopyUnroll];
#pragma unroll
        for (int j = 0; j < kCopyUnroll; ++j) {
          k[j] = base + j * kLanes + lane < pieces ? base + j * kLanes + lane : pieces - 1;
          r[j] = ((const uint4 *)from)[k[j]];
        }
#pragma unroll
        for (int j = 0; j < kCopyUnroll; ++j)
          ((uint4 *)img)[k[j]] = r[j];
      }
      if ((total & 1) && lane == 0) // what is left of the last piece: never past the end
        img[total - 1] = from[total - 1];
      return img + lead;
    } else {
      return src;
    }
  };

  // acc[c] + sum over k < count of blk[at(k)] * z[k][c], this lane's share (k = part, part + kParts, ...), in blocks of
  // kDotUnroll terms (a term past the end: the block's first again, against an entry of 0), DU of them loaded before
  // the first is used; at(k) = base + stride k, or, SYM, element (r, k) of a symmetric dim x dim matrix at `base` of
  // which the lower triangle is read.
  auto segment = [&](auto SYM, const double *blk, Pair(&acc)[NC], const int base, const int stride, const int count,
                     const double *z, const bool sym_lane, const int r, const int dim) {
    for (int k = part; k < count; k += kParts * kDotUnroll) {
#pragma unroll
      for (int j0 = 0; j0 < kDotUnroll; j0 += DU) {
        double a[DU], zz[DU][NC];
#pragma unroll
        for (int j = 0; j < DU; ++j) {
          const int kk = k + (j0 + j) * kParts < count ? k + (j0 + j) * kParts : k;
          int at = base + stride * kk;
          if constexpr (decltype(SYM)::value)
            at = sym_lane ? base + (kk < r ? r + dim * kk : kk + dim * r) : at;
          a[j] = blk[at];
          load_cols<NC>(z + ((size_t)kk << LOG), zz[j]);
        }
#pragma unroll
        for (int j = 0; j < DU; ++j) {
          const double aj = k + (j0 + j) * kParts < count ? a[j] : 0.0; // (a term of 0 changes nothing)
#pragma unroll
          for (int c = 0; c < NC; ++c)
            acc[c] = pair_fma(acc[c], aj, zz[j][c]);
        }
      }
    }
  };
  // the kParts partial sums of a row, the lower lane's first: every lane of the row ends with lane 0's pair.  (One
  // column is closed by lane 0 of the row alone, which is the lower lane of both of its joins.)
  auto join_row = [&](Pair(&acc)[NC]) {
#pragma unroll
    for (int mask = 1; mask < kParts; mask <<= 1) {
      const bool upper = NC > 1 && (lane & mask) != 0;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const Pair other = pair_shfl_xor(acc[c], mask);
        acc[c] = pair_join(upper ? other : acc[c], upper ? acc[c] : other);
      }
    }
  };

  const int passes = scaled != nullptr ? 2 : 1;
  double s_pc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c)
    s_pc[c] = 1.0;
  double s_mine = 1.0; // s_pc[my_c]
  for (int pass = 0; pass < passes; ++pass) {
    const bool want_norm = pass == 0, store = pass == passes - 1;
    double nrm[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c)
      nrm[c] = 0.0;
    auto put = [&](const int c, const long idx, const double v, const double s) {
      const long at = c * col_stride + p * mt.out_len + idx;
      if (scaled != nullptr)
        scaled[at] = v / s;
      else if (res != nullptr)
        res[at] = v;
    };
    // (c is a constant wherever this is called: the loops over columns are unrolled)
    auto emit = [&](const int c, const long idx, const double v) {
      if (want_norm)
        nrm[c] = nan_max(nrm[c], __builtin_fabs(v));
      if (store)
        put(c, idx, v, s_pc[c]);
    };
    // the same for the lane's own column my_c, where (k, c) pairs are dealt to lanes
    auto emit_mine = [&](const long idx, const double v) {
      if (my_c >= ncols)
        return;
      if (want_norm) {
        const double av = __builtin_fabs(v);
#pragma unroll
        for (int c = 0; c < NC; ++c)
          nrm[c] = c == my_c ? nan_max(nrm[c], av) : nrm[c];
      }
      if (store)
        put(my_c, idx, v, s_mine);
    };
    const int items = SPLIT ? mt.num_nodes + mt.num_edges : mt.num_nodes;
    for (int item = wave; item < items; item += waves) {
      const bool node_item = item < mt.num_nodes; // (always, unless SPLIT)
      const int i = node_item ? item : mt.edge_parents[item - mt.num_nodes];
      const int n = mt.state_dims[i];
      const int nl = n << LOG;
      const long ox = mt.ox[i], oy = mt.oy[i];
      const double *q_src = pr != nullptr ? pr + ox : pin + mt.oq[i]; // column 0
      double *q_sink = SPLIT ? parts + (long)item * 2 * stride_n : acc_q, *q_tail = q_sink + stride_n;
      lds_order(); // the previous item's reads of its vectors and of the image are done
      // ---- the node: x_i | y_i | q_i, then rows [0, n) of Q x_i
      if (node_item) {
        // Item t = k * NC + c of a list is entry k of column c and lands at [t]; a lane past the end of the lists
        // loads and stores their last item again; a masked column reads the last real column.
        for (int base = 0; base < 3 * nl; base += kLanes * kGatherUnroll) {
          double r[kGatherUnroll];
          int t[kGatherUnroll];
#pragma unroll
          for (int j = 0; j < kGatherUnroll; ++j) {
            t[j] = base + j * kLanes + lane < 3 * nl ? base + j * kLanes + lane : 3 * nl - 1;
            const int o = t[j] < nl ? t[j] : (t[j] < 2 * nl ? t[j] - nl : t[j] - 2 * nl);
            const int c = o & (NC - 1), k = o >> LOG;
            const long col = c < last_col ? c : last_col;
            const double *src = t[j] < nl ? ps + col * col_stride + ox
                                          : (t[j] < 2 * nl ? ps + col * col_stride + oy : q_src + col * rhs_stride);
            r[j] = src[k];
          }
#pragma unroll
          for (int j = 0; j < kGatherUnroll; ++j) // (xi, yi, qi are stride_n apart)
            (t[j] < nl ? xi : (t[j] < 2 * nl ? yi - nl : qi - 2 * nl))[t[j]] = r[j];
        }
        const double *Q = stage(pin + mt.oQ[i], n * n);
        lds_order();
        for (int w0 = 0; w0 < n * kParts; w0 += kLanes) {
          const int w = w0 + lane, row = w / kParts;
          const bool active = row < n;
          Pair acc[NC];
#pragma unroll
          for (int c = 0; c < NC; ++c)
            acc[c] = Pair{0.0, 0.0};
          segment(std::true_type{}, Q, acc, 0, 0, active ? n : 0, xi, true, row, n);
          join_row(acc);
          if (active) {
#pragma unroll
            for (int c = 0; c < NC; ++c)
              if ((c & (kParts - 1)) == part)
                q_sink[(row << LOG) + c] = acc[c].h, q_tail[(row << LOG) + c] = acc[c].l;
          }
        }
        if (i == mt.root) {
          const double *c_src = (pr != nullptr ? pr + oy : pin + mt.oc[i]) + (my_c < last_col ? my_c : last_col) * rhs_stride;
          const double *d_src = pin + mt.od[i];
          for (int t = lane; t < nl; t += kLanes) { // (t & (NC - 1) == my_c: NC divides kLanes)
            const int r = t >> LOG;
            emit_mine(oy + r, total(pair_add(pair_fma(Pair{-xi[t], 0.0}, -d_src[r], yi[t]), c_src[r])));
          }
        }
      }
      // ---- its child edges, in CSR order; SPLIT: the one edge of an edge item
      const int c_lo = SPLIT ? (node_item ? 0 : item - mt.num_nodes) : mt.child_offsets[i];
      const int c_hi = SPLIT ? (node_item ? 0 : c_lo + 1) : mt.child_offsets[i + 1];
      for (int ci = c_lo; ci < c_hi; ++ci) {
        const int e = SPLIT ? ci : mt.child_edges[ci], ch = mt.edge_children[e];
        const int nc = mt.state_dims[ch], m = mt.control_dims[e];
        const long oA = mt.oA[e], ou = mt.ou[e], oxc = mt.ox[ch], oyc = mt.oy[ch];
        // the matrices of the edge relative to its first block, A
        const int rB = (int)(mt.oB[e] - oA), rM = (int)(mt.oM[e] - oA), rR = (int)(mt.oR[e] - oA);
        const double *r_src = pr != nullptr ? pr + ou : pin + mt.orr[e]; // column 0
        const double *c_src = pr != nullptr ? pr + oyc : pin + mt.oc[ch], *d_src = pin + mt.od[ch];
        // x of the parent: gathered with the edge's vectors, else the node's x_i in LDS
        const int l0 = SPLIT ? nl : 0, lm = m << LOG, ln = nc << LOG;
        const double *xs = SPLIT ? ze : xi;
        double *u = ze + l0, *xc = u + lm, *yc = xc + ln, *re = yc + ln, *cc = re + lm, *dc = cc + ln;
        lds_order(); // the previous item's reads of the edge vectors and of the image are done
        const int zl = l0 + 2 * lm + 3 * ln + nc;
        for (int base = 0; base < zl; base += kLanes * kGatherUnroll) {
          double r[kGatherUnroll];
          int t[kGatherUnroll];
#pragma unroll
          for (int j = 0; j < kGatherUnroll; ++j) {
            t[j] = base + j * kLanes + lane < zl ? base + j * kLanes + lane : zl - 1;
            // (x_p |) u | x_c | y_c | r | c_c, NC columns each, then delta_c once
            int o = t[j];
            const double *src = ps + ox;
            long cs = col_stride;
            bool once = false;
            if (o >= l0) {
              o -= l0, src = ps + ou;
              if (o >= lm) {
                o -= lm, src = ps + oxc;
                if (o >= ln) {
                  o -= ln, src = ps + oyc;
                  if (o >= ln) {
                    o -= ln, src = r_src, cs = rhs_stride;
                    if (o >= lm) {
                      o -= lm, src = c_src;
                      if (o >= ln)
                        o -= ln, src = d_src, cs = 0, once = true;
                    }
                  }
                }
              }
            }
            const int c = o & (NC - 1);
            const long col = c < last_col ? c : last_col;
            r[j] = src[once ? (long)o : col * cs + (o >> LOG)];
          }
#pragma unroll
          for (int j = 0; j < kGatherUnroll; ++j)
            ze[t[j]] = r[j];
        }
        const double *blk = stage(pin + oA, nc * n + nc * m + n * m + m * m);
        lds_order();
        // rows [0, n) of M u + A^T y_c (into rho_q[i]) | [n, n + m) rho_r[e] | [n + m, n + m + nc) rho_c[ch]: three
        // segments each, against x of the parent (n terms), u (m) and y_c (nc); only where a segment's entries start
        // and how far apart they lie differs from row to row.
        const int rows = n + m + nc;
        for (int w0 = 0; w0 < rows * kParts; w0 += kLanes) {
          const int w = w0 + lane, row = w / kParts;
          const bool active = row < rows;
          const bool q_row = row < n, r_row = !q_row && row < n + m;
          const int j = row - n, r = row - n - m; // the row inside rho_r, inside rho_c
          // (base, stride) of the row in: nothing | M^T | A;  M | R | B;  A^T | B^T | nothing
          const int b0 = r_row ? rM + n * j : r, s0 = r_row ? 1 : nc;
          const int b1 = q_row ? rM + row : (r_row ? rR : rB + r), s1 = q_row ? n : nc;
          const int b2 = q_row ? nc * row : rB + nc * j;
          const int c0 = active && !q_row ? n : 0, c1 = active ? m : 0, c2 = active && (q_row || r_row) ? nc : 0;
          Pair acc[NC];
#pragma unroll
          for (int c = 0; c < NC; ++c)
            acc[c] = Pair{0.0, 0.0};
          segment(std::false_type{}, blk, acc, b0, s0, c0, xs, false, 0, 0);
          segment(std::true_type{}, blk, acc, b1, s1, c1, u, r_row, j, m);
          segment(std::false_type{}, blk, acc, b2, 1, c2, yc, false, 0, 0);
          join_row(acc);
          if (active) {
#pragma unroll
            for (int c = 0; c < NC; ++c) {
              if ((c & (kParts - 1)) != part)
                continue;
              if (q_row) {
                const int at = (row << LOG) + c;
                Pair v = acc[c];
                if constexpr (!SPLIT)
                  v = pair_join(Pair{q_sink[at], q_tail[at]}, v);
                q_sink[at] = v.h, q_tail[at] = v.l;
              } else if (c < ncols) {
                if (r_row) {
                  emit(c, ou + j, total(pair_add(acc[c], re[(j << LOG) + c])));
                } else {
                  const int at = (r << LOG) + c;
                  emit(c, oyc + r, total(pair_add(pair_fma(pair_add(acc[c], -xc[at]), -dc[r], yc[at]), cc[at])));
                }
              }
            }
          }
        }
      }
      if constexpr (!SPLIT) {
        lds_order();
        for (int t = lane; t < nl; t += kLanes) // (acc_q[t]: through LDS from the lane that closed row t >> LOG, column my_c)
          emit_mine(ox + (t >> LOG), total(pair_add(pair_add(Pair{acc_q[t], acc_q[stride_n + t]}, -yi[t]), qi[t])));
      }
    }
    if constexpr (SPLIT) { // rho_q[i] from the parts: Q x, then the child edges in CSR order
      __syncthreads();
      for (int i = wave; i < mt.num_nodes; i += waves) {
        const int n = mt.state_dims[i];
        const long ox = mt.ox[i];
        const double *y_src = ps + my_col + mt.oy[i];
        const double *q_src = pr != nullptr ? pr + my_col + ox : pin + mt.oq[i];
        for (int t = lane; t < (n << LOG); t += kLanes) {
          const int r = t >> LOG;
          const double *own = parts + (long)i * 2 * stride_n + t;
          Pair v{own[0], own[stride_n]};
          for (int ci = mt.child_offsets[i]; ci < mt.child_offsets[i + 1]; ++ci) {
            const double *of_edge = parts + (long)(mt.num_nodes + mt.child_edges[ci]) * 2 * stride_n + t;
            v = pair_join(v, Pair{of_edge[0], of_edge[stride_n]});
          }
          emit_mine(ox + r, total(pair_add(pair_add(v, -y_src[r]), q_src[r])));
        }
      }
    }
    if (want_norm) {
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        for (int off = kLanes / 2; off > 0; off >>= 1)
          nrm[c] = nan_max(nrm[c], __shfl_xor(nrm[c], off));
        if (lane == 0)
          red[wave * NC + c] = nrm[c];
      }
      __syncthreads();
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        double all = red[c];
        for (int k = 1; k < waves; ++k)
          all = nan_max(all, red[k * NC + c]);
        s_pc[c] = pow2_scale(all);
        s_mine = c == my_c ? s_pc[c] : s_mine;
        if (threadIdx.x == c && c < ncols) {
          norm[c * batch + p] = all;
          if (scaled != nullptr)
            scale[c * batch + p] = s_pc[c];
        }
      }
    }
  }
}

} // namespace residual
} // namespace sipamd
