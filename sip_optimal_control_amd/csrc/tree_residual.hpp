// tree_residual.hpp -- the residual of the tree KKT system on the tree-native arenas (include/sip_lqr_amd.h, second
// half), in fp64: the kernel of sip_lqr_tree_residual and of the rounds of sip_lqr_tree_refine.
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
// at an odd 8-byte offset has one scalar of lead-in, as in chain_residual.hpp), so the transposed products A^T y,
// B^T y, M^T x read columns out of LDS; the vectors of the item (x, y, u of the iterate; q, c, r, delta) are gathered
// as single doubles, kGatherUnroll per lane in flight.  Where the largest item's matrices do not fit a wavefront's
// share of LDS the host picks STAGED = false for the plan and the matrices are read in place.  Every row of a result is
// one dot product against the gathered vectors, summed as a head + tail pair (Pair, below), kParts lanes to a row, their
// partial sums meeting by two shuffles;
// rho_q[i] collects the contributions of the edges in LDS.  The norm and the scaled form are those of the chain
// kernel, whose helpers (nan_max, lds_order, pow2_scale) and update kernel this one shares.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "chain_residual.hpp"
#include "tree_generic.hpp"

namespace sipamd {
namespace residual {

// LDS of one wavefront, in doubles: the node's x | y | q and the running rho_q as head | tail (5 max_n), then the
// edge's x_p | u | x_c | y_c | r | c_c | delta_c (2 max_m + 5 max_n; x_p in the split form only), padded to a whole
// 16-byte piece.
__host__ __device__ inline int tree_z_doubles(const int max_n, const int max_m) {
  return (10 * max_n + 2 * max_m + 1) & ~1;
}
// The split form's parts: head | tail, max_n doubles each, per node and per edge, behind the wavefronts' areas.
__host__ __device__ inline size_t tree_parts_bytes(const int num_nodes, const int num_edges, const int max_n) {
  return (size_t)(num_nodes + num_edges) * 2 * (size_t)max_n * sizeof(double);
}

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
// then, when staged, the image: `scalars` doubles behind at most one of lead-in, padded likewise
__host__ __device__ inline long tree_image_bytes(const long scalars) { return (scalars * 8 + 16 + 15) & ~15L; }

// res != nullptr or scaled == nullptr: plain form (res may be nullptr: norms only); scaled != nullptr: rho / s_p to
// `scaled`, s_p to `scale`.  rhs == nullptr: q, c, r are those of `input`; else they are read from `rhs`, one column
// in the output arena's layout.
// SPLIT: the wavefronts take nodes AND edges in turn, so the children of one node spread over them; an item parks its
// part of rho_q (Q x of a node, M u + A^T y_c of an edge) in LDS, max_n doubles per item behind the wavefronts'
// areas, and after a barrier every rho_q[i] is summed from them in the order of the other form: Q x first, then the
// child edges in CSR order -- the same additions, the same bits.  The host picks it where one node's children outnumber
// a wavefront's even share of the items and the parts fit (tree_residual.hip); elsewhere nodes in turn are faster.
template <bool STAGED, bool SPLIT>
__global__ void __launch_bounds__(kLanes * kMaxWaves)
    tree_residual_kernel(const tree::Meta mt, const double *__restrict__ input, const double *__restrict__ rhs,
                         const double *__restrict__ sol, double *__restrict__ res, double *__restrict__ scaled,
                         double *__restrict__ scale, double *__restrict__ norm, const int wave_bytes) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const long p = blockIdx.x;
  const int lane = threadIdx.x & (kLanes - 1), wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kLanes);
  const int waves = blockDim.x / kLanes;
  const int part = lane & (kParts - 1);
  double *red = (double *)lds;
  unsigned char *mine = lds + kRedBytes + (size_t)wave * wave_bytes;
  // node part: xi | yi | qi | acc (max_n each); edge part: (SPLIT: x_p |) u | x_c | y_c | r | c_c | delta_c, packed by
  // the edge's dims
  double *xi = (double *)mine, *yi = xi + mt.max_n, *qi = yi + mt.max_n, *acc_q = qi + mt.max_n; // acc: head | tail
  double *ze = acc_q + 2 * mt.max_n;
  double *parts = (double *)(lds + kRedBytes + (size_t)(blockDim.x / kLanes) * wave_bytes); // SPLIT: [item][2 max_n]
  double *img = (double *)(mine + tree_z_doubles(mt.max_n, mt.max_m) * sizeof(double));
  const double *pin = input + p * mt.in0_len, *ps = sol + p * mt.out_len;
  const double *pr = rhs != nullptr ? rhs + p * mt.out_len : nullptr;

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

  // acc + sum over k < count of blk[at(k)] * z[k], this lane's share (k = part, part + kParts, ...); at(k) =
  // base + stride k, or, SYM, element (r, k) of a symmetric dim x dim matrix at `base` of which the lower triangle
  // is read.  kDotUnroll terms are loaded before the first is used.
  auto segment = [&](auto SYM, const double *blk, Pair acc, const int base, const int stride, const int count,
                     const double *z, const bool sym_lane, const int r, const int dim) {
    for (int k = part; k < count; k += kParts * kDotUnroll) {
      double a[kDotUnroll], zz[kDotUnroll];
#pragma unroll
      for (int j = 0; j < kDotUnroll; ++j) {
        const int kk = k + j * kParts < count ? k + j * kParts : k; // past the end: the first term again, unused
        int at = base + stride * kk;
        if constexpr (decltype(SYM)::value)
          at = sym_lane ? base + (kk < r ? r + dim * kk : kk + dim * r) : at;
        a[j] = blk[at], zz[j] = z[kk];
      }
#pragma unroll
      for (int j = 0; j < kDotUnroll; ++j)
        acc = pair_fma(acc, k + j * kParts < count ? a[j] : 0.0, zz[j]); // (a term of 0 changes nothing)
    }
    return acc;
  };

  const int passes = scaled != nullptr ? 2 : 1;
  double s_p = 1.0;
  for (int pass = 0; pass < passes; ++pass) {
    const bool want_norm = pass == 0, store = pass == passes - 1;
    double nrm = 0.0;
    auto emit = [&](const long idx, const double v) {
      if (want_norm)
        nrm = nan_max(nrm, __builtin_fabs(v));
      if (store) {
        if (scaled != nullptr)
          scaled[p * mt.out_len + idx] = v / s_p;
        else if (res != nullptr)
          res[p * mt.out_len + idx] = v;
      }
    };
    const int items = SPLIT ? mt.num_nodes + mt.num_edges : mt.num_nodes;
    for (int item = wave; item < items; item += waves) {
      const bool node_item = item < mt.num_nodes; // (always, unless SPLIT)
      const int i = node_item ? item : mt.edge_parents[item - mt.num_nodes];
      const int n = mt.state_dims[i];
      const long ox = mt.ox[i], oy = mt.oy[i];
      const double *q_src = pr != nullptr ? pr + ox : pin + mt.oq[i];
      double *q_sink = SPLIT ? parts + (long)item * 2 * mt.max_n : acc_q, *q_tail = q_sink + mt.max_n;
      lds_order(); // the previous item's reads of its vectors and of the image are done
      // ---- the node: x_i | y_i | q_i, then rows [0, n) of Q x_i
      if (node_item) {
        for (int base = 0; base < 3 * n; base += kLanes * kGatherUnroll) {
          double r[kGatherUnroll];
          int k[kGatherUnroll];
#pragma unroll
          for (int j = 0; j < kGatherUnroll; ++j) {
            k[j] = base + j * kLanes + lane < 3 * n ? base + j * kLanes + lane : 3 * n - 1;
            const int o = k[j] < n ? k[j] : (k[j] < 2 * n ? k[j] - n : k[j] - 2 * n);
            const double *src = k[j] < n ? ps + ox : (k[j] < 2 * n ? ps + oy : q_src);
            r[j] = src[o];
          }
#pragma unroll
          for (int j = 0; j < kGatherUnroll; ++j) // (xi, yi, qi are max_n apart)
            (k[j] < n ? xi : (k[j] < 2 * n ? yi - n : qi - 2 * n))[k[j]] = r[j];
        }
        const double *Q = stage(pin + mt.oQ[i], n * n);
        lds_order();
        for (int w0 = 0; w0 < n * kParts; w0 += kLanes) {
          const int w = w0 + lane, row = w / kParts;
          const bool active = row < n;
          Pair acc = segment(std::true_type{}, Q, Pair{0.0, 0.0}, 0, 0, active ? n : 0, xi, true, row, n);
          acc = pair_join(acc, pair_shfl_xor(acc, 1));
          acc = pair_join(acc, pair_shfl_xor(acc, 2));
          if (active && part == 0)
            q_sink[row] = acc.h, q_tail[row] = acc.l;
        }
        if (i == mt.root) {
          const double *c_src = pr != nullptr ? pr + oy : pin + mt.oc[i], *d_src = pin + mt.od[i];
          for (int r = lane; r < n; r += kLanes)
            emit(oy + r, total(pair_add(pair_fma(Pair{-xi[r], 0.0}, -d_src[r], yi[r]), c_src[r])));
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
        const double *r_src = pr != nullptr ? pr + ou : pin + mt.orr[e];
        const double *c_src = pr != nullptr ? pr + oyc : pin + mt.oc[ch], *d_src = pin + mt.od[ch];
        const int xp = SPLIT ? n : 0; // x of the parent: gathered with the edge's vectors, else the node's x_i in LDS
        const double *xs = SPLIT ? ze : xi;
        double *u = ze + xp, *xc = u + m, *yc = xc + nc, *re = yc + nc, *cc = re + m, *dc = cc + nc;
        lds_order(); // the previous item's reads of the edge vectors and of the image are done
        const int zl = xp + 2 * m + 4 * nc;
        for (int base = 0; base < zl; base += kLanes * kGatherUnroll) {
          double r[kGatherUnroll];
          int k[kGatherUnroll];
#pragma unroll
          for (int j = 0; j < kGatherUnroll; ++j) {
            k[j] = base + j * kLanes + lane < zl ? base + j * kLanes + lane : zl - 1;
            // (x_p |) u | x_c | y_c | r | c_c | delta_c
            int o = k[j];
            const double *src = ps + ox;
            if (o >= xp) {
              o -= xp, src = ps + ou;
              if (o >= m) {
                o -= m, src = ps + oxc;
                if (o >= nc) {
                  o -= nc, src = ps + oyc;
                  if (o >= nc) {
                    o -= nc, src = r_src;
                    if (o >= m) {
                      o -= m, src = c_src;
                      if (o >= nc)
                        o -= nc, src = d_src;
                    }
                  }
                }
              }
            }
            r[j] = src[o];
          }
#pragma unroll
          for (int j = 0; j < kGatherUnroll; ++j)
            ze[k[j]] = r[j];
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
          Pair acc = segment(std::false_type{}, blk, Pair{0.0, 0.0}, b0, s0, c0, xs, false, 0, 0);
          acc = segment(std::true_type{}, blk, acc, b1, s1, c1, u, r_row, j, m);
          acc = segment(std::false_type{}, blk, acc, b2, 1, c2, yc, false, 0, 0);
          acc = pair_join(acc, pair_shfl_xor(acc, 1));
          acc = pair_join(acc, pair_shfl_xor(acc, 2));
          if (active && part == 0) {
            if (q_row) {
              if constexpr (!SPLIT)
                acc = pair_join(Pair{q_sink[row], q_tail[row]}, acc);
              q_sink[row] = acc.h, q_tail[row] = acc.l;
            } else if (r_row) {
              emit(ou + j, total(pair_add(acc, re[j])));
            } else {
              emit(oyc + r, total(pair_add(pair_fma(pair_add(acc, -xc[r]), -dc[r], yc[r]), cc[r])));
            }
          }
        }
      }
      if constexpr (!SPLIT) {
        lds_order();
        for (int r = lane; r < n; r += kLanes) // (acc_q[r]: through LDS from the first lane of row r's group)
          emit(ox + r, total(pair_add(pair_add(Pair{acc_q[r], acc_q[mt.max_n + r]}, -yi[r]), qi[r])));
      }
    }
    if constexpr (SPLIT) { // rho_q[i] from the parts: Q x, then the child edges in CSR order
      __syncthreads();
      for (int i = wave; i < mt.num_nodes; i += waves) {
        const int n = mt.state_dims[i];
        const long ox = mt.ox[i];
        const double *y_src = ps + mt.oy[i], *q_src = pr != nullptr ? pr + ox : pin + mt.oq[i];
        for (int r = lane; r < n; r += kLanes) {
          const double *own = parts + (long)i * 2 * mt.max_n + r;
          Pair v{own[0], own[mt.max_n]};
          for (int ci = mt.child_offsets[i]; ci < mt.child_offsets[i + 1]; ++ci) {
            const double *of_edge = parts + (long)(mt.num_nodes + mt.child_edges[ci]) * 2 * mt.max_n + r;
            v = pair_join(v, Pair{of_edge[0], of_edge[mt.max_n]});
          }
          emit(ox + r, total(pair_add(pair_add(v, -y_src[r]), q_src[r])));
        }
      }
    }
    if (want_norm) {
      for (int off = kLanes / 2; off > 0; off >>= 1)
        nrm = nan_max(nrm, __shfl_xor(nrm, off));
      if (lane == 0)
        red[wave] = nrm;
      __syncthreads();
      double all = red[0];
      for (int k = 1; k < waves; ++k)
        all = nan_max(all, red[k]);
      s_p = pow2_scale(all);
      if (threadIdx.x == 0) {
        norm[p] = all;
        if (scaled != nullptr)
          scale[p] = s_p;
      }
    }
  }
}

} // namespace residual
} // namespace sipamd
