// tree_mrhs_qw16.hpp -- LQR::solve() for SEVERAL right-hand sides in one sweep, on TREES (fp64).
//
// Replaces the multi-right-hand-side block of the reference's solve_stagewise_kkt_matrix
// (helpers.cpp:521-665: LQR::solve generalised from GEMV to GEMM over the columns of J_theta, reading
// LQR::Workspace directly) for any tree whose state dimensions are <= 15 and control dimensions <= 8:
// the tree counterpart of chain_mrhs.hpp.  It reads the factor state the reference keeps in
// LQR::Workspace (lqr.hpp:109-135) from the tree work arena, as sip_lqr_tree_factor() or
// sip_lqr_tree_factor_solve_workspace() leave it: W, G_factor, K per edge; V, F_factor, sqrt_delta,
// sqrt_delta_inv per node.  G_factor / F_factor hold Eigen's L in their lower triangles (the entries
// above the diagonal are stale and never read), so the G solve of k and F_inv_mult_vector
// (lqr.cpp:531-549) are two triangular solves with L, as in lqr.cpp.  The work arena is only read.
//
// Mapping as tree_qw16.hpp / chain_mrhs.hpp: one problem per 16-lane DPP row, vectors DISTRIBUTED over
// the lanes (lane r holds element r), every matrix-vector product one broadcast-FMA block (dotv:
// acc += x@lane k * B[k]) on the lane's own row / column of the operand, each node padded to the size
// class (N, M) in registers by clamped loads and selects.  The triangular solves run distributed too:
// step j broadcasts the finished element j (one v_fmac_f64_dpp per step), lane i keeps row i of L for
// the forward and column i for the backward substitution.  Every matrix operand of a step is fetched
// once and applied to all columns of the wavefront's group.  Traversal: the plan's TreeStep records
// (postorder backward, preorder rollout; a forward record carries the work-arena offsets of its CHILD).
//
// Per-column state (column scratch, per column and problem: v (N) per node | k (M) per edge, padded):
// v of a node is written by its node step and read back by the edge step of its parent and by the
// rollout, k by the rollout; x of a parent is read back from the output column.  Every element is
// read back by the lane that wrote it, so no barrier is needed between the two sweeps.
//
// Layouts (include/sip_lqr_amd.h): column `col` of problem b of the right-hand sides (node blocks
// q (n) | c (n), edge blocks r (m): the output arena's layout) and of the outputs (x | y, u) at
// (col * batch + b) * out_len.  A launch of `ncols_launch` columns is a grid of (batch / 4) x
// ceil(ncols_launch / P) single-wave workgroups: wavefront (b, y) carries columns [y P, y P + P).
//
// SINGLE (P = 1; tree_solve_qw16, sip_lqr_tree_solve_fused): LQR::solve itself (lqr.cpp:735-871), with the contract
// of sip_lqr_tree_solve: q, c and r come from the INPUT arena (rhs_all is not read), v per node and k per edge go
// to their LQR::Workspace slots of the work arena, which cols_all then points at (the other fields of that arena
// are only read, through work_all).  The backward records of edge steps carry the CHILD's v offset in `ov`.
#pragma once
#include <hip/hip_runtime.h>

#include "tree_qw16.hpp"

namespace sipamd {

template <int N, int M>
struct TreeColLayout {
  __host__ __device__ static long len(const TreeSchedule &ts) { return (long)ts.Nn * N + (long)ts.E * M; } // per column and problem
};

template <int N, int M, int P, bool SINGLE = false>
__global__ __launch_bounds__(64) void tree_solve_mrhs_qw16(
    const TreeSchedule ts, const double *__restrict__ in_all, const double *__restrict__ work_all,
    const double *__restrict__ rhs_all, double *out_all, double *cols_all, const int *__restrict__ status,
    const long batch, const int ncols_launch) {
  static_assert(N >= 1 && N <= 16 && M >= 1 && M <= 16 && P >= 1 && P <= 16, "");
  static_assert(!SINGLE || P == 1, "one right-hand side");
  const int col0 = (int)blockIdx.y * P;
  const int ncols = ncols_launch - col0 < P ? ncols_launch - col0 : P;
  const int lane = threadIdx.x & 63, c = lane & 15, rr = lane >> 4;
  long p = (long)blockIdx.x * 4 + rr;
  const bool valid = p < batch;
  if (!valid)
    p = batch - 1;
  // a problem whose factorization failed is skipped: its output columns stay untouched
  const bool live = valid && status[p] == 0;
  const long CL = TreeColLayout<N, M>::len(ts), KOFF = (long)ts.Nn * N;
  const double *in = in_all + p * ts.in_len;
  const double *wk = work_all + p * ts.ws_len;
  // column col of this group: base + col * stride
  const long io_stride = batch * ts.out_len, cl_stride = batch * CL;
  const double *rhs = SINGLE ? in : rhs_all + ((long)col0 * batch + p) * ts.out_len;
  double *out = out_all + ((long)col0 * batch + p) * ts.out_len;
  double *cl = cols_all + (SINGLE ? p * ts.ws_len : ((long)col0 * batch + p) * CL);
  // where q of a node, c of a child, r of an edge (in `rhs`), v of a node and k of an edge (in `cl`) are
  auto off_q = [](const TreeStep &st) { return SINGLE ? st.oq : st.oxp; };
  auto off_cc = [](const TreeStep &st) { return SINGLE ? st.odc - st.nc : st.oyc; }; // input arena: c | delta
  auto off_r = [](const TreeStep &st) { return SINGLE ? st.orr : st.ou; };
  auto off_vc = [](const TreeStep &st) { return SINGLE ? st.ov : (long)st.child * N; };
  auto off_vn = [](const TreeStep &st) { return SINGLE ? st.ov : (long)st.node * N; };
  auto off_k = [&](const TreeStep &st) { return SINGLE ? st.ok : KOFF + (long)st.edge * M; };

  // Element (r, k) of the column-major rows x cols block at `off` of arena `a` (0 outside it): the
  // load is issued unconditionally from a clamped address (the arena's first scalar, always readable)
  // and the padding selected afterwards -- plain locals, conditions joined with `&`, so that the front
  // end emits a select and no exec-masked branch around the load.
  auto at = [](const double *a, const long off, const int rows, const int cols, const int r, const int k) {
    const bool in_ = (r < rows) & (k < cols);
    const double ld = a[in_ ? off + r + (long)rows * k : 0];
    return in_ ? ld : 0.0;
  };
  auto sum4 = [](const double (&a)[4]) { return (a[0] + a[1]) + (a[2] + a[3]); };
  // L^{-T} L^{-1} z for z distributed over the lanes (L of an S x S factor, padded to R): lane i holds
  // row i of L strictly below the diagonal in Lr, column i strictly below it in Lc, 1 / L(i, i) in li
  // (0 on the padding, which zeroes the padded entries of the result).
  auto llt_solve = [](auto RR, const double (&Lr)[decltype(RR)::value], const double (&Lc)[decltype(RR)::value],
                      const double li, double z) {
    constexpr int R = decltype(RR)::value;
    sfor<0, R>([&](auto jj) { // forward: w_j = (z_j - sum_{i<j} L(j, i) w_i) / L(j, j)
      constexpr int j = decltype(jj)::value;
      double w[1] = {z * li};
      rank1<1, j, true, true>(&z, w, Lr[j]);
    });
    z *= li;
    sfor_down<R - 1, -1>([&](auto jj) { // backward: x_j = (w_j - sum_{i>j} L(i, j) x_i) / L(j, j)
      constexpr int j = decltype(jj)::value;
      double x[1] = {z * li};
      rank1<1, j, true, true>(&z, x, Lc[j]);
    });
    return z * li;
  };
  // the lower-triangular factor L (rows x rows) at `off`: row c / column c strictly below the diagonal and
  // 1 / L(c, c) (as lqr.cpp, only the lower triangle is read)
  auto load_L = [&](auto RR, const long off, const int rows, double (&Lr)[decltype(RR)::value],
                    double (&Lc)[decltype(RR)::value], double &li) {
    sfor<0, decltype(RR)::value>([&](auto jj) {
      constexpr int j = decltype(jj)::value;
      const double lr = at(wk, off, rows, rows, c, j), lc = at(wk, off, rows, rows, j, c);
      Lr[j] = (j < c) ? lr : 0.0;
      Lc[j] = (j > c) ? lc : 0.0;
    });
    const double d = at(wk, off, rows, rows, c, c);
    li = c < rows ? rcp_nr(d) : 0.0;
  };
  using NN = std::integral_constant<int, N>;
  using MM = std::integral_constant<int, M>;

  // ---- backward affine sweep (lqr.cpp:738-796) ------------------------------------------------------
  struct Bwd { // operands of one step: W row, B column, A column, K column, L of G; per column q, c, r, v_child
    double Wr[N], Bc[N], Ac[N], Kc[M], Lr[M], Lc[M], li, dl, qv[P], cv[P], rv[P], vc[P];
  };
  auto load_bwd = [&](const TreeStep &st, Bwd &o) {
    const int n = st.n, nc = st.nc, m = st.m;
    if (st.flags & TS_LOAD_V)
      sfor<0, P>([&](auto cc) {
        constexpr int col = decltype(cc)::value;
        if (col < ncols)
          o.qv[col] = at(rhs + col * io_stride, off_q(st), n, 1, c, 0); // q of `node` (the x slot of the layout)
      });
    if (st.kind != 0)
      return;
    sfor<0, N>([&](auto kk) {
      constexpr int k = decltype(kk)::value;
      o.Wr[k] = at(wk, st.oW, nc, nc, c, k); // row c of W (nc x nc)
      o.Bc[k] = at(in, st.oB, nc, m, k, c);  // column c of B (nc x m)
      o.Ac[k] = at(in, st.oA, nc, n, k, c);  // column c of A (nc x n)
    });
    sfor<0, M>([&](auto jj) { o.Kc[decltype(jj)::value] = at(wk, st.oK, m, n, decltype(jj)::value, c); });
    load_L(MM{}, st.oG, m, o.Lr, o.Lc, o.li);
    o.dl = at(in, st.odc, nc, 1, c, 0);
    sfor<0, P>([&](auto cc) {
      constexpr int col = decltype(cc)::value;
      if (col < ncols) {
        o.cv[col] = at(rhs + col * io_stride, off_cc(st), nc, 1, c, 0); // c of the child (the y slot)
        o.rv[col] = at(rhs + col * io_stride, off_r(st), m, 1, c, 0);   // r of the edge (the u slot)
        o.vc[col] = at(cl + col * cl_stride, off_vc(st), nc, 1, c, 0);
      }
    });
  };
  double v[P]; // v of the node being accumulated, per column
  sfor<0, P>([&](auto cc) { v[decltype(cc)::value] = 0.0; });
  for (int s = 0; s < ts.n_backward; ++s) {
    const TreeStep st = ts.backward[s];
    Bwd o;
    load_bwd(st, o);
    if (st.flags & TS_LOAD_V) // v = q  (lqr.cpp:744)
      sfor<0, P>([&](auto cc) { v[decltype(cc)::value] = o.qv[decltype(cc)::value]; });
    if (st.kind == 0) { // one child edge of `node` (lqr.cpp:776-794)
      const long ko = off_k(st);
      sfor<0, P>([&](auto cc) {
        constexpr int col = decltype(cc)::value;
        if (col < ncols) {
          const double f = o.dl * o.vc[col] - o.cv[col]; // f = delta o v_c - c  (:778-779)
          double acc[4] = {0.0, 0.0, 0.0, 0.0};
          dotv<N, true>(acc, f, o.Wr);
          const double g = o.vc[col] - sum4(acc); // g = v_c - W f  (:780-781)
          double ah[4] = {o.rv[col], 0.0, 0.0, 0.0};
          dotv<N, true>(ah, g, o.Bc);
          const double h = sum4(ah);                       // h = r + B^T g  (:783-784), lanes < m
          const double k = -llt_solve(MM{}, o.Lr, o.Lc, o.li, h); // k = -G^{-1} h  (:785-791)
          if (live & (c < st.m))
            cl[col * cl_stride + ko + c] = k;
          double av[4] = {0.0, 0.0, 0.0, 0.0};
          dotv<N, true>(av, g, o.Ac);
          dotv<M, true>(av, h, o.Kc);
          v[col] += sum4(av); // v += A^T g + K^T h  (:793-794)
        }
      });
    } else if (live & (c < st.n)) { // the node is finished: its v, for its parent's edge step and the rollout
      sfor<0, P>([&](auto cc) {
        constexpr int col = decltype(cc)::value;
        if (col < ncols)
          cl[col * cl_stride + off_vn(st) + c] = v[col];
      });
    }
  }

  // ---- root (lqr.cpp:798-819): x = -F^{-1}(delta o v - c), y = v + V x -----------------------------
  {
    const TreeStep st = ts.backward[ts.n_backward - 1]; // the root's node step (last in postorder)
    const int n = ts.root_n;
    double Vr[N], Lr[N], Lc[N], li;
    sfor<0, N>([&](auto kk) { Vr[decltype(kk)::value] = at(wk, st.oV, n, n, c, decltype(kk)::value); });
    load_L(NN{}, st.oF, n, Lr, Lc, li);
    const double dl = at(in, ts.root_od, n, 1, c, 0), sd = at(wk, st.osd, n, 1, c, 0),
                 sdi = at(wk, st.osdi, n, 1, c, 0);
    sfor<0, P>([&](auto cc) {
      constexpr int col = decltype(cc)::value;
      if (col < ncols) {
        const double cr = at(rhs + col * io_stride, SINGLE ? ts.root_od - n : ts.root_oy, n, 1, c, 0);
        const double f = dl * v[col] - cr;
        const double x = -sd * llt_solve(NN{}, Lr, Lc, li, sdi * f); // F_inv_mult_vector  (lqr.cpp:531-549)
        double ay[4] = {v[col], 0.0, 0.0, 0.0};
        dotv<N, true>(ay, x, Vr);
        if (live & (c < n)) {
          out[col * io_stride + ts.root_ox + c] = x;
          out[col * io_stride + ts.root_oy + c] = sum4(ay);
        }
      }
    });
  }

  // ---- forward rollout (lqr.cpp:821-870); lane r owns row r -----------------------------------------
  struct Fwd { // K row, A row, B row of the edge; V row, L of F, sqrt_delta(_inv), delta of the child
    double KT[N], Ar[N], Br[M], Vr[N], Lr[N], Lc[N], li, sd, sdi, dl, xp[P], kk[P], cc[P], vc[P];
  };
  auto load_fwd = [&](const TreeStep &st, Fwd &o) {
    const int n = st.n, nc = st.nc, m = st.m;
    sfor<0, N>([&](auto kk) {
      constexpr int k = decltype(kk)::value;
      o.KT[k] = at(wk, st.oK, m, n, c, k);  // row c of K (m x n)
      o.Ar[k] = at(in, st.oA, nc, n, c, k); // row c of A (nc x n)
      o.Vr[k] = at(wk, st.oV, nc, nc, c, k); // row c of V of the child
    });
    sfor<0, M>([&](auto jj) { o.Br[decltype(jj)::value] = at(in, st.oB, nc, m, c, decltype(jj)::value); });
    load_L(NN{}, st.oF, nc, o.Lr, o.Lc, o.li);
    o.sd = at(wk, st.osd, nc, 1, c, 0), o.sdi = at(wk, st.osdi, nc, 1, c, 0), o.dl = at(in, st.odc, nc, 1, c, 0);
    const long ko = off_k(st);
    sfor<0, P>([&](auto cc) {
      constexpr int col = decltype(cc)::value;
      if (col < ncols) {
        o.xp[col] = at(out + col * io_stride, st.oxp, n, 1, c, 0); // x of the parent (written by this lane)
        o.kk[col] = at(cl + col * cl_stride, ko, m, 1, c, 0);
        o.cc[col] = at(rhs + col * io_stride, off_cc(st), nc, 1, c, 0);
        o.vc[col] = at(cl + col * cl_stride, off_vc(st), nc, 1, c, 0);
      }
    });
  };
  for (int s = 0; s < ts.n_forward; ++s) {
    const TreeStep st = ts.forward[s];
    Fwd o;
    load_fwd(st, o);
    sfor<0, P>([&](auto cc) {
      constexpr int col = decltype(cc)::value;
      if (col < ncols) {
        double au[4] = {o.kk[col], 0.0, 0.0, 0.0};
        dotv<N, true>(au, o.xp[col], o.KT);
        const double u = sum4(au); // u = k + K x  (:856-857), lanes < m
        double af[4] = {o.cc[col] - o.dl * o.vc[col], 0.0, 0.0, 0.0};
        dotv<N, true>(af, o.xp[col], o.Ar);
        dotv<M, true>(af, u, o.Br);
        const double f = sum4(af); // c - delta o v + A x + B u  (:859-862)
        const double xc = o.sd * llt_solve(NN{}, o.Lr, o.Lc, o.li, o.sdi * f); // (:863-865)
        double ay[4] = {o.vc[col], 0.0, 0.0, 0.0};
        dotv<N, true>(ay, xc, o.Vr);
        if (live) {
          if (c < st.m)
            out[col * io_stride + st.ou + c] = u;
          if (c < st.nc) {
            out[col * io_stride + st.oxc + c] = xc;
            out[col * io_stride + st.oyc + c] = sum4(ay); // y = v + V x  (:867-868)
          }
        }
      }
    });
  }
}

} // namespace sipamd
