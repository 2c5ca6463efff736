// chain_qf32_sweeps.hpp -- the separate sweeps of the fused fp32 chain kernel (chain_qf32.hpp), opted into by
// sip_lqr_plan_set_separate_sweeps on a plan that took sip_lqr_plan_set_fused_f32:
//
//   chain_factor_qf32<N, M>          the backward MATRIX sweep alone (LQR::factor_with_status): the mapping and the
//                                    arithmetic of chain_factor_solve_qf32 through the same node_factor / chol_ldl_dpp /
//                                    ldl_solve_dpp, without the affine lane, without a right-hand side and without the
//                                    rollout.  Leaves S = F^{-1} per node in the spill (qf32::Layout), K in the K part of
//                                    `gains`, the LDL factor of G per edge in `gfac` (Lt column-major in M * M scalars,
//                                    then the M reciprocals of the pivots: the form chain_mrhs.hpp reads) and the statuses.
//   chain_solve_cols_qf32<N, M, P>   LQR::solve for up to P right-hand sides against that state: chain_mrhs.hpp on
//                                    `float`.  One problem per 16-lane row, vectors DISTRIBUTED over the lanes (lane r
//                                    holds element r), every matrix-vector product one dotv block on the lane's own
//                                    column / row of the operand; the operands of the next stage are requested before
//                                    the columns of the current one are processed, two alternating operand sets in both
//                                    passes.  1 / sqrt(delta) is v_rsq_f32 without a Newton step, as node_factor has it.
//
// Per-column state of the rollout (g, h of the child node, k of the edge):
//   cws != nullptr   cws[problem][node i][col][g (N) | h (N) | k of edge i (M)]   (sip_lqr_solve_multi)
//   cws == nullptr   one column: g | h to the g | h part of the node's spill slot, k to the k part of `gains`
//                    (sip_lqr_solve, which leaves K and k in `gains`)
// A problem whose status is not 0 is skipped: nothing of it is written.
//
// Batch tail as in the fused kernel: the whole wave stays active, the rows past the batch are clamped to the last problem
// and only their stores are predicated off.
#pragma once
#include <hip/hip_runtime.h>

#include "chain_qf32.hpp"

namespace sipamd {
namespace qf32 {

template <int N, int M>
__global__ __launch_bounds__(64) void chain_factor_qf32(const float *__restrict__ mats, float *__restrict__ gains,
                                                        float *__restrict__ wsp, float *__restrict__ gfac,
                                                        int *__restrict__ status, const long batch, const int T) {
  static_assert(N >= 1 && N <= 15 && M >= 1 && M <= 8, "the rows of chain_factor_solve_qf32");
  using L = Layout<N, M>;
  constexpr int STG = L::STG, WSN = L::WSN;
  constexpr int OFF_M = L::NODE + N * N + N * M, OFF_R = OFF_M + N * M; // M^T and R inside a mats stage block

  const int lane = threadIdx.x & 63;
  const int c = lane & 15;
  long p = (long)blockIdx.x * 4 + (lane >> 4);
  const bool valid = p < batch;
  if (!valid)
    p = batch - 1;
  const bool isM = c < N;
  const int cm = isM ? c : N - 1;   // clamped matrix column / row
  const int cu = c < M ? c : M - 1; // clamped control column / row

  const long mats_len = (long)(T + 1) * L::NODE + (long)T * L::EDGE;
  const float *pm = mats + p * mats_len;
  float *pg = gains + p * ((long)T * L::GAIN);
  float *pw = wsp + p * ((long)(T + 1) * WSN);
  float *pf = gfac + p * ((long)T * (M * M + M));

  float E[N], zero[N];
  sfor<0, N>([&](auto ii) {
    constexpr int r = decltype(ii)::value;
    E[r] = (c == r) ? 1.0f : 0.0f;
    zero[r] = 0.0f; // the right-hand side node_factor carries on the affine lane: none here
  });

  int stat = 0;
  float W[N], V[N];

  auto load_q = [&](const float *nm, float(&Vq)[N]) {
    sfor<0, N>([&](auto ii) { Vq[decltype(ii)::value] = nm[cm * N + decltype(ii)::value]; });
  };
  auto load_delta = [&](const float *nm) {
    const float d = nm[N * N + cm];
    return isM ? d : 1.0f;
  };
  // Common tail of every node: statuses, F / W and the spill of S.
  auto finish_node = [&](const int i, const float dl) {
    const unsigned long long bad = __ballot(isM && dl <= 0.0f);
    const bool bad_row = ((bad >> (lane & 48)) & 0xffffull) != 0;
    if (stat == 0 && bad_row)
      stat = 1; // INVALID_DELTA
    float X[N];
    const bool ffail = node_factor<N, true>(V, dl, c, E, zero, W, X); // this kernel's schedule needs the wait states
    if (stat == 0 && ffail)
      stat = 2; // F_FACTORIZATION_FAILURE
    if (valid && isM) { // column c of S
      float *wn = pw + (long)i * WSN + c * N;
      sfor<0, N>([&](auto ii) { wn[decltype(ii)::value] = X[decltype(ii)::value]; });
    }
  };

  // One backward step over edge i.  nm: stage block i of mats.  Operands are fetched one segment ahead of their use, as
  // in the fused kernel.
  auto backward_edge = [&](const int i, const float *nm, float &dl) {
    const float *ea = nm + L::NODE; // the stage's A | B
    float F[N], Acol[N], Bcol[N];
    float Hc[M], G[M], rinvG[M], H[M], K[M];
    sfor<0, M>([&](auto jj) {
      constexpr int j = decltype(jj)::value;
      G[j] = nm[OFF_R + cu * M + j];     // column c of R
      H[j] = nm[OFF_M + cm + j * N];     // column c of M^T = row c of M
    });
    sfor<0, N>([&](auto kk) {
      constexpr int k = decltype(kk)::value;
      Acol[k] = ea[cm * N + k];
      F[k] = 0.0f;
      Bcol[k] = ea[N * N + cu * N + k];
    });
    rank1x<N, N, true>(F, W, Acol); // F = W A
    asm volatile("" ::: "memory");
    float Vn[N];
    load_q(nm, Vn); // Q: in flight behind the G / K work

    // H_child = B^T W; G = R + H_child B
    sfor<0, M>([&](auto jj) { Hc[decltype(jj)::value] = 0.0f; });
    spreadx<M, N, false>(Hc, Bcol, W);
    rank1x<M, N, true>(G, Hc, Bcol);
    const bool gfail = chol_ldl_dpp<M>(G, rinvG, c);
    if (stat == 0 && gfail)
      stat = 3; // G_FACTORIZATION_FAILURE
    if (valid) { // the G factor for the solve sweeps: lane j < M column j of Lt, then 1 / d
      float *gf = pf + (long)i * (M * M + M);
      if (c < M)
        sfor<0, M>([&](auto jj) { gf[c * M + decltype(jj)::value] = G[decltype(jj)::value]; });
      if (c == 0)
        sfor<0, M>([&](auto jj) { gf[M * M + decltype(jj)::value] = rinvG[decltype(jj)::value]; });
    }

    // H = M^T + B^T F;  K = -G^{-1} H
    spreadx<M, N, false>(H, Bcol, F);
    sfor<0, M>([&](auto jj) { K[decltype(jj)::value] = H[decltype(jj)::value]; });
    ldl_solve_dpp<M>(G, rinvG, K);
    sfor<0, M>([&](auto jj) { K[decltype(jj)::value] = -K[decltype(jj)::value]; });
    if (valid && isM) { // column c of K; the k part is the solve sweep's
      float *gi = pg + (long)i * L::GAIN + c * M;
      sfor<0, M>([&](auto jj) { gi[decltype(jj)::value] = K[decltype(jj)::value]; });
    }

    // V = Q + A^T F + K^T H
    spreadx<N, N, false>(Vn, Acol, F);
    asm volatile("" ::: "memory");
    dl = load_delta(nm); // delta of the node: in flight behind the K^T H product
    asm volatile("" ::: "memory");
    spreadx<N, M, true>(Vn, K, H);
    sfor<0, N>([&](auto ii) { V[decltype(ii)::value] = Vn[decltype(ii)::value]; });
    asm volatile("" ::: "memory");
  };

  load_q(pm + (long)T * STG, V);
  finish_node(T, load_delta(pm + (long)T * STG));
  for (int i = T - 1; i >= 0; --i) {
    float dl;
    backward_edge(i, pm + (long)i * STG, dl);
    finish_node(i, dl);
  }
  if (valid && c == 0)
    status[p] = stat;
}

// blockIdx.x: four problems; the launch carries columns [0, ncols_launch), ncols_launch <= P, `col_stride` scalars apart in
// vecs_cols / sol_cols.
template <int N, int M, int P = 8>
__global__ __launch_bounds__(64) void chain_solve_cols_qf32(const float *__restrict__ mats,
                                                            const float *__restrict__ vecs_cols, float *sol_cols,
                                                            float *gains, float *wsp, const float *__restrict__ gfac,
                                                            float *cws, const int *__restrict__ status,
                                                            const long batch, const int T, const int ncols,
                                                            const long col_stride) {
  static_assert(N >= 1 && N <= 15 && M >= 1 && M <= 8 && P >= 1 && P <= 16, "");
  using L = Layout<N, M>;
  constexpr int STG = L::STG, VSTG = L::VSTG, WSN = L::WSN, WG = L::WG;
  constexpr int CW = 2 * N + M; // g | h | k per (node, column)

  const int lane = threadIdx.x & 63, c = lane & 15;
  long p = (long)blockIdx.x * 4 + (lane >> 4);
  const bool valid = p < batch;
  if (!valid)
    p = batch - 1;
  const bool isM = c < N;
  const int cm = isM ? c : N - 1, cu = c < M ? c : M - 1;
  const bool live = valid && status[p] == 0; // a failed factorisation: the problem is skipped
  const bool columns = cws != nullptr;

  const long mats_len = (long)(T + 1) * L::NODE + (long)T * L::EDGE;
  const long vecs_len = (long)(T + 1) * L::VNODE + (long)T * L::VEDGE;
  const float *pm = mats + p * mats_len;
  const float *pv = vecs_cols + p * vecs_len;
  float *ps = sol_cols + p * vecs_len;
  float *pg = gains + p * ((long)T * L::GAIN);
  float *pw = wsp + p * ((long)(T + 1) * WSN);
  const float *pf = gfac + p * ((long)T * (M * M + M));
  float *pc = columns ? cws + p * ((long)(T + 1) * ncols * CW) : nullptr;
  // g | h of (node i, column col): h follows g at + N in both forms
  auto gh_slot = [&](const int i, const int col) -> float * {
    return columns ? pc + ((long)i * ncols + col) * CW : pw + (long)i * WSN + WG;
  };
  auto k_slot = [&](const int i, const int col) -> float * {
    return columns ? pc + ((long)i * ncols + col) * CW + 2 * N : pg + (long)i * L::GAIN + N * M;
  };
  auto sum4 = [](const float(&a)[4]) { return (a[0] + a[1]) + (a[2] + a[3]); };

  // ---- backward affine sweep ----------------------------------------------------------------------------------------
  struct NodeOps { // node i: S row, delta, and per column c_i, q_i
    float Srow[N], dl, cvec[P], qvec[P];
  };
  struct EdgeOps { // edge i: columns of B, A; K column; the LDL factor of G; per column r_i
    float Bcol[N], Acol[N], Kc[M], Lf[M][M], rinv[M], rvec[P];
  };
  auto load_node = [&](const int i, NodeOps &o) {
    const float *slot = pw + (long)i * WSN;
    sfor<0, N>([&](auto kk) { o.Srow[decltype(kk)::value] = slot[cm * N + decltype(kk)::value]; });
    o.dl = pm[(long)i * STG + N * N + cm];
    sfor<0, P>([&](auto cc) {
      constexpr int col = decltype(cc)::value;
      if (col < ncols) {
        o.qvec[col] = pv[col * col_stride + (long)i * VSTG + cm];
        o.cvec[col] = pv[col * col_stride + (long)i * VSTG + N + cm];
      }
    });
  };
  auto load_edge = [&](const int i, EdgeOps &o) {
    const float *em = pm + (long)i * STG + L::NODE;
    const float *gi = pg + (long)i * L::GAIN;
    const float *gf = pf + (long)i * (M * M + M);
    sfor<0, N>([&](auto kk) {
      constexpr int k = decltype(kk)::value;
      o.Bcol[k] = em[N * N + cu * N + k];
      o.Acol[k] = em[cm * N + k];
    });
    sfor<0, M>([&](auto jj) {
      constexpr int j = decltype(jj)::value;
      o.Kc[j] = gi[cm * M + j];
      o.rinv[j] = gf[M * M + j];
      sfor<0, j>([&](auto iv) { o.Lf[j][decltype(iv)::value] = gf[decltype(iv)::value * M + j]; });
    });
    sfor<0, P>([&](auto cc) {
      constexpr int col = decltype(cc)::value;
      if (col < ncols)
        o.rvec[col] = pv[col * col_stride + (long)i * VSTG + L::VNODE + cu];
    });
  };
  // t = c - delta o v; h = S D^{-1/2} t (kept for the rollout); returns W t = D^{-1/2} (D^{-1/2} t - S D^{-1/2} t)
  auto node_step = [&](const int i, const int col, const NodeOps &o, const float v_) {
    const float t_ = o.cvec[col] - o.dl * v_;
    const float sdi = __builtin_amdgcn_rsqf(o.dl);
    const float phi = sdi * t_;
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    dotv<N, true>(acc, phi, o.Srow);
    const float sphi = sum4(acc);
    if (live && isM)
      gh_slot(i, col)[N + c] = sphi;
    return sdi * (phi - sphi);
  };

  float v_[P], wt[P];
  {
    NodeOps term;
    load_node(T, term);
    sfor<0, P>([&](auto cc) {
      constexpr int col = decltype(cc)::value;
      if (col < ncols) {
        v_[col] = term.qvec[col]; // v_T = q_T
        wt[col] = node_step(T, col, term, v_[col]);
      }
    });
  }
  // One backward step over edge i with the operands in (ed, nd); the next stage's operands are requested into
  // (ed_next, nd_next) first, so that they travel while the columns are processed.
  auto backward_stage = [&](const int i, const EdgeOps &ed, const NodeOps &nd, EdgeOps &ed_next, NodeOps &nd_next) {
    if (i > 0) {
      load_edge(i - 1, ed_next);
      load_node(i - 1, nd_next);
    }
    sfor<0, P>([&](auto cc) {
      constexpr int col = decltype(cc)::value;
      if (col < ncols) {
        const float gd = v_[col] + wt[col]; // g = v_c + W t
        if (live && isM)
          gh_slot(i + 1, col)[c] = gd;
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        dotv<N, true>(acc, gd, ed.Bcol);
        const float hd = ed.rvec[col] + sum4(acc); // r + B^T g, lane j < M holds element j
        float hf[M], kf[M];
        sfor<0, M>([&](auto jj) { hf[decltype(jj)::value] = bcast<decltype(jj)::value>(hd); });
        sfor<0, M>([&](auto jj) { // G^{-1} (r + B^T g), replicated over the lanes
          constexpr int j = decltype(jj)::value;
          float w = hf[j];
          sfor<0, j>([&](auto iv) { w = __builtin_fmaf(-ed.Lf[j][decltype(iv)::value], kf[decltype(iv)::value], w); });
          kf[j] = w * ed.rinv[j];
        });
        sfor_down<M - 1, -1>([&](auto jj) {
          constexpr int j = decltype(jj)::value;
          float a = 0.0f;
          sfor<j + 1, M>([&](auto iv) { a = __builtin_fmaf(ed.Lf[decltype(iv)::value][j], kf[decltype(iv)::value], a); });
          kf[j] = __builtin_fmaf(-ed.rinv[j], a, kf[j]);
        });
        if (live && c == 0) {
          float *kd = k_slot(i, col);
          sfor<0, M>([&](auto jj) { kd[decltype(jj)::value] = -kf[decltype(jj)::value]; });
        }
        float acc2[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        dotv<N, true>(acc2, gd, ed.Acol);
        float kh = 0.0f; // K^T (r + B^T g) with K = -G^{-1} H (the stored gain)
        sfor<0, M>([&](auto jj) { kh = __builtin_fmaf(ed.Kc[decltype(jj)::value], hf[decltype(jj)::value], kh); });
        v_[col] = nd.qvec[col] + sum4(acc2) + kh; // v = q + A^T g + K^T h
        wt[col] = node_step(i, col, nd, v_[col]);
      }
    });
  };
  {
    NodeOps nd_a, nd_b;
    EdgeOps ed_a, ed_b;
    if (T > 0) {
      load_edge(T - 1, ed_a);
      load_node(T - 1, nd_a);
    }
    for (int i = T - 1; i >= 0; i -= 2) {
      backward_stage(i, ed_a, nd_a, ed_b, nd_b);
      if (i >= 1)
        backward_stage(i - 1, ed_b, nd_b, ed_a, nd_a);
    }
  }
  sfor<0, P>([&](auto cc) { // root: g_0 = v_0 + W_0 (c_0 - delta_0 o v_0)
    constexpr int col = decltype(cc)::value;
    if (col < ncols && live && isM)
      gh_slot(0, col)[c] = v_[col] + wt[col];
  });
  // the rollout reads g / h / k written above by other lanes of this wave (the block is one wavefront)
  __syncthreads();

  // ---- forward rollout; lane r < N owns row r -----------------------------------------------------------------------
  struct FwdOps {
    float KT[N], Arow[N], Brow[M], Sr[N], dd, kk0[P], gg[P], hh[P];
  };
  auto load_fwd = [&](const int i, FwdOps &o) {
    const float *em = pm + (long)i * STG + L::NODE;
    const float *gi = pg + (long)i * L::GAIN;
    const float *wn = pw + (long)(i + 1) * WSN;
    sfor<0, N>([&](auto kk) {
      constexpr int k = decltype(kk)::value;
      o.KT[k] = gi[k * M + cu];
      o.Arow[k] = em[k * N + cm];
      o.Sr[k] = wn[cm * N + k]; // S symmetric: row r = column r
    });
    sfor<0, M>([&](auto jj) { o.Brow[decltype(jj)::value] = em[N * N + decltype(jj)::value * N + cm]; });
    o.dd = pm[(long)(i + 1) * STG + N * N + cm];
    sfor<0, P>([&](auto cc) {
      constexpr int col = decltype(cc)::value;
      if (col < ncols) {
        o.kk0[col] = k_slot(i, col)[cu];
        const float *gh = gh_slot(i + 1, col);
        o.gg[col] = gh[cm];
        o.hh[col] = gh[N + cm];
      }
    });
  };
  float x[P];
  {
    const float dd = pm[N * N + cm];
    const float sd0 = dd * __builtin_amdgcn_rsqf(dd);
    sfor<0, P>([&](auto cc) { // root: x_0 = D^{1/2} h_0, y_0 = g_0
      constexpr int col = decltype(cc)::value;
      if (col < ncols) {
        const float *gh = gh_slot(0, col);
        const float gg = gh[cm], hh = gh[N + cm];
        x[col] = sd0 * hh;
        if (live && isM) {
          ps[col * col_stride + c] = x[col];
          ps[col * col_stride + N + c] = gg;
        }
      }
    });
  }
  auto forward_stage = [&](const int i, const FwdOps &fw, FwdOps &fw_next) {
    if (i + 1 < T)
      load_fwd(i + 1, fw_next);
    const float sdi = __builtin_amdgcn_rsqf(fw.dd), sdv = fw.dd * sdi; // as node_factor computed them
    sfor<0, P>([&](auto cc) {
      constexpr int col = decltype(cc)::value;
      if (col < ncols) {
        float acc[4] = {fw.kk0[col], 0.0f, 0.0f, 0.0f};
        dotv<N, true>(acc, x[col], fw.KT);
        const float u = sum4(acc); // u = k + K x; lanes < M
        float az[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        dotv<N, true>(az, x[col], fw.Arow);
        dotv<M, true>(az, u, fw.Brow);
        const float zeta = sum4(az) * sdi; // D^{-1/2} (A x + B u)
        float as[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        dotv<N, true>(as, zeta, fw.Sr);
        const float sz = sum4(as);
        x[col] = sdv * (sz + fw.hh[col]);                           // x_c = D^{1/2} (S zeta + h)
        const float y = __builtin_fmaf(sdi, zeta - sz, fw.gg[col]); // y_c = g_c + D^{-1/2} (zeta - S zeta)
        if (live) {
          float *si = ps + col * col_stride + (long)i * VSTG;
          if (c < M)
            si[2 * N + c] = u;
          if (isM) {
            si[VSTG + c] = x[col];
            si[VSTG + N + c] = y;
          }
        }
      }
    });
  };
  FwdOps fw_a, fw_b;
  if (T > 0)
    load_fwd(0, fw_a);
  for (int i = 0; i < T; i += 2) {
    forward_stage(i, fw_a, fw_b);
    if (i + 1 < T)
      forward_stage(i + 1, fw_b, fw_a);
  }
}

} // namespace qf32
} // namespace sipamd
