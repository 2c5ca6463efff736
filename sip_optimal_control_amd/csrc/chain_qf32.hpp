// chain_qf32.hpp -- fp32 batched chain Riccati kernel, "quarter-wave" layout: the arithmetic of the direct, full-layout,
// mode-0 path of chain_qw16.hpp on `float`, for 1 <= N <= 15 and 1 <= M <= 8.
//
// One problem per 16-lane DPP row (4 problems per wavefront, one wavefront per workgroup).  Lane c < N of a row owns
// COLUMN c of every n x n / m x n matrix of its problem (rows live in registers); lane N carries the affine
// ("vector") column, so the backward affine sweep (g, h, k, v) rides along in the instructions of the matrix
// recursion: [F|g] = W [A|t], [H|h] = [M^T|r] + B^T [F|g], [K|k] = -G^{-1} [H|h], [V|v] = [Q|q] + A^T [F|g] + K^T [H|h].
//
// Cross-lane traffic is `v_fmac_f32_dpp ... row_newbcast:k` (dpp_blocks_f32_gen.hpp): hipcc does not fold a
// `v_mov_b32_dpp` into the consuming FMA, and the fp32 DPP FMA issues at the rate of the fp64 one (5 cycles per wave
// instruction), so an unfused broadcast + FMA would issue twice what the fp64 kernel issues.
//
// Factorisations are square-root-free LDL on the full symmetric storage; "a pivot <= 0" is the failure condition of
// the Cholesky factorisation they stand for.  Statuses: G before delta before F at a node, the first failing node in
// postorder.  The rollout runs on S = F^{-1} with zeta = D^{-1/2} z:
//   x_c = D^{1/2} (S zeta + h),   y_c = g_c + D^{-1/2} (zeta - S zeta),   h = S D^{-1/2} (c_c - delta_c o v_c),
// so the state spilled per node is [S | g | h] (qf32::Layout); the cheaper x_c = z + c - delta o y_c cancels for large
// delta.
//
// Memory: every lane loads its columns straight from global memory (no LDS at all).  The reciprocals of the pivots and
// 1 / sqrt(delta) are the hardware's v_rcp_f32 / v_rsq_f32 (1 ulp) without a Newton step: their error is that of one
// more rounding in a recursion of fp32 roundings.  Only compiler-scheduled instructions consume them, so the TRANS
// forwarding hazard is the compiler's to pad.
//
// The matrix sweep alone, a vector-only solve and several right-hand sides per sweep: chain_qf32_sweeps.hpp.
// Not here: LDS-DMA staging, the split (A | B in place) form, the symmetric-packed layout, n = 16.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

#include "dpp_blocks_f32_gen.hpp"
#include "qf32_launch.hpp"

namespace sipamd {
namespace qf32 {

template <int I, int E, class F>
__device__ __forceinline__ void sfor(F &&f) {
  if constexpr (I < E) {
    f(std::integral_constant<int, I>{});
    sfor<I + 1, E>(f);
  }
}
// I, I-1, ..., E+1
template <int I, int E, class F>
__device__ __forceinline__ void sfor_down(F &&f) {
  if constexpr (I > E) {
    f(std::integral_constant<int, I>{});
    sfor_down<I - 1, E>(f);
  }
}

// Value of x in lane K of the caller's 16-lane row.  x may have been written by the asm block right before (the last
// column of a rank-1 update is the next pivot column), which the compiler's hazard padding does not see: the wait
// states are part of the statement.
template <int K>
__device__ __forceinline__ float bcast(float x) {
  float r;
  asm volatile("s_nop 1\n\tv_mov_b32_dpp %0, %1 row_newbcast:%2 row_mask:0xf bank_mask:0xf" : "=v"(r) : "v"(x), "n"(K));
  return r;
}

// In-place square-root-free Cholesky (A = Lt D^-1 Lt^T) of the S x S symmetric matrix held one column per lane
// (lanes c < S).  On exit lane j holds Lt(i,j) = L(i,j) * L(j,j) in A[i], i >= j (so A[j] of lane j is the pivot
// d_j = L(j,j)^2 of the Cholesky factor) and dinv[k] = 1 / d_k replicated in every lane.  Returns true on failure
// (some pivot <= 0; a NaN pivot passes, as it passes an `x <= 0` test).
// WAIT0: the first rank-1 update carries its own wait states.  It reads columns of A that the caller's
// compiler-scheduled instructions wrote; the compiler may place such a write right before the asm block, whose DPP reads
// it does not see.  (The later updates follow the s_nop of bcast.)  The fused kernel's schedule keeps the distance
// (its listing is checked) and stays as it was compiled: false.
template <int S, bool WAIT0 = false>
__device__ __forceinline__ bool chol_ldl_dpp(float (&A)[S], float (&dinv)[S], const int c) {
  float dmin = __builtin_inff(); // the smallest pivot so far, row-replicated like the pivots
  sfor<0, S>([&](auto kk) {
    constexpr int k = decltype(kk)::value;
    const float d = bcast<k>(A[k]);
    dmin = __builtin_fminf(dmin, d);
    // lane j > k: Lt(j,k) (by symmetry its own A[k]), zero on the finished columns
    const float own = A[k] * ((c > k && c < S) ? 1.0f : 0.0f);
    const float y2 = __builtin_amdgcn_rcpf(d);
    dinv[k] = y2;
    const float upd = own * y2; // Lt(j,k) / d_k
    // A(i,j) -= Lt(i,k) Lt(j,k) / d_k, i > k, lanes j > k
    rank1<S - k - 1, k, true, (WAIT0 && k == 0)>(A + k + 1, A + k + 1, upd);
  });
  return dmin <= 0.0f;
}

// X <- (Lt D^-1 Lt^T)^{-1} X for X held one column per lane (any lane of the row may carry a right-hand side).
//   forward :  w_j = (x_j - sum_{i<j} Lt(j,i) w_i) / d_j
//   backward:  x_j = w_j - (sum_{i>j} Lt(i,j) x_i) / d_j
template <int S>
__device__ __forceinline__ void ldl_solve_dpp(const float (&Lt)[S], const float (&dinv)[S], float (&X)[S]) {
  sfor<0, S>([&](auto jj) {
    constexpr int j = decltype(jj)::value;
    X[j] *= dinv[j];
    rank1<S - j - 1, j, true, (j == 0)>(X + j + 1, Lt + j + 1, X[j]);
  });
  float acc[S];
  sfor<0, S>([&](auto jj) { acc[decltype(jj)::value] = 0.0f; });
  sfor_down<S - 1, -1>([&](auto jj) {
    constexpr int j = decltype(jj)::value;
    X[j] = __builtin_fmaf(-dinv[j], acc[j], X[j]);
    spread<j, false, false>(acc, Lt[j], X[j]); // acc[i] += Lt(j,i) x_j, i < j
  });
}

// F_factor / W of one node.  V: column c of V (lanes < N).  dl: delta_c one per lane (1 on lanes >= N).  tv:
// c - delta o v on the vector lane, zeros elsewhere.  X returns S = F^{-1} (lanes < N) and, on the vector lane,
// S D^{-1/2} tv; W = D^{-1/2} (I - S) D^{-1/2}.  Returns pivot failure.  WAIT0: see chol_ldl_dpp.
template <int N, bool WAIT0 = false>
__device__ __forceinline__ bool node_factor(const float (&V)[N], const float dl, const int c, const float (&E)[N],
                                            const float (&tv)[N], float (&W)[N], float (&X)[N]) {
  const float sdi = __builtin_amdgcn_rsqf(dl); // 1 / sqrt(delta)
  const float sd = dl * sdi;                   // sqrt(delta)
  float S[N], A[N], rinv[N];
  sfor<0, N>([&](auto ii) { S[decltype(ii)::value] = 0.0f; });
  spread<N, false, true>(S, sd, sd); // S[r] = sd_r sd_c
  sfor<0, N>([&](auto ii) {
    constexpr int r = decltype(ii)::value;
    A[r] = __builtin_fmaf(S[r], V[r], E[r]); // I + D^1/2 V D^1/2
  });
  const bool fail = chol_ldl_dpp<N, WAIT0>(A, rinv, c);
  sfor<0, N>([&](auto ii) { X[decltype(ii)::value] = E[decltype(ii)::value]; });
  spreadv<N, false>(X, sdi, tv); // vector lane: D^{-1/2} (c - delta o v)
  ldl_solve_dpp<N>(A, rinv, X);  // F^{-1} [I | .]
  sfor<0, N>([&](auto ii) { S[decltype(ii)::value] = 0.0f; });
  spread<N, false, true>(S, sdi, sdi);
  sfor<0, N>([&](auto ii) {
    constexpr int r = decltype(ii)::value;
    W[r] = (E[r] - X[r]) * S[r];
  });
  return fail;
}

// Fused factor + solve of `batch` problems, four per wavefront; grid = ceil(batch / 4) blocks of 64 threads.
// The whole wave stays active to the end (DPP reads from disabled lanes are undefined): the rows past the batch are
// clamped to the last problem and only their stores are predicated off.
template <int N, int M>
__global__ __launch_bounds__(64) void chain_factor_solve_qf32(const float *__restrict__ mats,
                                                              const float *__restrict__ vecs, float *__restrict__ sol,
                                                              float *__restrict__ gains, float *__restrict__ wsp,
                                                              int *__restrict__ status, const long batch, const int T) {
  static_assert(N >= 1 && N <= 15, "one problem per 16-lane row, lane N carries the affine column");
  static_assert(M >= 1 && M <= 8, "");
  using L = Layout<N, M>;
  constexpr int STG = L::STG, VSTG = L::VSTG, WSN = L::WSN, WG = L::WG;
  constexpr int OFF_M = L::NODE + N * N + N * M, OFF_R = OFF_M + N * M; // M^T and R inside a mats stage block

  const int lane = threadIdx.x & 63;
  const int c = lane & 15;
  long p = (long)blockIdx.x * 4 + (lane >> 4);
  const bool valid = p < batch;
  if (!valid)
    p = batch - 1;
  const bool isM = c < N;
  const bool isV = c == N;
  const int cm = isM ? c : N - 1;   // clamped matrix column / row
  const int cu = c < M ? c : M - 1; // clamped control column / row

  const long mats_len = (long)(T + 1) * L::NODE + (long)T * L::EDGE;
  const long vecs_len = (long)(T + 1) * L::VNODE + (long)T * L::VEDGE;
  const float *pm = mats + p * mats_len;
  const float *pv = vecs + p * vecs_len;
  float *ps = sol + p * vecs_len;
  float *pg = gains + p * ((long)T * L::GAIN);
  float *pw = wsp + p * ((long)(T + 1) * WSN);

  float E[N];
  sfor<0, N>([&](auto ii) {
    constexpr int r = decltype(ii)::value;
    E[r] = (c == r) ? 1.0f : 0.0f;
  });

  int stat = 0;
  float W[N], V[N], t[N], vch[N];

  // [Q_i | q_i] as the augmented column.  nm / nv: stage block of mats / vecs.
  auto load_vq = [&](const float *nm, const float *nv, float(&Vq)[N]) {
    const float *src = isV ? nv : nm + cm * N;
    sfor<0, N>([&](auto ii) {
      constexpr int r = decltype(ii)::value;
      Vq[r] = src[r];
    });
  };

  // Operands of finish_node, fetched ahead of it: delta_c one per lane, and (on the vector lane) c and delta as
  // columns.
  struct NodeTail {
    float dl, cv[N], dv[N];
  };
  auto load_tail = [&](const float *nm, const float *nv, NodeTail &nt) {
    const float d = nm[N * N + cm];
    nt.dl = isM ? d : 1.0f;
    sfor<0, N>([&](auto ii) {
      constexpr int r = decltype(ii)::value;
      nt.cv[r] = isV ? nv[N + r] : 0.0f;
      nt.dv[r] = isV ? nm[N * N + r] : 0.0f;
    });
  };
  // Common tail of every node: statuses, F / W, the vector-lane terms of the parent step (t = c - delta o v, and v)
  // and the spill of S and h.
  auto finish_node = [&](const int i, const NodeTail &nt) {
    const float dl = nt.dl;
    const unsigned long long bad = __ballot(isM && dl <= 0.0f);
    const bool bad_row = ((bad >> (lane & 48)) & 0xffffull) != 0;
    if (stat == 0 && bad_row)
      stat = 1; // INVALID_DELTA
    // c - delta o v on the vector lane, exact zeros elsewhere (cv = dv = 0)
    float tv[N], X[N];
    sfor<0, N>([&](auto ii) {
      constexpr int r = decltype(ii)::value;
      tv[r] = nt.cv[r] - nt.dv[r] * V[r];
      t[r] = tv[r];
      vch[r] = V[r];
    });
    const bool ffail = node_factor<N>(V, dl, c, E, tv, W, X);
    if (stat == 0 && ffail)
      stat = 2; // F_FACTORIZATION_FAILURE
    if (valid && c <= N) { // lanes < N: column c of S; the vector lane: h = S D^{-1/2} (c - delta o v)
      float *wn = pw + (long)i * WSN + (isV ? WG + N : c * N);
      sfor<0, N>([&](auto ii) { wn[decltype(ii)::value] = X[decltype(ii)::value]; });
    }
  };

  // One backward step over edge i.  nm / nv: stage block i of mats / vecs.  Operands are fetched one segment ahead of
  // their use (the memory fences keep the compiler from hoisting every load of a stage to the top).
  auto backward_edge = [&](const int i, const float *nm, const float *nv, NodeTail &nt) {
    const float *ea = nm + L::NODE; // the stage's A | B
    // [F | g - v_c] = W [A | t]
    float F[N], Aaug[N], Bcol[N];
    float Hc[M], G[M], rinvG[M], H[M], K[M];
    {
      const float *msrc = isV ? nv + L::VNODE : nm + (OFF_M + cm);
      sfor<0, M>([&](auto jj) {
        constexpr int j = decltype(jj)::value;
        G[j] = nm[OFF_R + cu * M + j];       // column c of R
        H[j] = isV ? msrc[j] : msrc[j * N]; // column c of M^T = row c of M; vector lane: r
      });
    }
    sfor<0, N>([&](auto kk) {
      constexpr int k = decltype(kk)::value;
      Aaug[k] = isV ? t[k] : ea[cm * N + k];
      F[k] = isV ? vch[k] : 0.0f; // the vector lane accumulates g = v_c + W t
      Bcol[k] = ea[N * N + cu * N + k];
    });
    rank1x<N, N, true>(F, W, Aaug);
    if (valid && isV) {
      float *gn = pw + (long)(i + 1) * WSN + WG;
      sfor<0, N>([&](auto ii) { gn[decltype(ii)::value] = F[decltype(ii)::value]; });
    }
    asm volatile("" ::: "memory");
    float Vn[N];
    load_vq(nm, nv, Vn); // [Q | q]: in flight behind the G / K work

    // H_child = B^T W; G = R + H_child B
    sfor<0, M>([&](auto jj) { Hc[decltype(jj)::value] = 0.0f; });
    spreadx<M, N, false>(Hc, Bcol, W);
    rank1x<M, N, true>(G, Hc, Bcol);
    const bool gfail = chol_ldl_dpp<M>(G, rinvG, c);
    if (stat == 0 && gfail)
      stat = 3; // G_FACTORIZATION_FAILURE

    // [H | h] = [M^T | r] + B^T [F | g]
    spreadx<M, N, false>(H, Bcol, F);
    // [K | k] = -G^{-1} [H | h]
    sfor<0, M>([&](auto jj) { K[decltype(jj)::value] = H[decltype(jj)::value]; });
    ldl_solve_dpp<M>(G, rinvG, K);
    sfor<0, M>([&](auto jj) { K[decltype(jj)::value] = -K[decltype(jj)::value]; });
    if (valid && c <= N) { // lanes < N: column c of K; the vector lane: k (at N * M)
      float *gi = pg + (long)i * L::GAIN + c * M;
      sfor<0, M>([&](auto jj) { gi[decltype(jj)::value] = K[decltype(jj)::value]; });
    }

    // [V | v] = [Q | q] + A^T [F | g] + K^T [H | h]   (Aaug's vector lane is never broadcast: spread reads lanes < N)
    spreadx<N, N, false>(Vn, Aaug, F);
    asm volatile("" ::: "memory");
    load_tail(nm, nv, nt); // c, delta of the node: in flight behind the K^T H product
    asm volatile("" ::: "memory");
    spreadx<N, M, true>(Vn, K, H);
    sfor<0, N>([&](auto ii) { V[decltype(ii)::value] = Vn[decltype(ii)::value]; });
    asm volatile("" ::: "memory");
  };

  // ---- terminal node ----------------------------------------------------------------------------------------------
  {
    NodeTail nt;
    load_vq(pm + (long)T * STG, pv + (long)T * VSTG, V);
    load_tail(pm + (long)T * STG, pv + (long)T * VSTG, nt);
    finish_node(T, nt);
  }
  // ---- backward recursion over edges i = T-1 .. 0 -----------------------------------------------------------------
  for (int i = T - 1; i >= 0; --i) {
    NodeTail nt;
    backward_edge(i, pm + (long)i * STG, pv + (long)i * VSTG, nt);
    finish_node(i, nt);
  }
  // ---- root: g_0 = v_0 + W_0 (c_0 - delta_0 o v_0) ----------------------------------------------------------------
  {
    float F[N];
    sfor<0, N>([&](auto ii) { F[decltype(ii)::value] = vch[decltype(ii)::value]; });
    rank1x<N, N, true>(F, W, t); // only the vector lane's column is kept
    if (valid && isV) {
      float *gn = pw + WG;
      sfor<0, N>([&](auto ii) { gn[decltype(ii)::value] = F[decltype(ii)::value]; });
    }
  }
  if (valid && c == 0)
    status[p] = stat;
  // The rollout reads S / g / h / K / k written above by other lanes of this wave: workgroup-scope release / acquire
  // (the block is one wavefront).
  __syncthreads();

  // ---- forward rollout; lane r < N owns row r ---------------------------------------------------------------------
  // root: x_0 = D^{1/2} h_0, y_0 = g_0
  float x, y;
  {
    const float gg = pw[WG + cm];
    const float hh = pw[WG + N + cm];
    const float dd = pm[N * N + cm];
    y = gg;
    x = (dd * __builtin_amdgcn_rsqf(dd)) * hh;
    if (valid && isM) {
      ps[c] = x;
      ps[N + c] = y;
    }
  }
  for (int i = 0; i < T; ++i) {
    const float *em = pm + (long)i * STG + L::NODE;
    const float *gi = pg + (long)i * L::GAIN;
    const float *wn = pw + (long)(i + 1) * WSN;
    float KT[N], Arow[N], Brow[M], Sr[N];
    sfor<0, N>([&](auto kk) {
      constexpr int k = decltype(kk)::value;
      KT[k] = gi[k * M + cu];
      Arow[k] = em[k * N + cm];
      Sr[k] = wn[cm * N + k]; // S symmetric: row r = column r
    });
    sfor<0, M>([&](auto jj) {
      constexpr int j = decltype(jj)::value;
      Brow[j] = em[N * N + j * N + cm];
    });
    const float kk0 = gi[N * M + cu];
    const float gg = wn[WG + cm];
    const float hh = wn[WG + N + cm];
    const float dd = pm[(long)(i + 1) * STG + N * N + cm];

    const float sdi = __builtin_amdgcn_rsqf(dd), sdv = dd * sdi; // as node_factor computed them
    float acc[4];
    // u = k + K x; lanes < M
    acc[0] = kk0, acc[1] = 0.0f, acc[2] = 0.0f, acc[3] = 0.0f;
    dotv<N, true>(acc, x, KT);
    const float u = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    // z = A x + B u
    acc[0] = 0.0f, acc[1] = 0.0f, acc[2] = 0.0f, acc[3] = 0.0f;
    dotv<N, true>(acc, x, Arow);
    dotv<M, true>(acc, u, Brow);
    const float z = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    // zeta = D^{-1/2} z;  x_c = D^{1/2} (S zeta + h);  y_c = g_c + D^{-1/2} (zeta - S zeta)
    const float zeta = z * sdi;
    acc[0] = 0.0f, acc[1] = 0.0f, acc[2] = 0.0f, acc[3] = 0.0f;
    dotv<N, true>(acc, zeta, Sr);
    const float sz = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    x = sdv * (sz + hh);
    y = __builtin_fmaf(sdi, zeta - sz, gg);
    if (valid) {
      float *si = ps + (long)i * VSTG;
      if (c < M)
        si[2 * N + c] = u;
      if (isM) {
        si[VSTG + c] = x;
        si[VSTG + N + c] = y;
      }
    }
  }
}

} // namespace qf32
} // namespace sipamd
