// chain_mt16_solve.hpp -- LQR::solve() for up to 16 right-hand sides against the factor state the factor sweep of
// chain_mt16.hpp (chain_factor_mt16) left, n = 32 on 16 x 16 matrix-core tiles, fp32 and fp64.
//
// One problem per wavefront, as in the fused kernel.  The right-hand sides are the 16 COLUMNS of a C/D tile: a
// vector quantity of the recursion (g, t, v, x, z, y: 32 x ncols) is a Pair of tiles, lane (j, g) register v of tile
// I holding element 16 I + row(g, v) of column j; the control quantities (h, k, u: m x ncols) are one tile with
// control g + 4 v in register v.  Every product is then a pattern the fused kernel already issues, with the
// tile pair in the place of a matrix operand:
//      g = v + W t              as  Z = W B                 (lqr.cpp:778-781)      16 MFMAs
//      h = r + B^T g            as  G = R + B^T Z           (lqr.cpp:783-784)       8
//      k = -G^-1 h              as  K = -G^-1 H             (lqr.cpp:785-791)       VM
//      v = q + A^T g + K^T h    as  V = Q + A^T F + K^T H   (lqr.cpp:793-794)      16 + 2 VM
// and in the rollout (lqr.cpp:821-870), with K^T, A^T, B^T and W fetched as the fused rollout fetches them,
//      u = k + K x   (8),   z = A x + B u   (16 + 2 VM),   y = g + W z   (16),   x+ = z + c - delta o y.
// No sweep, no LDS.  At m = 8 (VM = 2) the backward pass issues 46 MFMAs of 16x16x4 per stage and the rollout 44,
// each against ~ 19 KB of operands in fp64 (W, A, B, K, G^-1): the kernel is bound by the bytes it reads, and these
// do not depend on the number of columns.
//
// Tile columns >= ncols read zeros and store nothing.  A problem whose stored status is not 0 exits at once.
// Between the two passes g (per node) and k (per edge) of every column live
//   cws != nullptr:  in the column workspace, cws[problem][node i][column][g (32) | k of edge i (M)];
//   cws == nullptr:  (ncols == 1, sip_lqr_solve) in the g slot of the spill and the k part of `gains`, where the
//                    fused kernel keeps them.
// Every lane reads back exactly the elements it wrote itself.
#pragma once
#include "chain_mt16.hpp"

namespace sipamd {
namespace mt16 {

// acc.t[I] += (U^T X).t[I]: U 32 x 32 in tiles, X a 32 x 16 tile pair
template <typename S> __device__ __forceinline__ void mul_t_pair(const Mat32<S> &U, const Pair<S> &X, Pair<S> &acc) {
#pragma unroll
  for (int R = 0; R < 2; ++R)
#pragma unroll
    for (int v = 0; v < 4; ++v)
#pragma unroll
      for (int I = 0; I < 2; ++I)
        acc.t[I] = Tr<S>::mfma(U.t[R][I][v], X.t[R][v], acc.t[I]);
}

template <typename S, int M>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2)))
void chain_solve_mt16(const S *__restrict__ mats, const S *__restrict__ vecs_cols, S *sol_cols, S *gains, S *wsp,
                      const S *__restrict__ gfac, S *cws, const int *__restrict__ status, const long batch,
                      const int T, const int ncols, const long col_stride) {
  static_assert(M >= 1 && M <= 16, "controls live in registers 0 .. VM - 1 of the four lane groups: 16 tile rows");
  using TR = Tr<S>;
  using v4 = typename TR::v4;
  using LY = Layout<S, M>;
  constexpr int STG = LY::NODE + LY::EDGE, VSTG = LY::VNODE + LY::VEDGE, VM = LY::VM;
  constexpr bool VEC = LY::VEC_LOADS;
  constexpr unsigned ES = sizeof(S);
  constexpr int GF = M * M + M; // scalars of gfac per edge: -G^-1 (M x M, column-major) | M unused
  constexpr int CW = N + M;     // scalars of cws per (node, column)
  const long p = blockIdx.x;
  if (p >= batch || status[p] != 0)
    return; // (uniform over the wavefront) LQR::solve after a failed factor is undefined in the reference
  const int lane = threadIdx.x & 63, j = lane & 15, g = lane >> 4;
  const int acol = ctrl_of_col<S>(j); // control index of this lane's tile column (valid if < M)
  const bool colok = j < ncols;       // this lane's tile column is a right-hand side
  const long cj = colok ? j : 0;
  const long mats_len = (long)(T + 1) * LY::NODE + (long)T * LY::EDGE, vecs_len = (long)(T + 1) * LY::VNODE + (long)T * LY::VEDGE;
  const rsrc_t rM = make_rsrc(mats + p * mats_len, mats_len * ES);
  const rsrc_t rG = make_rsrc(gains + p * ((long)T * LY::GAIN), (long)T * LY::GAIN * ES);
  const rsrc_t rW = make_rsrc(wsp + p * ((long)(T + 1) * LY::WSN), (long)(T + 1) * LY::WSN * ES);
  const rsrc_t rF = make_rsrc(gfac + p * ((long)T * GF), (long)T * GF * ES);
  // the columns are col_stride scalars apart (a whole batch): 64-bit addresses, one base per lane
  const S *pv = vecs_cols + cj * col_stride + p * vecs_len;
  S *ps = sol_cols + cj * col_stride + p * vecs_len;
  S *pg, *pk; // g of node i: pg[i * gstride + row]; k of edge i: pk[i * kstride + control]
  long gstride, kstride;
  if (cws != nullptr) {
    pg = cws + (p * (long)(T + 1) * ncols + cj) * CW, gstride = (long)ncols * CW;
    pk = pg + N, kstride = gstride;
  } else {
    pg = wsp + p * ((long)(T + 1) * LY::WSN) + LY::WTILES * 256, gstride = LY::WSN;
    pk = gains + p * ((long)T * LY::GAIN) + M * N, kstride = LY::GAIN;
  }
  const unsigned acolc = (unsigned)(acol < M ? acol : 0);
  const unsigned uj = (unsigned)j, ug = (unsigned)g, r0 = (unsigned)TR::row(g, 0);
  const unsigned ocol = uj * N + r0;     // column-major tile: element (row(g, 0), j)
  const unsigned obcol = acolc * N + r0; // ... of B: the column of the control of tile column j
  const unsigned orow = r0 * N + uj;     // transposed tile (A^T): element (j, row(g, 0)) of A
  const unsigned octl = ug * N + uj;     // control rows: element (j, g) of B; control g + 4 v is 4 v N further
  auto ldM = [&](const unsigned vo, const unsigned so) { return Mem<S>::ld(rM, vo * ES, so * ES); };
  int arow[VM]; // control of register v, clamped into the block for the addresses
  bool aok[VM];
#pragma unroll
  for (int v = 0; v < VM; ++v) {
    const int a = ctrl_of(g, v);
    aok[v] = a < M, arow[v] = a < M ? a : M - 1;
  }

  // a 32-vector per column at scalar offset `off` of the problem's vecs / sol / g arrays: rows 16 I + row(g, v)
  auto ld_pair = [&](const S *base, const long off) {
    Pair<S> r;
#pragma unroll
    for (int I = 0; I < 2; ++I)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const S x = base[off + 16 * I + TR::row(g, v)];
        r.t[I][v] = colok ? x : S(0);
      }
    return r;
  };
  auto st_pair = [&](S *base, const long off, const Pair<S> &x) {
    if (colok) {
#pragma unroll
      for (int I = 0; I < 2; ++I)
#pragma unroll
        for (int v = 0; v < 4; ++v)
          base[off + 16 * I + TR::row(g, v)] = x.t[I][v];
    }
  };
  // an m-vector per column (r, k, u): control g + 4 v in register v < VM
  auto ld_ctl = [&](const S *base, const long off) {
    v4 r = zero4<S>();
#pragma unroll
    for (int v = 0; v < VM; ++v) {
      const S x = base[off + arow[v]];
      r[v] = (colok && aok[v]) ? x : S(0);
    }
    return r;
  };
  auto st_ctl = [&](S *base, const long off, const v4 x) {
#pragma unroll
    for (int v = 0; v < VM; ++v)
      if (colok && aok[v])
        base[off + arow[v]] = x[v];
  };
  // delta of node i by row (the same for every column)
  auto ld_delta = [&](const int i) {
    Pair<S> r;
#pragma unroll
    for (int I = 0; I < 2; ++I)
#pragma unroll
      for (int v = 0; v < 4; ++v)
        r.t[I][v] = ldM((unsigned)(N * N + 16 * I) + r0 + (unsigned)(TR::RSTEP * v), (unsigned)i * STG);
    return r;
  };
  // W of node i out of the factor's dump: tiles (0, 0), (1, 0), (1, 1) as they sat in the registers, tile (0, 1) =
  // tile (1, 0) transposed (element (row(g, v), 16 + j) is in register v' of lane (row(g, v), g'), row(g', v') = j)
  auto fetch_W = [&](const int i) {
    Mat32<S> W;
    const unsigned sW = (unsigned)i * LY::WSN * ES, vl = (unsigned)lane * 4u * ES;
    W.t[0][0] = Mem<S>::ld4(rW, vl, sW), W.t[1][0] = Mem<S>::ld4(rW, vl + 256u * ES, sW);
    W.t[1][1] = Mem<S>::ld4(rW, vl + 512u * ES, sW);
    const unsigned gq = TR::ROWS_CONTIGUOUS ? (uj >> 2) : (uj & 3u), vq = TR::ROWS_CONTIGUOUS ? (uj & 3u) : (uj >> 2);
    const unsigned ot = (16u * gq + r0) * 4u + vq;
#pragma unroll
    for (int v = 0; v < 4; ++v)
      W.t[0][1][v] = Mem<S>::ld(rW, (ot + (unsigned)((64 + TR::RSTEP * v) * 4)) * ES, sW);
    return W;
  };
  auto t_of = [&](const Pair<S> &c, const Pair<S> &dl, const Pair<S> &v) { // c - delta o v
    Pair<S> t;
#pragma unroll
    for (int I = 0; I < 2; ++I)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        t.t[I][r] = fma_(-dl.t[I][r], v.t[I][r], c.t[I][r]);
    return t;
  };

  // ---- backward affine sweep (lqr.cpp:738-796) ------------------------------------------------------------------
  // Operands of edge i: A, B as the fused backward loop loads them, K (m x 32: row = control g + 4 v) out of the
  // gains, -G^-1 out of gfac; of node i: q, c per column and delta.  One register set: what the next stage needs
  // is requested as soon as this stage has used the registers it lands in.
  Mat32<S> W, A;
  Pair<S> B, K, q, c, dl;
  v4 Gm, rv;
  auto fetch_B = [&](const int i) {
    const unsigned sB = (unsigned)i * STG + LY::NODE + N * N;
#pragma unroll
    for (int I = 0; I < 2; ++I) {
      if constexpr (VEC) {
        B.t[I] = Mem<S>::ld4(rM, (obcol + (unsigned)(16 * I)) * ES, sB * ES);
      } else {
#pragma unroll
        for (int v = 0; v < 4; ++v)
          B.t[I][v] = ldM(obcol + (unsigned)(16 * I + TR::RSTEP * v), sB);
      }
      if (acol >= M)
        B.t[I] = zero4<S>();
    }
    rv = ld_ctl(pv, (long)i * VSTG + LY::VNODE);
  };
  auto fetch_G = [&](const int i) {
    Gm = zero4<S>();
#pragma unroll
    for (int v = 0; v < VM; ++v) {
      const S x = Mem<S>::ld(rF, (acolc * M + (unsigned)arow[v]) * ES, (unsigned)i * GF * ES);
      Gm[v] = (aok[v] && acol < M) ? x : S(0);
    }
  };
  auto fetch_AK = [&](const int i) {
    A = load32<S, VEC>(rM, ocol, (unsigned)i * STG + LY::NODE);
    K.t[0] = zero4<S>(), K.t[1] = zero4<S>();
#pragma unroll
    for (int v = 0; v < VM; ++v) {
      const S k0 = Mem<S>::ld(rG, (uj * M + (unsigned)arow[v]) * ES, (unsigned)i * LY::GAIN * ES);
      const S k1 = Mem<S>::ld(rG, ((uj + 16u) * M + (unsigned)arow[v]) * ES, (unsigned)i * LY::GAIN * ES);
      K.t[0][v] = aok[v] ? k0 : S(0);
      K.t[1][v] = aok[v] ? k1 : S(0);
    }
  };
  auto fetch_node = [&](const int i) {
    q = ld_pair(pv, (long)i * VSTG), c = ld_pair(pv, (long)i * VSTG + N);
    dl = ld_delta(i);
  };

  fetch_node(T);
  W = fetch_W(T);
  Pair<S> v = q;               // v_T = q_T
  Pair<S> t = t_of(c, dl, v);  // t = c - delta o v
  if (T > 0) {
    fetch_B(T - 1), fetch_G(T - 1), fetch_AK(T - 1);
    fetch_node(T - 1);
  }
  for (int i = T - 1; i >= 0; --i) {
    // g = v_c + W t  (lqr.cpp:778-781), kept for the rollout
    Pair<S> gd = v;
    mul_t_pair<S>(W, t, gd);
    W = fetch_W(i);
    st_pair(pg, (long)(i + 1) * gstride, gd);
    // h = r + B^T g  (lqr.cpp:783-784)
    v4 h = rv;
#pragma unroll
    for (int R = 0; R < 2; ++R)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        h = TR::mfma(B.t[R][r], gd.t[R][r], h);
    if (i > 0)
      fetch_B(i - 1);
    // k = -G^-1 h  (lqr.cpp:785-791)
    v4 k = zero4<S>();
#pragma unroll
    for (int r = 0; r < VM; ++r)
      k = TR::mfma(Gm[r], h[r], k);
    if (i > 0)
      fetch_G(i - 1);
    st_ctl(pk, (long)i * kstride, k);
    // v = q + A^T g + K^T h  (lqr.cpp:793-794)
    v = q;
    mul_t_pair<S>(A, gd, v);
#pragma unroll
    for (int r = 0; r < VM; ++r) {
      v.t[0] = TR::mfma(K.t[0][r], h[r], v.t[0]);
      v.t[1] = TR::mfma(K.t[1][r], h[r], v.t[1]);
    }
    if (i > 0)
      fetch_AK(i - 1);
    t = t_of(c, dl, v);
    if (i > 0)
      fetch_node(i - 1);
  }

  // ---- root: g_0 = v_0 + W_0 t_0 ; x_0 = c_0 - delta_0 o g_0, y_0 = g_0 (lqr.cpp:798-819) ------------------------
  Pair<S> x;
  {
    Pair<S> g0 = v;
    mul_t_pair<S>(W, t, g0);
    x = t_of(c, dl, g0);
    st_pair(ps, 0, x);
    st_pair(ps, N, g0);
  }

  // ---- forward rollout (lqr.cpp:821-870) ------------------------------------------------------------------------
  // The products sum over the rows of the tile, so the operands are loaded transposed (K^T, A^T, B^T: rows = the
  // index summed over), as the fused rollout loads them; W is symmetric.
  Pair<S> KT;  // t[I]: K^T rows 16 I + row(g, v), control acol
  Mat32<S> AT; // A^T
  Pair<S> BT;  // t[J]: B^T rows = controls (registers < VM), columns 16 J + j
  Pair<S> gc, cc, dc;
  v4 ku;
  auto fetch_K = [&](const int i) {
    const unsigned so = (unsigned)i * LY::GAIN * ES;
#pragma unroll
    for (int I = 0; I < 2; ++I)
#pragma unroll
      for (int r = 0; r < 4; ++r) { // K(acol, row), row = 16 I + row(g, r)
        const S x_ = Mem<S>::ld(rG, (r0 * M + acolc + (unsigned)((16 * I + TR::RSTEP * r) * M)) * ES, so);
        KT.t[I][r] = acol < M ? x_ : S(0);
      }
    ku = ld_ctl(pk, (long)i * kstride);
  };
  auto fetch_ABT = [&](const int i) {
    const unsigned sE = (unsigned)i * STG + LY::NODE;
#pragma unroll
    for (int I = 0; I < 2; ++I)
#pragma unroll
      for (int r = 0; r < 4; ++r) { // A(j, row), row = 16 I + row(g, r)
        AT.t[I][0][r] = ldM(orow + (unsigned)((16 * I + TR::RSTEP * r) * N), sE);
        AT.t[I][1][r] = ldM(orow + (unsigned)((16 * I + TR::RSTEP * r) * N + 16), sE);
      }
    BT.t[0] = zero4<S>(), BT.t[1] = zero4<S>();
#pragma unroll
    for (int r = 0; r < VM; ++r) { // B(j, a), a = g + 4 r
      const unsigned ob = uj + (unsigned)(N * N + arow[r] * N);
      const S b0 = ldM(ob, sE), b1 = ldM(ob + 16u, sE);
      BT.t[0][r] = aok[r] ? b0 : S(0);
      BT.t[1][r] = aok[r] ? b1 : S(0);
    }
  };
  auto fetch_child = [&](const int i) { // W, g and the node vectors of node i + 1
    W = fetch_W(i + 1);
    gc = ld_pair(pg, (long)(i + 1) * gstride);
    cc = ld_pair(pv, (long)(i + 1) * VSTG + N);
    dc = ld_delta(i + 1);
  };
  if (T > 0) {
    fetch_K(0);
    fetch_ABT(0);
    fetch_child(0);
  }
  for (int i = 0; i < T; ++i) {
    const bool more = i + 1 < T;
    // u = k + K x
    v4 u = ku;
#pragma unroll
    for (int R = 0; R < 2; ++R)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        u = TR::mfma(KT.t[R][r], x.t[R][r], u);
    if (more)
      fetch_K(i + 1);
    st_ctl(ps, (long)i * VSTG + 2 * N, u);
    // z = A x + B u
    Pair<S> z;
    z.t[0] = zero4<S>(), z.t[1] = zero4<S>();
    mul_t_pair<S>(AT, x, z);
#pragma unroll
    for (int r = 0; r < VM; ++r) {
      z.t[0] = TR::mfma(BT.t[0][r], u[r], z.t[0]);
      z.t[1] = TR::mfma(BT.t[1][r], u[r], z.t[1]);
    }
    if (more)
      fetch_ABT(i + 1);
    // y_c = g_c + W_c z ; x_c = z + c_c - delta_c o y_c
    Pair<S> y = gc;
    mul_t_pair<S>(W, z, y);
#pragma unroll
    for (int I = 0; I < 2; ++I)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        x.t[I][r] = z.t[I][r] + fma_(-dc.t[I][r], y.t[I][r], cc.t[I][r]);
    if (more)
      fetch_child(i + 1);
    st_pair(ps, (long)(i + 1) * VSTG, x);
    st_pair(ps, (long)(i + 1) * VSTG + N, y);
  }
}

} // namespace mt16

// The launcher of mt16_launch.hpp for the kernel above (instantiated in chain_mt16_solve.hip and
// chain_mt16_wide_solve.hip).
template <typename S, int M>
hipError_t launch_mt16_solve(long batch, int T, const void *mats, const void *vecs_cols, void *sol_cols, void *gains,
                             void *ws, const void *gfac, void *cws, const int32_t *status, int ncols, long col_stride,
                             hipStream_t stream) {
  if (ncols < 1 || ncols > kMt16SolveColumns || (cws == nullptr && ncols != 1))
    return hipErrorInvalidValue;
  // 16-byte loads of the stage blocks (fp32, even m) and of the W dump: bases must be 16-byte aligned
  if (((uintptr_t)mats | (uintptr_t)ws) & 15)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL((mt16::chain_solve_mt16<S, M>), dim3((unsigned)batch), dim3(64), 0, stream, (const S *)mats,
                     (const S *)vecs_cols, (S *)sol_cols, (S *)gains, (S *)ws, (const S *)gfac, (S *)cws,
                     (const int *)status, batch, T, ncols, col_stride);
  return hipGetLastError();
}

} // namespace sipamd
