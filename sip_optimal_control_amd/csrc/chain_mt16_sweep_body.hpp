// chain_mt16_sweep_body.hpp -- the body of the n = 32 matrix-core chain sweep, included by chain_mt16.hpp INSIDE its
// two kernels (no include guard: it is text, not declarations).  The including function provides
//   S, M, FACTOR (constexpr bool), mats, vecs, sol, gains, wsp, gfac, status, batch, T (and `stamps` in the diagnostic build).
// FACTOR = false: the fused factor + solve.  FACTOR = true: the backward matrix sweep alone -- no right-hand side is
// read, no vector of the affine sweep computed, no rollout; it leaves W per node in the spill, K in the gains, -G^-1
// per edge in `gfac` (M x M column-major, M * M + M scalars per edge) and the statuses: the state chain_solve_mt16
// (chain_mt16_solve.hpp) solves against.  The text is shared by inclusion, not through a function template called
// from both kernels: the fused kernel's register allocation is tuned to the last VGPR, and any change of the
// function structure around it moves it.
#ifndef SIP_MT16_SWEEP_BODY
#error "chain_mt16_sweep_body.hpp is the text of the two kernels of chain_mt16.hpp: include it only where they do"
#endif
  static_assert(M >= 1 && M <= 16, "controls live in registers 0 .. VM - 1 of the four lane groups: 16 tile rows");
#ifdef SIP_MT16_STAMPS
  unsigned long long seg_[16] = {0}, last_ = __builtin_amdgcn_s_memtime();
  const unsigned long long start_ = last_;
#endif
  using TR = Tr<S>;
  using v4 = typename TR::v4;
  using LY = Layout<S, M>;
  constexpr int STG = LY::NODE + LY::EDGE, VSTG = LY::VNODE + LY::VEDGE, VM = LY::VM;
  constexpr bool VEC = LY::VEC_LOADS;
  const long p = blockIdx.x;
  if (p >= batch)
    return;
  LaneT<S> L;
  L.lane = threadIdx.x & 63, L.j = L.lane & 15, L.g = L.lane >> 4;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if constexpr (sizeof(S) == 4) {
      L.mg[k] = opaque_mask(L.g == k);
      L.mj[k] = opaque_mask(L.j == TR::row(k, 0));
    } else {
      L.eg[k] = L.g == k ? S(1) : S(0);
      L.ej[k] = L.j == TR::row(k, 0) ? S(1) : S(0);
    }
  }
  const int j = L.j, g = L.g;
  const int acol = ctrl_of_col<S>(j); // control index of this lane's tile column (valid if < M)
  constexpr unsigned ES = sizeof(S);
  const long mats_len = (long)(T + 1) * LY::NODE + (long)T * LY::EDGE, vecs_len = (long)(T + 1) * LY::VNODE + (long)T * LY::VEDGE;
  // one buffer descriptor per array, based at this wavefront's problem (SGPRs); every access below is
  // descriptor + 32-bit lane offset + stage offset (SGPR) + immediate
  const rsrc_t rM = make_rsrc(mats + p * mats_len, mats_len * ES), rV = make_rsrc(vecs + p * vecs_len, vecs_len * ES);
  const rsrc_t rS = make_rsrc(sol + p * vecs_len, vecs_len * ES);
  const rsrc_t rG = make_rsrc(gains + p * ((long)T * LY::GAIN), (long)T * LY::GAIN * ES);
  const rsrc_t rW = make_rsrc(wsp + p * ((long)(T + 1) * LY::WSN), (long)(T + 1) * LY::WSN * ES);
  const unsigned acolc = (unsigned)(acol < M ? acol : 0);
  const unsigned uj = (unsigned)j, ug = (unsigned)g, r0 = (unsigned)TR::row(g, 0);
  const unsigned ocol = uj * N + r0;     // column-major tile: element (row(g, 0), j)
  const unsigned obcol = acolc * N + r0; // ... of B: the column of the control of tile column j
  const unsigned orow = r0 * N + uj;     // transposed tile (A^T): element (j, row(g, 0)) of A
  const unsigned octl = ug * N + uj;     // control rows: element (j, g) of B or M; control g + 4 v is 4 v N further
  constexpr unsigned RS = (unsigned)TR::RSTEP;
  auto ldM = [&](const unsigned vo, const unsigned so) { return Mem<S>::ld(rM, vo * ES, so * ES); };
  auto ldV = [&](const unsigned vo, const unsigned so) { return Mem<S>::ld(rV, vo * ES, so * ES); };

  constexpr int MH = M <= 8 ? 8 : 16; // entries of the control vectors h and u: every control register of the lanes
  __shared__ S s_v[N], s_t[N], s_g[N], s_sd[N], s_sdi[N], s_x[N], s_z[N], s_gs[16], s_h[MH], s_u[MH];
  constexpr int LDM = TR::ROWS_CONTIGUOUS ? 36 : 33; // column stride of the mirror image (bank spread; 16-byte columns)
  __shared__ __attribute__((aligned(16))) S s_m[N * LDM];
  __shared__ __attribute__((aligned(16))) S s_p[16]; // pivot block of the sweep's current step


  if constexpr (!FACTOR) {
    if (L.lane < MH)
      s_h[L.lane] = S(0), s_u[L.lane] = S(0); // the entries of no control are read as zeros
  }
  int stat = 0;
  Mat32<S> W, V;

  // ---- node tail: F = I + D^1/2 V D^1/2, its sweep, W (lqr.cpp:487-529, 722-727), plus the vector
  // term t = c - delta o v for the parent step.
  auto finish_node = [&](const int i, const S dl0, const S dl1, const S c0, const S c1) {
    if (stat == 0 && __any(!(dl0 > S(0)) || !(dl1 > S(0))))
      stat = 1; // INVALID_DELTA
    const S sd0 = TR::sqrt(dl0), sd1 = TR::sqrt(dl1);
    const S sdi0 = S(1) / sd0, sdi1 = S(1) / sd1;
    if (g == 0) {
      s_sd[j] = sd0, s_sd[16 + j] = sd1;
      s_sdi[j] = sdi0, s_sdi[16 + j] = sdi1;
      if constexpr (!FACTOR) {
        s_t[j] = c0 - dl0 * s_v[j]; // c - delta o v   (lqr.cpp:778-779, negated)
        s_t[16 + j] = c1 - dl1 * s_v[16 + j];
      }
    }
    SIP_MT16_STAMP(7);
    // Only the lower triangle of V counts (Eigen::LLT reads nothing else, lqr.cpp:505): mirror it through
    // LDS.  V = Q + A^T F + K^T H is symmetric only up to rounding, the sweep reads rows as columns, and the
    // recursion does not damp an antisymmetric part (the feedback term K^T H is symmetric by construction):
    // left alone it grows by |A|^2 per stage.
#pragma unroll
    for (int I = 0; I < 2; ++I)
#pragma unroll
      for (int J = 0; J <= I; ++J) { // tile (0, 1) is not read back
        S *col = s_m + (16 * J + j) * LDM + 16 * I;
        if constexpr (TR::ROWS_CONTIGUOUS) {
          *(v4 *)(col + 4 * g) = V.t[I][J];
        } else {
#pragma unroll
          for (int v = 0; v < 4; ++v)
            col[TR::row(g, v)] = V.t[I][J][v];
        }
      }
    lds_order();
#pragma unroll
    for (int I = 0; I < 2; ++I)
#pragma unroll
      for (int J = I; J < 2; ++J)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int r = 16 * I + TR::row(g, v), c = 16 * J + j;
          const S mirrored = s_m[r * LDM + c]; // element (c, r)
          V.t[I][J][v] = (J > I || r < c) ? mirrored : V.t[I][J][v];
        }
    // F = I + sd V sd (lqr.cpp:497-503), in place
    {
      const v4 sr[2] = {by_row<S>(s_sd, 0, g), by_row<S>(s_sd, 1, g)};
#pragma unroll
      for (int I = 0; I < 2; ++I)
#pragma unroll
        for (int J = 0; J < 2; ++J)
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const bool dg = I == J && j == TR::row(g, v);
            V.t[I][J][v] = fma_(V.t[I][J][v] * sr[I][v], J == 0 ? sd0 : sd1, dg ? S(1) : S(0));
          }
    }
    SIP_MT16_STAMP(8);
    // The factor sweep alone, and the fused sweep in fp64, sweep the unit-diagonal S F S, S = diag(F)^-1/2, and scale
    // back, as the G sweep below does: the sweep's modified operands work against an identity on the pivot block, and
    // the F of a condensed Newton-KKT problem (V ~ J^T R2^-1 J) has a diagonal far from 1.  (A diagonal <= 0 gives a
    // NaN scale: the sweep then fails, as it must.)  The fp32 fused kernel of m <= 8 keeps its sweep of F as it stands:
    // its register allocation is tuned to the last VGPR.  The wide rows (m > 8) have no such budget: they scale.
    constexpr bool SCALE_F = FACTOR || sizeof(S) == 8 || M > 8;
    S fs0 = S(1), fs1 = S(1);
    if constexpr (SCALE_F) {
      S d0 = S(0), d1 = S(0);
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        d0 += j == TR::row(g, v) ? V.t[0][0][v] : S(0);
        d1 += j == TR::row(g, v) ? V.t[1][1][v] : S(0);
      }
      fs0 = TR::rsqrt(sum_groups(d0)), fs1 = TR::rsqrt(sum_groups(d1)); // of tile columns j and 16 + j
      if (g == 0)
        s_x[j] = fs0, s_x[16 + j] = fs1; // (s_x is the rollout's, first written after the backward sweep: free here)
      lds_order();
      const v4 fr[2] = {by_row<S>(s_x, 0, g), by_row<S>(s_x, 1, g)};
      lds_order();
#pragma unroll
      for (int I = 0; I < 2; ++I)
#pragma unroll
        for (int J = 0; J < 2; ++J)
#pragma unroll
          for (int v = 0; v < 4; ++v)
            V.t[I][J][v] *= fr[I][v] * (J == 0 ? fs0 : fs1);
      const bool ffail_scaled = sweep<S, 2, 4>(V.t, L, s_p);
#pragma unroll
      for (int I = 0; I < 2; ++I)
#pragma unroll
        for (int J = 0; J < 2; ++J)
#pragma unroll
          for (int v = 0; v < 4; ++v)
            V.t[I][J][v] *= fr[I][v] * (J == 0 ? fs0 : fs1);
      if (stat == 0 && ffail_scaled)
        stat = 2; // F_FACTORIZATION_FAILURE
    }
    const bool ffail = SCALE_F ? false : sweep<S, 2, 4>(V.t, L, s_p); // V now holds -F^-1
    SIP_MT16_STAMP(9);
    if (stat == 0 && ffail)
      stat = 2; // F_FACTORIZATION_FAILURE
    // W = D^-1/2 (I - F^-1) D^-1/2
    {
      const v4 ir[2] = {by_row<S>(s_sdi, 0, g), by_row<S>(s_sdi, 1, g)};
#pragma unroll
      for (int I = 0; I < 2; ++I)
#pragma unroll
        for (int J = 0; J < 2; ++J)
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const bool dg = I == J && j == TR::row(g, v);
            W.t[I][J][v] = (V.t[I][J][v] + (dg ? S(1) : S(0))) * (ir[I][v] * (J == 0 ? sdi0 : sdi1));
          }
    }
    // spill W for the rollout: W is symmetric, tile (0, 1) is read back out of the dump of tile (1, 0)
    {
      const unsigned so = (unsigned)i * LY::WSN * ES, vo = (unsigned)L.lane * 4u * ES;
      Mem<S>::st4(W.t[0][0], rW, vo, so);
      Mem<S>::st4(W.t[1][0], rW, vo + 256u * ES, so);
      Mem<S>::st4(W.t[1][1], rW, vo + 512u * ES, so);
    }
    lds_order();
    SIP_MT16_STAMP(10);
  };

  // ---- terminal node -------------------------------------------------------------------------
  {
    const unsigned sM = (unsigned)T * STG, sV = (unsigned)T * VSTG;
    V = load32<S, VEC>(rM, ocol, sM);
    if constexpr (!FACTOR) {
      const S qT0 = ldV(uj, sV), qT1 = ldV(uj + 16u, sV);
      if (g == 0)
        s_v[j] = qT0, s_v[16 + j] = qT1; // v = q
    }
    const S dl0 = ldM(uj + (unsigned)(N * N), sM), dl1 = ldM(uj + (unsigned)(N * N + 16), sM);
    S c0 = S(0), c1 = S(0);
    if constexpr (!FACTOR)
      c0 = ldV(uj + (unsigned)N, sV), c1 = ldV(uj + (unsigned)(N + 16), sV);
    lds_order();
    finish_node(T, dl0, dl1, c0, c1);
  }

  // ---- backward recursion --------------------------------------------------------------------
  for (int i = T - 1; i >= 0; --i) {
    // element offsets of the stage's blocks inside the problem (SGPRs)
    const unsigned sN = (unsigned)i * STG, sE = sN + LY::NODE, sB = sE + N * N, sMm = sB + N * M, sR = sMm + N * M;
    const unsigned sV = (unsigned)i * VSTG;
    const Mat32<S> A = load32<S, VEC>(rM, ocol, sE);
    // the node's and the edge's vectors: requested here, used at the bottom of the stage
    const S dl0 = ldM(uj + (unsigned)(N * N), sN), dl1 = ldM(uj + (unsigned)(N * N + 16), sN);
    S c0 = S(0), c1 = S(0), q0 = S(0), q1 = S(0), rv = S(0);
    if constexpr (!FACTOR) {
      c0 = ldV(uj + (unsigned)N, sV), c1 = ldV(uj + (unsigned)(N + 16), sV);
      q0 = ldV(uj, sV), q1 = ldV(uj + 16u, sV), rv = ldV(acolc + (unsigned)LY::VNODE, sV);
    }
    // B (32 x M, ld 32): control acol on tile column j; columns of no control are zero
    Pair<S> B;
#pragma unroll
    for (int I = 0; I < 2; ++I) {
      if constexpr (VEC) {
        B.t[I] = Mem<S>::ld4(rM, (obcol + (unsigned)(16 * I)) * ES, sB * ES);
      } else {
#pragma unroll
        for (int v = 0; v < 4; ++v)
          B.t[I][v] = ldM(obcol + (unsigned)(16 * I) + RS * v, sB);
      }
      if (acol >= M)
        B.t[I] = zero4<S>();
    }
    // H starts as M^T (row = control ctrl_of(g, v), column 16 J + j), G as R with an identity on the
    // rows / columns of no control
    Pair<S> H;
    v4 G;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int a = ctrl_of(g, v);
      const bool ok = v < VM && a < M;
      if (v < VM) { // unconditional loads (a row a >= M of the 8-row window lies in the blocks behind: read, dropped)
        const S h0 = ldM(octl + (unsigned)(4 * v * N), sMm), h1 = ldM(octl + (unsigned)(4 * v * N + 16), sMm);
        const S rr = ldM(acolc * M + ug + (unsigned)(4 * v), sR);
        H.t[0][v] = ok ? h0 : S(0);
        H.t[1][v] = ok ? h1 : S(0);
        G[v] = (ok && acol < M) ? rr : (j == TR::row(g, v) ? S(1) : S(0));
      } else {
        H.t[0][v] = S(0), H.t[1][v] = S(0);
        G[v] = j == TR::row(g, v) ? S(1) : S(0);
      }
    }
    // g = v_c + W t   (lqr.cpp:778-781)
    if constexpr (!FACTOR) {
      const v4 tr[2] = {by_row<S>(s_t, 0, g), by_row<S>(s_t, 1, g)};
      S w0 = S(0), w1 = S(0);
      mat_t_vec<S>(W, tr, w0, w1);
      const S g0 = s_v[j] + sum_groups(w0), g1 = s_v[16 + j] + sum_groups(w1);
      if (g == 0) {
        s_g[j] = g0, s_g[16 + j] = g1;
        const unsigned so = ((unsigned)(i + 1) * LY::WSN + LY::WTILES * 256) * ES;
        Mem<S>::st(g0, rW, uj * ES, so);
        Mem<S>::st(g1, rW, (uj + 16u) * ES, so);
      }
    }
    SIP_MT16_STAMP(0);
    Mat32<S> F;
    Pair<S> Z;
#pragma unroll
    for (int I = 0; I < 2; ++I) {
      Z.t[I] = zero4<S>();
#pragma unroll
      for (int J = 0; J < 2; ++J)
        F.t[I][J] = zero4<S>();
    }
    // Z = W B and F = W A, interleaved: six independent accumulators
#pragma unroll
    for (int R = 0; R < 2; ++R)
#pragma unroll
      for (int v = 0; v < 4; ++v)
#pragma unroll
        for (int I = 0; I < 2; ++I) {
          Z.t[I] = TR::mfma(W.t[R][I][v], B.t[R][v], Z.t[I]);
#pragma unroll
          for (int J = 0; J < 2; ++J)
            F.t[I][J] = TR::mfma(W.t[R][I][v], A.t[R][J][v], F.t[I][J]);
        }
    // G = R + B^T Z, H = M^T + B^T F
#pragma unroll
    for (int R = 0; R < 2; ++R)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        G = TR::mfma(B.t[R][v], Z.t[R][v], G);
        H.t[0] = TR::mfma(B.t[R][v], F.t[R][0][v], H.t[0]);
        H.t[1] = TR::mfma(B.t[R][v], F.t[R][1][v], H.t[1]);
      }
    SIP_MT16_STAMP(1);
    v4 gr[2];
    // h = r + B^T g  (lqr.cpp:783-784): control acol on the lanes of tile column j
    if constexpr (!FACTOR) {
      lds_order(); // s_g
      gr[0] = by_row<S>(s_g, 0, g), gr[1] = by_row<S>(s_g, 1, g);
      S pb = S(0);
#pragma unroll
      for (int I = 0; I < 2; ++I)
#pragma unroll
        for (int v = 0; v < 4; ++v)
          pb = fma_(B.t[I][v], gr[I][v], pb);
      pb = sum_groups(pb);
      if (g == 0 && acol < M)
        s_h[acol] = rv + pb;
    }
    SIP_MT16_STAMP(2);
    // LLT of G (lqr.cpp:696-701) as a sweep: G <- -G^-1 on the control rows / columns.  The sweep's modified
    // operands work against an identity on the pivot block, which costs accuracy when the pivots are far from
    // 1 (G ~ R is not scaled like F = I + ...): sweep the unit-diagonal S G S, S = diag(G)^-1/2, and scale back.
    {
      S dsel = S(0);
#pragma unroll
      for (int v = 0; v < 4; ++v)
        dsel += j == TR::row(g, v) ? G[v] : S(0);
      const S sc = TR::rsqrt(sum_groups(dsel)); // of tile column j; NaN for a diagonal <= 0: the sweep then fails
      if (g == 0)
        s_gs[j] = sc;
      lds_order();
      const v4 sr = by_row<S>(s_gs, 0, g);
      v4 Gt[1][1];
#pragma unroll
      for (int v = 0; v < 4; ++v)
        Gt[0][0][v] = G[v] * (sr[v] * sc);
      const bool gfail = sweep<S, 1, VM>(Gt, L, s_p);
#pragma unroll
      for (int v = 0; v < 4; ++v)
        G[v] = Gt[0][0][v] * (sr[v] * sc);
      if (stat == 0 && gfail)
        stat = 3; // G_FACTORIZATION_FAILURE
      if constexpr (FACTOR) { // -G^-1 for the separate solve: element (control g + 4 v, control acol)
        const rsrc_t rF = make_rsrc(gfac + p * ((long)T * (M * M + M)), (long)T * (M * M + M) * ES);
#pragma unroll
        for (int v = 0; v < VM; ++v)
          if (ctrl_of(g, v) < M && acol < M)
            Mem<S>::st(G[v], rF, (acolc * M + ug + (unsigned)(4 * v)) * ES, (unsigned)i * (M * M + M) * ES);
      }
    }
    SIP_MT16_STAMP(3);
    // K = -G^-1 H   (lqr.cpp:707-713); -G^-1 symmetric
    Pair<S> K;
    K.t[0] = zero4<S>(), K.t[1] = zero4<S>();
#pragma unroll
    for (int v = 0; v < VM; ++v) {
      K.t[0] = TR::mfma(G[v], H.t[0][v], K.t[0]);
      K.t[1] = TR::mfma(G[v], H.t[1][v], K.t[1]);
    }
    S hr[VM];
    S kb = S(0);
    if constexpr (!FACTOR) {
      lds_order(); // s_h
#pragma unroll
      for (int v = 0; v < VM; ++v)
        hr[v] = s_h[ctrl_of(g, v)]; // entries >= M stay zero
      // k = -G^-1 h   (lqr.cpp:785-791), control acol on tile column j
#pragma unroll
      for (int v = 0; v < VM; ++v)
        kb = fma_(G[v], hr[v], kb);
      kb = sum_groups(kb);
    }
    // gains out: K (m x 32 column-major) | k
    {
      const unsigned so = (unsigned)i * LY::GAIN * ES;
#pragma unroll
      for (int v = 0; v < VM; ++v)
        if (ctrl_of(g, v) < M) {
          Mem<S>::st(K.t[0][v], rG, (uj * M + ug + (unsigned)(4 * v)) * ES, so);
          Mem<S>::st(K.t[1][v], rG, (uj * M + ug + (unsigned)(4 * v + 16 * M)) * ES, so);
        }
      if constexpr (!FACTOR) {
        if (g == 0 && acol < M)
          Mem<S>::st(kb, rG, (acolc + (unsigned)(M * N)) * ES, so);
      }
    }
    // v = q + A^T g + K^T h   (lqr.cpp:793-794)
    if constexpr (!FACTOR) {
      S p0 = S(0), p1 = S(0);
      mat_t_vec<S>(A, gr, p0, p1);
#pragma unroll
      for (int v = 0; v < VM; ++v) {
        p0 = fma_(K.t[0][v], hr[v], p0);
        p1 = fma_(K.t[1][v], hr[v], p1);
      }
      const S vn0 = q0 + sum_groups(p0), vn1 = q1 + sum_groups(p1);
      lds_order(); // everyone is done with s_v / s_t / s_g of the child
      if (g == 0)
        s_v[j] = vn0, s_v[16 + j] = vn1;
    }
    SIP_MT16_STAMP(4);
    // V = Q + A^T F + K^T H   (lqr.cpp:715-719): tiles (0, 0), (1, 0), (1, 1) only -- the node tail keeps the lower
    // triangle and mirrors it, so tile (0, 1) is never read (10 MFMAs and a 16-byte load less per stage)
    {
      const Mat32<S> Qm = load32<S, VEC>(rM, ocol, sN); // (its tile (0, 1) is dead code)
      V.t[0][0] = Qm.t[0][0], V.t[1][0] = Qm.t[1][0], V.t[1][1] = Qm.t[1][1];
    }
#pragma unroll
    for (int R = 0; R < 2; ++R)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        V.t[0][0] = TR::mfma(A.t[R][0][v], F.t[R][0][v], V.t[0][0]);
        V.t[1][0] = TR::mfma(A.t[R][1][v], F.t[R][0][v], V.t[1][0]);
        V.t[1][1] = TR::mfma(A.t[R][1][v], F.t[R][1][v], V.t[1][1]);
      }
#pragma unroll
    for (int v = 0; v < VM; ++v) {
      V.t[0][0] = TR::mfma(K.t[0][v], H.t[0][v], V.t[0][0]);
      V.t[1][0] = TR::mfma(K.t[1][v], H.t[0][v], V.t[1][0]);
      V.t[1][1] = TR::mfma(K.t[1][v], H.t[1][v], V.t[1][1]);
    }
    lds_order();
    SIP_MT16_STAMP(5);
    finish_node(i, dl0, dl1, c0, c1);
  }
#ifdef SIP_MT16_STAMPS
  const unsigned long long back_end_ = __builtin_amdgcn_s_memtime();
#endif

  // ---- root: g_0 = v_0 + W_0 t_0 ; x_0 = c_0 - delta_0 o g_0, y_0 = g_0 -----------------------
  if constexpr (!FACTOR) {
    const v4 tr[2] = {by_row<S>(s_t, 0, g), by_row<S>(s_t, 1, g)};
    S w0 = S(0), w1 = S(0);
    mat_t_vec<S>(W, tr, w0, w1);
    const S g0 = s_v[j] + sum_groups(w0), g1 = s_v[16 + j] + sum_groups(w1);
    if (g == 0) {
      const S x0 = ldV(uj + (unsigned)N, 0u) - ldM(uj + (unsigned)(N * N), 0u) * g0;
      const S x1 = ldV(uj + (unsigned)(N + 16), 0u) - ldM(uj + (unsigned)(N * N + 16), 0u) * g1;
      Mem<S>::st(x0, rS, uj * ES, 0u), Mem<S>::st(x1, rS, (uj + 16u) * ES, 0u);
      Mem<S>::st(g0, rS, (uj + (unsigned)N) * ES, 0u), Mem<S>::st(g1, rS, (uj + (unsigned)(N + 16)) * ES, 0u);
      s_x[j] = x0, s_x[16 + j] = x1;
    }
  }
  if (L.lane == 0)
    status[p] = stat;
  lds_order();

  if constexpr (!FACTOR) {
  // ---- forward rollout (lqr.cpp:821-870) -----------------------------------------------------
  // The products sum over the rows of the tile, so the operands are loaded transposed (K^T, A^T, B^T:
  // rows = the index summed over); W is symmetric.  Nothing a stage reads from memory depends on x:
  // every operand of stage i + 1 is requested as soon as stage i has used the registers it lands in
  // (one register set, a stage of lead time).
  Pair<S> KT;   // t[I]: K^T rows 16 I + row(g, v), control acol
  Mat32<S> AT;  // A^T
  Pair<S> BT;   // t[J]: B^T rows = controls (registers < VM), columns 16 J + j
  Mat32<S> Wc;  // W of the child
  S kb, gc0, gc1, cc0, cc1, dc0, dc1;
  auto fetch_K = [&](const int i) {
    const unsigned so = (unsigned)i * LY::GAIN * ES;
#pragma unroll
    for (int I = 0; I < 2; ++I)
#pragma unroll
      for (int v = 0; v < 4; ++v) // K(acol, r), r = 16 I + row(g, v); lanes of no control: unused
        KT.t[I][v] = Mem<S>::ld(rG, (r0 * M + acolc + (unsigned)((16 * I + TR::RSTEP * v) * M)) * ES, so);
    kb = Mem<S>::ld(rG, (acolc + (unsigned)(M * N)) * ES, so);
  };
  auto fetch_AB = [&](const int i) {
    const unsigned sE = (unsigned)i * STG + LY::NODE;
#pragma unroll
    for (int I = 0; I < 2; ++I)
#pragma unroll
      for (int v = 0; v < 4; ++v) { // A(j, r), r = 16 I + row(g, v)
        AT.t[I][0][v] = ldM(orow + (unsigned)((16 * I + TR::RSTEP * v) * N), sE);
        AT.t[I][1][v] = ldM(orow + (unsigned)((16 * I + TR::RSTEP * v) * N + 16), sE);
      }
#pragma unroll
    for (int v = 0; v < VM; ++v) {
      const int a = ctrl_of(g, v);
      // B(j, a), a = g + 4 v (a row a >= M of the window lies in the blocks behind B: read, then dropped)
      const S b0 = ldM(octl + (unsigned)(N * N + 4 * v * N), sE), b1 = ldM(octl + (unsigned)(N * N + 4 * v * N + 16), sE);
      BT.t[0][v] = a < M ? b0 : S(0);
      BT.t[1][v] = a < M ? b1 : S(0);
    }
  };
  auto fetch_W = [&](const int i) { // the child's W, g and the node vectors of the child
    const unsigned sN1 = (unsigned)(i + 1) * STG, sV1 = (unsigned)(i + 1) * VSTG, sW = (unsigned)(i + 1) * LY::WSN;
    const unsigned vl = (unsigned)L.lane * 4u * ES;
    Wc.t[0][0] = Mem<S>::ld4(rW, vl, sW * ES), Wc.t[1][0] = Mem<S>::ld4(rW, vl + 256u * ES, sW * ES);
    Wc.t[1][1] = Mem<S>::ld4(rW, vl + 512u * ES, sW * ES);
    // tile (0, 1) = tile (1, 0) transposed: element (row(g, v), 16 + j) is W(16 + j, row(g, v)), which the dump of
    // tile (1, 0) holds in register v' of lane (row(g, v), g') with row(g', v') = j
    {
      const unsigned gq = TR::ROWS_CONTIGUOUS ? (uj >> 2) : (uj & 3u), vq = TR::ROWS_CONTIGUOUS ? (uj & 3u) : (uj >> 2);
      const unsigned ot = (16u * gq + r0) * 4u + vq;
#pragma unroll
      for (int v = 0; v < 4; ++v)
        Wc.t[0][1][v] = Mem<S>::ld(rW, (ot + (unsigned)((64 + TR::RSTEP * v) * 4)) * ES, sW * ES);
    }
    gc0 = Mem<S>::ld(rW, (uj + (unsigned)(LY::WTILES * 256)) * ES, sW * ES);
    gc1 = Mem<S>::ld(rW, (uj + (unsigned)(LY::WTILES * 256 + 16)) * ES, sW * ES);
    cc0 = ldV(uj + (unsigned)N, sV1), cc1 = ldV(uj + (unsigned)(N + 16), sV1);
    dc0 = ldM(uj + (unsigned)(N * N), sN1), dc1 = ldM(uj + (unsigned)(N * N + 16), sN1);
  };
  if (T > 0) {
    fetch_K(0);
    fetch_AB(0);
    fetch_W(0);
  }
  for (int i = 0; i < T; ++i) {
    const bool more = i + 1 < T;
    const v4 xr[2] = {by_row<S>(s_x, 0, g), by_row<S>(s_x, 1, g)};
    // u = k + K x : control acol on tile column j
    S pu = S(0);
#pragma unroll
    for (int I = 0; I < 2; ++I)
#pragma unroll
      for (int v = 0; v < 4; ++v)
        pu = fma_(KT.t[I][v], xr[I][v], pu);
    const S ub = kb + sum_groups(pu);
    if (more)
      fetch_K(i + 1);
    if (g == 0 && acol < M)
      s_u[acol] = ub;
    lds_order();
    // z = A x + B u
    S z0 = S(0), z1 = S(0);
    mat_t_vec<S>(AT, xr, z0, z1);
#pragma unroll
    for (int v = 0; v < VM; ++v) {
      const S ur = s_u[ctrl_of(g, v)]; // entries >= M stay zero
      z0 = fma_(BT.t[0][v], ur, z0);
      z1 = fma_(BT.t[1][v], ur, z1);
    }
    if (more)
      fetch_AB(i + 1);
    z0 = sum_groups(z0), z1 = sum_groups(z1);
    if (g == 0)
      s_z[j] = z0, s_z[16 + j] = z1;
    lds_order();
    // y_c = g_c + W_c z ; x_c = z + c_c - delta_c o y_c
    const v4 zr[2] = {by_row<S>(s_z, 0, g), by_row<S>(s_z, 1, g)};
    S y0 = S(0), y1 = S(0);
    mat_t_vec<S>(Wc, zr, y0, y1);
    y0 = gc0 + sum_groups(y0), y1 = gc1 + sum_groups(y1);
    const S xn0 = z0 + (cc0 - dc0 * y0), xn1 = z1 + (cc1 - dc1 * y1);
    if (more)
      fetch_W(i + 1);
    if (g == 0) {
      const unsigned so = (unsigned)i * VSTG * ES;
      if (acol < M)
        Mem<S>::st(ub, rS, (acolc + (unsigned)(2 * N)) * ES, so);
      Mem<S>::st(xn0, rS, (uj + (unsigned)VSTG) * ES, so), Mem<S>::st(xn1, rS, (uj + (unsigned)(VSTG + 16)) * ES, so);
      Mem<S>::st(y0, rS, (uj + (unsigned)(VSTG + N)) * ES, so), Mem<S>::st(y1, rS, (uj + (unsigned)(VSTG + N + 16)) * ES, so);
      s_x[j] = xn0, s_x[16 + j] = xn1;
    }
    lds_order();
  }
  } // !FACTOR: the factor sweep has no rollout
#ifdef SIP_MT16_STAMPS
  if (stamps != nullptr && L.lane == 0) {
    unsigned long long *o = stamps + (long)blockIdx.x * 20;
    o[0] = start_, o[1] = back_end_, o[2] = __builtin_amdgcn_s_memtime();
    for (int k = 0; k < 16; ++k)
      o[3 + k] = seg_[k];
  }
#endif
