// chain_mt16.hpp -- batched chain Riccati kernel for n = 32 on 16 x 16 matrix-core tiles
// (BASELINE config 4: batch 4096, T = 100, n = 32, m = 8, fp32; the same code in fp64).
//
// One problem per wavefront.  A 32 x 32 matrix is 2 x 2 tiles in the C/D layout of
// v_mfma_{f32,f64}_16x16x4: lane (j = lane & 15, g = lane >> 4), register v of tile (I, J) holds
// element (16 I + row(g, v), 16 J + j), row(g, v) = 4 g + v in fp32 and g + 4 v in fp64.  In that layout
//
//      sum_v mfma(U[v], V[v]) = U^T V            (one 16 x 16 tile, contraction over the tile's rows)
//
// takes both operands as they stand (register v of lane (j, g) is A[i = j][k = g] of one operand and
// B[k = g][j] of the other), so no operand of the recursion ever goes through LDS:
//      F = W A = W^T A                         lqr.cpp:703          32 MFMAs
//      Z = W B                                 (H_child^T, :692)     16
//      G = R + B^T Z                           lqr.cpp:693-694        8
//      H = M^T + B^T F                         lqr.cpp:704-705       16
//      K = -G^-1 H                             lqr.cpp:707-713        4
//      V = Q + A^T F + K^T H                   lqr.cpp:715-719       32 + 8
// Against the 32x32x2 formulation of chain_mf32.hpp the m-row blocks (Z, G, H, K: 8 of 32 rows or
// columns) cost a 16-wide tile instead of a 32-wide one.  Controls sit at the tile rows / columns
// row(a & 3, a >> 2): registers 0 and 1 of every lane group at m <= 8, so a contraction over the control index
// (K = Gn^T H, K^T H) issues two MFMAs per tile, not four.  The tile has room for 16 controls: m = 12 and m = 16
// (chain_mt16_wide.hip, the rows of sip_lqr_plan_set_wide_controls) fill registers 0 .. 2 and 0 .. 3 -- VM =
// ceil(m / 4) MFMAs per contraction, a G sweep of VM steps; every other product is a whole tile at any m.
//
// The factorisations are symmetric SWEEPS on the matrix pipe, four pivots per step: with K the pivot
// set, C = A[:, K], P = A[K, K],
//      A[i][j] <- A[i][j] - C_i P^-1 C_j^T  (i, j not in K),  A[:, K] <- C P^-1,  A[K, K] <- -P^-1,
// and after all pivots A holds -A^-1 (the sweep operator).  The pivots met on the way are the Schur
// complements a Cholesky meets (d_k = L_kk^2 of Eigen::LLT, lqr.cpp:505 / :697, in this pivot order),
// so "pivot <= 0" <=> the reference's failure status.  One sweep replaces Cholesky + triangular
// inverse + X^T X of chain_mf32.hpp (48 MFMAs of 32x32x2 -> the equivalent of 24), and W follows as
// W = D^-1/2 (I - F^-1) D^-1/2 (lqr.cpp:521-528) elementwise.  The pivot set of a step is register v of
// the four lane groups (rows row(0..3, v) of tile row I): then C^T is register v of tile row I AS IT
// STANDS for both operands of the update
//      A += (-C + [I on the pivot rows]) * (P^-1 (C^T - [I on the pivot columns])),
// whose modified operands also write the pivot rows and columns (C P^-1) and leave 2 I - P^-1 on the
// pivot block (corrected by a subtraction on four lanes).  P^-1 (4 x 4, from an LDL^T in registers,
// uniform over the wave) enters through one more MFMA per tile column ("mix").
//
// Vectors (g, h, k, v of the affine sweep; x, u, y of the rollout) are small LDS arrays and
// broadcast-FMA sums over the lane groups.
#pragma once
#include <hip/hip_runtime.h>

#include "mt16_launch.hpp"

// Diagnostic build (tools/dev/mt16_stamps.hip): cycles per segment of the backward loop, per wavefront.
#ifdef SIP_MT16_STAMPS
#define SIP_MT16_STAMP_ARG , unsigned long long *__restrict__ stamps
#define SIP_MT16_STAMP(k)                                                                                     \
  do {                                                                                                       \
    const unsigned long long now_ = __builtin_amdgcn_s_memtime();                                            \
    seg_[k] += now_ - last_;                                                                                 \
    last_ = now_;                                                                                            \
  } while (0)
#else
#define SIP_MT16_STAMP_ARG
#define SIP_MT16_STAMP(k)
#endif

namespace sipamd {
namespace mt16 {

constexpr int N = 32;

template <typename S> struct Tr;
template <> struct Tr<float> {
  typedef float v4 __attribute__((ext_vector_type(4)));
  static constexpr bool ROWS_CONTIGUOUS = true; // registers 0..3 of a lane are consecutive rows
  static constexpr int RSTEP = 1;                // row(g, v) = row(g, 0) + RSTEP * v
  static __device__ __forceinline__ constexpr int row(const int g, const int v) { return 4 * g + v; }
  static __device__ __forceinline__ v4 mfma(const float a, const float b, const v4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ float rcp(const float x) {
    return __builtin_amdgcn_rcpf(x); // 1 ulp; the pivots' reciprocals enter P^-1 = M^T D^-1 M linearly
  }
  static __device__ __forceinline__ float uniform(const float x, const int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), lane));
  }
  static __device__ __forceinline__ float sqrt(const float x) { return sqrtf(x); }
  static __device__ __forceinline__ float rsqrt(const float x) { return __builtin_amdgcn_rsqf(x); }
  static __device__ __forceinline__ float fma(const float a, const float b, const float c) { return __builtin_fmaf(a, b, c); }
};
template <> struct Tr<double> {
  typedef double v4 __attribute__((ext_vector_type(4)));
  static constexpr bool ROWS_CONTIGUOUS = false;
  static constexpr int RSTEP = 4;
  static __device__ __forceinline__ constexpr int row(const int g, const int v) { return g + 4 * v; }
  static __device__ __forceinline__ v4 mfma(const double a, const double b, const v4 c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ double rcp(const double x) { return 1.0 / x; }
  static __device__ __forceinline__ double uniform(const double x, const int lane) {
    const long long bits = __double_as_longlong(x);
    const int lo = __builtin_amdgcn_readlane((int)(bits & 0xffffffffll), lane);
    const int hi = __builtin_amdgcn_readlane((int)(bits >> 32), lane);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
  }
  static __device__ __forceinline__ double sqrt(const double x) { return ::sqrt(x); }
  static __device__ __forceinline__ double rsqrt(const double x) { return 1.0 / ::sqrt(x); }
  static __device__ __forceinline__ double fma(const double a, const double b, const double c) { return __builtin_fma(a, b, c); }
};

// typed fused multiply-add (__builtin_fma on floats would go through double)
__device__ __forceinline__ float fma_(const float a, const float b, const float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_(const double a, const double b, const double c) { return __builtin_fma(a, b, c); }

// The workgroup is ONE wavefront: the LDS instructions of a wavefront execute in order, so a write by some lanes
// is visible to a later read by others without a barrier.  __syncthreads() would also drain vmcnt -- every
// outstanding load, spill store and gains store -- six times per stage; this only keeps the compiler from moving
// memory operations across the point (no instruction is emitted).
__device__ __forceinline__ void lds_order() { __builtin_amdgcn_wave_barrier(); }

// Global memory through buffer instructions: SGPR descriptor (one per array, based at the wavefront's problem), one
// 32-bit VGPR byte offset per lane pattern, an SGPR offset for the stage and a 12-bit immediate -- no 64-bit pointer
// pair per access in the VGPRs.  Offsets in BYTES.
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2b __attribute__((ext_vector_type(2)));
typedef __amdgpu_buffer_rsrc_t rsrc_t;
__device__ __forceinline__ rsrc_t make_rsrc(const void *base, const long bytes) {
  return __builtin_amdgcn_make_buffer_rsrc((void *)base, 0, (int)bytes, 0x00020000);
}
template <typename S> struct Mem;
template <> struct Mem<float> {
  typedef Tr<float>::v4 v4;
  static __device__ __forceinline__ float ld(const rsrc_t r, const unsigned vo, const unsigned so) {
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, vo, so, 0));
  }
  static __device__ __forceinline__ v4 ld4(const rsrc_t r, const unsigned vo, const unsigned so) {
    return __builtin_bit_cast(v4, __builtin_amdgcn_raw_buffer_load_b128(r, vo, so, 0));
  }
  static __device__ __forceinline__ void st(const float x, const rsrc_t r, const unsigned vo, const unsigned so) {
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(x), r, vo, so, 0);
  }
  static __device__ __forceinline__ void st4(const v4 x, const rsrc_t r, const unsigned vo, const unsigned so) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, x), r, vo, so, 0);
  }
};
template <> struct Mem<double> {
  typedef Tr<double>::v4 v4;
  typedef double d2 __attribute__((ext_vector_type(2)));
  static __device__ __forceinline__ double ld(const rsrc_t r, const unsigned vo, const unsigned so) {
    return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, vo, so, 0));
  }
  static __device__ __forceinline__ v4 ld4(const rsrc_t r, const unsigned vo, const unsigned so) {
    const d2 a = __builtin_bit_cast(d2, __builtin_amdgcn_raw_buffer_load_b128(r, vo, so, 0));
    const d2 b = __builtin_bit_cast(d2, __builtin_amdgcn_raw_buffer_load_b128(r, vo + 16u, so, 0));
    return v4{a[0], a[1], b[0], b[1]};
  }
  static __device__ __forceinline__ void st(const double x, const rsrc_t r, const unsigned vo, const unsigned so) {
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2b, x), r, vo, so, 0);
  }
  static __device__ __forceinline__ void st4(const v4 x, const rsrc_t r, const unsigned vo, const unsigned so) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, d2{x[0], x[1]}), r, vo, so, 0);
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, d2{x[2], x[3]}), r, vo + 16u, so, 0);
  }
};

template <typename S> struct Mat32 { // 32 x 32: t[I][J]
  typename Tr<S>::v4 t[2][2];
};
template <typename S> struct Pair { // 32 x 16 (t[I]: B, Z) or 16 x 32 (t[J]: H, K, M^T)
  typename Tr<S>::v4 t[2];
};

template <typename S> __device__ __forceinline__ typename Tr<S>::v4 zero4() {
  return typename Tr<S>::v4{S(0), S(0), S(0), S(0)};
}

// acc += U^T V (32 x 32 each); four independent accumulators take turns (the 16x16x4 MFMA has a
// 40-cycle dependent latency against a 32-cycle issue interval)
template <typename S>
__device__ __forceinline__ void mul_tt(const Mat32<S> &U, const Mat32<S> &V, Mat32<S> &acc) {
#pragma unroll
  for (int R = 0; R < 2; ++R)
#pragma unroll
    for (int v = 0; v < 4; ++v)
#pragma unroll
      for (int I = 0; I < 2; ++I)
#pragma unroll
        for (int J = 0; J < 2; ++J)
          acc.t[I][J] = Tr<S>::mfma(U.t[R][I][v], V.t[R][J][v], acc.t[I][J]);
}

// Position of the lane and the control index of a tile row / column.
// Lane selectors of the sweep.  fp64: one-hot vectors in registers (the selection is a handful of FMAs).  fp32,
// where the register budget decides the occupancy: lane MASKS in SGPR pairs, applied by v_cndmask.
typedef unsigned long long lanemask_t;
template <typename S> struct LaneT {
  int lane, j, g;
  S eg[4]; // one-hot of the lane group:      eg[k] = (g == k)
  S ej[4]; // one-hot of the tile rows row(kk, 0): ej[kk] = (j == row(kk, 0))
};
template <> struct LaneT<float> {
  int lane, j, g;
  lanemask_t mg[4], mj[4]; // lanes with g == k / with j == row(kk, 0)
};
// mask[lane] ? a : b.  The masks are laundered through an empty asm when they are built (so that the compiler cannot
// fold them back into comparisons of the lane group, which it then lowers to exec-masked branches -- a switch -- when
// selects on the same value nest); the selects themselves are the compiler's own v_cndmask with an SGPR-pair mask,
// so every hazard around them (transcendental results, MFMA operands) is its business, not an inline asm's.
__device__ __forceinline__ float sel(const lanemask_t m, const float a, const float b) {
  return __builtin_amdgcn_inverse_ballot_w64(m) ? a : b;
}
__device__ __forceinline__ lanemask_t opaque_mask(const bool lane_predicate) {
  lanemask_t m = __builtin_amdgcn_ballot_w64(lane_predicate);
  asm volatile("" : "+s"(m));
  return m;
}

// control index of tile row row(g, v): a = g + 4 v
__device__ __forceinline__ constexpr int ctrl_of(const int g, const int v) { return g + 4 * v; }
// control index of tile COLUMN j (the (g', v') with row(g', v') == j)
template <typename S> __device__ __forceinline__ int ctrl_of_col(const int j) {
  return Tr<S>::ROWS_CONTIGUOUS ? (j >> 2) + 4 * (j & 3) : j;
}

// sum over the four lane groups (lanes j, j + 16, j + 32, j + 48): every lane gets the total.  On the vector
// pipe: v_permlane32_swap / v_permlane16_swap (gfx950) exchange the halves / the odd and even 16-lane rows of two
// registers, so x + swap(x) is the sum with the partner row -- no LDS round trip (ds_bpermute) in the dependent
// chains of the vector work.
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float sum_groups(const float x) {
  const unsigned b = __float_as_uint(x);
  const u32x2 h = __builtin_amdgcn_permlane32_swap(b, b, false, false); // {[lo, lo], [hi, hi]}
  const float s = __uint_as_float(h[0]) + __uint_as_float(h[1]);
  const unsigned c = __float_as_uint(s);
  const u32x2 q = __builtin_amdgcn_permlane16_swap(c, c, false, false); // rows {[0, 0, 2, 2], [1, 1, 3, 3]}
  return __uint_as_float(q[0]) + __uint_as_float(q[1]);
}
__device__ __forceinline__ double swap_sum(const double x, const bool rows16) {
  const unsigned long long bits = (unsigned long long)__double_as_longlong(x);
  const unsigned lo = (unsigned)bits, hi = (unsigned)(bits >> 32);
  const u32x2 a = rows16 ? __builtin_amdgcn_permlane16_swap(lo, lo, false, false)
                         : __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
  const u32x2 b = rows16 ? __builtin_amdgcn_permlane16_swap(hi, hi, false, false)
                         : __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
  const double u = __longlong_as_double((long long)(((unsigned long long)b[0] << 32) | a[0]));
  const double w = __longlong_as_double((long long)(((unsigned long long)b[1] << 32) | a[1]));
  return u + w;
}
__device__ __forceinline__ double sum_groups(const double x) { return swap_sum(swap_sum(x, false), true); }

// vec[16 I + row(g, v)], v = 0..3 (LDS array indexed by row)
template <typename S>
__device__ __forceinline__ typename Tr<S>::v4 by_row(const S *vec, const int I, const int g) {
  typename Tr<S>::v4 r;
#pragma unroll
  for (int v = 0; v < 4; ++v)
    r[v] = vec[16 * I + Tr<S>::row(g, v)];
  return r;
}

// y = Mt^T vec: returns the partial sums of this lane group for columns j and 16 + j (sum_groups
// completes them); vec given by row.
template <typename S>
__device__ __forceinline__ void mat_t_vec(const Mat32<S> &Mt, const typename Tr<S>::v4 (&xr)[2], S &p0, S &p1) {
#pragma unroll
  for (int I = 0; I < 2; ++I)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      p0 = fma_(Mt.t[I][0][v], xr[I][v], p0);
      p1 = fma_(Mt.t[I][1][v], xr[I][v], p1);
    }
}

// ---- the sweep -------------------------------------------------------------------------------
// T: TILES x TILES symmetric matrix in tiles; sweeps the pivots of registers 0 .. VP-1 of every tile
// row (all of them for VP = 4).  Returns true iff a pivot was <= 0.  On return the swept rows and
// columns hold -A^-1 restricted to them (all of -A^-1 for VP = 4).
template <typename S, int TILES, int VP>
__device__ __forceinline__ bool sweep(typename Tr<S>::v4 (&T)[TILES][TILES], const LaneT<S> &L, S *sp) {
  using TR = Tr<S>;
  using v4 = typename TR::v4;
  bool fail = false;
#pragma unroll
  for (int I = 0; I < TILES; ++I) {
#pragma unroll
    for (int v = 0; v < VP; ++v) {
      // P[a][b] = A[p_a][p_b], p_g = 16 I + row(g, v): register v of lane (j = row(b, v), g = a).  Through
      // LDS rather than v_readlane: the 16 lanes that hold P write it compactly, every lane reads it back as
      // four broadcast 16-byte reads -- no vector-pipe time (a v_readlane costs 7 to 26 cycles of it, and the
      // f32 matrix instructions share that pipe), no SGPR operands in the arithmetic below.
      S P[4][4];
      {
        const int b_of_j = TR::ROWS_CONTIGUOUS ? (L.j >> 2) : (L.j & 3); // j = row(b, v') for this b
        const int v_of_j = TR::ROWS_CONTIGUOUS ? (L.j & 3) : (L.j >> 2); //   and this v'
        if (v_of_j == v)
          sp[4 * L.g + b_of_j] = T[I][I][v];
        lds_order();
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = 0; b <= a; ++b)
            P[a][b] = sp[4 * a + b];
        lds_order();
      }
      // LDL^T of P: the pivots d_k are those of an unblocked Cholesky (squared)
      const S d0 = P[0][0], i0 = TR::rcp(d0);
      const S l10 = P[1][0] * i0, l20 = P[2][0] * i0, l30 = P[3][0] * i0;
      const S d1 = fma_(-l10, P[1][0], P[1][1]), i1 = TR::rcp(d1);
      const S t21 = fma_(-l20, P[1][0], P[2][1]), t31 = fma_(-l30, P[1][0], P[3][1]);
      const S l21 = t21 * i1, l31 = t31 * i1;
      const S d2 = fma_(-l21, t21, fma_(-l20, P[2][0], P[2][2])), i2 = TR::rcp(d2);
      const S t32 = fma_(-l31, t21, fma_(-l30, P[2][0], P[3][2]));
      const S l32 = t32 * i2;
      const S d3 = fma_(-l32, t32, fma_(-l31, t31, fma_(-l30, P[3][0], P[3][3])));
      const S i3 = TR::rcp(d3);
      fail |= !(d0 > S(0)) | !(d1 > S(0)) | !(d2 > S(0)) | !(d3 > S(0));
      // With M = L^-1 (unit lower) and X = C^T - [I on the pivot columns] (register v of tile row I as it stands,
      // minus one on the diagonal lanes) the whole step is  A <- A - Y^T D^-1 Y,  Y = M X :
      //   mix    Y_J = M X_J : the A operand carries M[kk][kq] on lane (i = row(kk, 0), kq = g), so that the result
      //          lands in register 0 of lane group kk -- which is both the B operand layout of Y and the A operand
      //          layout of Y^T;
      //   update A[It][Jt] += (-Y_It)^T-as-A-operand * (d_g^-1 Y_Jt)-as-B-operand.
      // Column g of M for this lane group, by the one-hot of the group (no selects, no P^-1):
      const S m10 = -l10, m21 = -l21, m32 = -l32;
      const S m20 = fma_(l21, l10, -l20);
      const S m31 = fma_(l32, l21, -l31);
      const S m30 = fma_(-l32, m20, fma_(l31, l10, -l30));
      S amix, ig;
      if constexpr (sizeof(S) == 4) { // column g of M = (M e_g): selected by the lane-group masks
        const S e1 = sel(L.mg[1], S(1), S(0)), e2 = sel(L.mg[2], S(1), S(0)), e3 = sel(L.mg[3], S(1), S(0));
        const S t1 = sel(L.mg[0], m10, e1);
        const S t2 = sel(L.mg[0], m20, sel(L.mg[1], m21, e2));
        const S t3 = sel(L.mg[0], m30, sel(L.mg[1], m31, sel(L.mg[2], m32, e3)));
        amix = sel(L.mj[0], sel(L.mg[0], S(1), S(0)), sel(L.mj[1], t1, sel(L.mj[2], t2, sel(L.mj[3], t3, S(0)))));
        ig = sel(L.mg[0], i0, sel(L.mg[1], i1, sel(L.mg[2], i2, i3))); // 1 / d_g
      } else {
        const S t1 = fma_(m10, L.eg[0], L.eg[1]);
        const S t2 = fma_(m20, L.eg[0], fma_(m21, L.eg[1], L.eg[2]));
        const S t3 = fma_(m30, L.eg[0], fma_(m31, L.eg[1], fma_(m32, L.eg[2], L.eg[3])));
        amix = fma_(L.ej[0], L.eg[0], fma_(L.ej[1], t1, fma_(L.ej[2], t2, L.ej[3] * t3)));
        ig = fma_(i0, L.eg[0], fma_(i1, L.eg[1], fma_(i2, L.eg[2], i3 * L.eg[3]))); // 1 / d_g
      }
      const bool diag = L.j == TR::row(L.g, v); // this lane's register v of tile (I, I) is a diagonal element
      const S one_d = diag ? S(1) : S(0);
      S bop[TILES], aop[TILES];
#pragma unroll
      for (int Jt = 0; Jt < TILES; ++Jt) {
        const S src = T[I][Jt][v] - (Jt == I ? one_d : S(0));
        const v4 mixed = TR::mfma(amix, src, zero4<S>());
        aop[Jt] = -mixed[0];
        bop[Jt] = mixed[0] * ig;
      }
#pragma unroll
      for (int It = 0; It < TILES; ++It)
#pragma unroll
        for (int Jt = 0; Jt < TILES; ++Jt)
          T[It][Jt] = TR::mfma(aop[It], bop[Jt], T[It][Jt]);
      T[I][I][v] -= S(2) * one_d;
    }
  }
  return fail;
}

template <typename S, int M> struct Layout {
  static constexpr int NODE = N * N + N;                 // Q | delta
  static constexpr int EDGE = N * N + 2 * N * M + M * M; // A | B | M | R
  static constexpr int VNODE = 2 * N, VEDGE = M, GAIN = M * N + M;
  // spill per node: tiles (0, 0), (1, 0), (1, 1) of the symmetric W as they sit in the registers | g
  static constexpr int WTILES = 3, WSN = WTILES * 256 + N;
  static constexpr int VM = (M + 3) / 4; // registers of a lane that hold controls
  // 16-byte loads of four consecutive rows need every block 16-byte aligned
  static constexpr bool VEC_LOADS = Tr<S>::ROWS_CONTIGUOUS && (EDGE % 4 == 0);
};

// Column-major 32 x 32 (ld 32) at element offset `so` of the array behind `r` -> tiles.  ocol = j * 32 + row(g, 0).
template <typename S, bool VEC>
__device__ __forceinline__ Mat32<S> load32(const rsrc_t r, const unsigned ocol, const unsigned so) {
  constexpr unsigned ES = sizeof(S);
  Mat32<S> m;
#pragma unroll
  for (int I = 0; I < 2; ++I)
#pragma unroll
    for (int J = 0; J < 2; ++J) {
      if constexpr (VEC) {
        m.t[I][J] = Mem<S>::ld4(r, (ocol + (unsigned)(16 * J * N + 16 * I)) * ES, so * ES);
      } else {
#pragma unroll
        for (int v = 0; v < 4; ++v)
          m.t[I][J][v] = Mem<S>::ld(r, (ocol + (unsigned)(16 * J * N + 16 * I + Tr<S>::RSTEP * v)) * ES, so * ES);
      }
    }
  return m;
}

// Waves per SIMD the register allocator is held to.  fp32: 4 (128 VGPRs) -- BASELINE's batch of 4096 is exactly four
// wavefronts per SIMD, and with three resident the fourth runs alone behind them at a lone wavefront's latency.  What
// made 128 registers enough (the first version spilled ~30 loop-invariant lane constants there and was slower than
// three wavefronts): every global access through a buffer descriptor in SGPRs + one 32-bit lane offset + an SGPR
// stage offset + an immediate (no 64-bit pointer pair per access pattern), and the sweep's lane selectors as SGPR
// masks instead of one-hot vectors.  bench.py --workload c4: 2.43 ms at 3 wavefronts with pointer addressing, 2.37
// with buffer addressing, 2.22 at 4 (7 dwords of scratch left).
#ifndef SIP_MT16_WAVES_F32
#define SIP_MT16_WAVES_F32 4
#endif
// The wide rows (M > 8) scale F in the fused fp32 sweep too and have no tuned allocation to protect: they are held to
// three wavefronts per SIMD in fp32 (168 VGPRs: no scratch at m = 16, 2 dwords at m = 12; the factor sweep fits in 147)
// and to two in fp64, like the others.
template <typename S, int M> struct Waves {
  static constexpr int value = sizeof(S) == 8 ? 2 : M > 8 ? 3 : SIP_MT16_WAVES_F32;
};

// The fused factor + solve sweep and the factor sweep alone share their text (chain_mt16_sweep_body.hpp).
template <typename S, int M>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(Waves<S, M>::value, Waves<S, M>::value)))
void chain_factor_solve_mt16(
    const S *__restrict__ mats, const S *__restrict__ vecs, S *__restrict__ sol, S *__restrict__ gains,
    S *__restrict__ wsp, int *__restrict__ status, const long batch, const int T SIP_MT16_STAMP_ARG) {
  constexpr bool FACTOR = false;
  S *const gfac = nullptr;
#define SIP_MT16_SWEEP_BODY
#include "chain_mt16_sweep_body.hpp"
#undef SIP_MT16_SWEEP_BODY
}

// The factor sweep of sip_lqr_plan_set_separate_sweeps: W, K, -G^-1 and the statuses.
template <typename S, int M>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(Waves<S, M>::value, Waves<S, M>::value)))
void chain_factor_mt16(const S *__restrict__ mats, S *__restrict__ gains, S *__restrict__ wsp, S *__restrict__ gfac,
                       int *__restrict__ status, const long batch, const int T SIP_MT16_STAMP_ARG) {
  constexpr bool FACTOR = true;
  const S *const vecs = nullptr;
  S *const sol = nullptr;
#define SIP_MT16_SWEEP_BODY
#include "chain_mt16_sweep_body.hpp"
#undef SIP_MT16_SWEEP_BODY
}

} // namespace mt16

// The launchers of mt16_launch.hpp for the two kernels above; the units that instantiate them: chain_mt16.hip and
// chain_mt16_solve.hip (m = 4, 8), chain_mt16_wide.hip and chain_mt16_wide_solve.hip (m = 12, 16).
#ifndef SIP_MT16_STAMPS
template <typename S, int M>
hipError_t launch_mt16(long batch, int T, const void *mats, const void *vecs, void *sol, void *gains,
                       int32_t *status, void *ws, hipStream_t stream, int /*mode: always the full sweep*/,
                       void * /*gfac*/) {
  // 16-byte loads of the stage blocks (fp32, even m) and of the W dump: bases must be 16-byte aligned
  if (((uintptr_t)mats | (uintptr_t)ws) & 15)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL((mt16::chain_factor_solve_mt16<S, M>), dim3((unsigned)batch), dim3(64), 0, stream,
                     (const S *)mats, (const S *)vecs, (S *)sol, (S *)gains, (S *)ws, (int *)status, batch, T);
  return hipGetLastError();
}

template <typename S, int M>
hipError_t launch_mt16_factor(long batch, int T, const void *mats, void *gains, int32_t *status, void *ws, void *gfac,
                              hipStream_t stream) {
  if (((uintptr_t)mats | (uintptr_t)ws) & 15)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL((mt16::chain_factor_mt16<S, M>), dim3((unsigned)batch), dim3(64), 0, stream, (const S *)mats,
                     (S *)gains, (S *)ws, (S *)gfac, (int *)status, batch, T);
  return hipGetLastError();
}
#endif

} // namespace sipamd
