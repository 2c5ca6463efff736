// chain_vjp.hpp -- the gradient of a scalar loss L(z) with respect to `mats`, through the chain KKT system
// K z + b = 0 (z = (x, u, y), b = (q, r, c), K symmetric: the formulas at sip_lqr_residual, include/sip_lqr_amd.h).
// With g = dL/dz the adjoint lambda solves K lambda + g = 0 (the plan's own solve with g as the right-hand side), and
// dL/db = lambda.  dL/dK = lambda z^T, so the gradient of a block of `mats` is a sum of outer products of lambda and
// z, block by block; z = (x_i, y_i, u_i) and lambda = (lx_i, ly_i, lu_i) both in the vecs / sol layout:
//
//   Q_i, FULL layout       1/2 (lx_i x_i^T + x_i lx_i^T), the whole square
//   Q_i, SYMMETRIC layout  packed entry (r, c):  lx_r x_c + lx_c x_r  for r > c,  lx_r x_r  for r = c
//   R_i                    the same two rules with lu_i, u_i
//   delta_i                -ly_i o y_i
//   A_i                    ly_{i+1} x_i^T + y_{i+1} lx_i^T
//   B_i                    ly_{i+1} u_i^T + y_{i+1} lu_i^T
//   M_i                    lx_i u_i^T + x_i lu_i^T
//
// Q and R are taken symmetric everywhere in this library.  The FULL rule is the gradient over symmetric
// perturbations: dL = <G, dQ> for symmetric dQ.  The SYMMETRIC rule is the derivative with respect to the packed
// parameter.  The two agree: <G_full, dQ> = sum over the packed entries of g_rc dQ_rc.
//
// Every entry has one form: s (lambda[ia] z[ib] + z[ia] lambda[ib]) with ia, ib two places in the 4 n + m entries
// x_i | y_i | u_i | x_{i+1} | y_{i+1} that stage i of sol spans, and s one of 1, 1/2, -1/2 (delta: ia = ib, s = -1/2;
// a diagonal entry of a packed triangle: ia = ib, s = 1/2).  (ia, ib, s) of an entry of the stage image
// [Q | delta | A | B | M | R] does not depend on the stage: the workgroup decodes the image once into a table in LDS
// (the divisions by n and m happen there), and the stage loop reads it.  A table that does not fit the LDS budget is
// replaced by decoding in place (TABLE = false).
//
// Shape: blockIdx.x is the problem, blockIdx.y a run of stages.  The workgroup first widens z and lambda of its whole
// run -- one contiguous piece of sol and of adj -- into LDS as pairs (z[k], lambda[k]), kGather loads per lane in
// flight, so the latency of memory is paid once per workgroup and not once per stage; nothing after that reads
// memory, and no store is ever waited for.  Then its wavefronts take the stages of the run in turn: an entry of the
// gradient takes two 16-byte LDS reads, and the image is stored in 16-byte pieces, consecutive lanes consecutive
// pieces.  The pieces are those of the address, not of the stage: a stage that starts off a 16-byte boundary
// (mats_len or the stage length odd) begins and ends with a partial piece, stored scalar by scalar, so every scalar
// of the output is written exactly once and nothing else is.
// Arithmetic: fma(lambda[ia], z[ib], z[ia] * lambda[ib]) in fp64 -- two roundings -- times s (exact), then one
// rounding to the output scalar.  A problem whose status is not SIP_LQR_SUCCESS gets zeros by a branch: its sol and
// adj are not read.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "chain_residual.hpp" // residual::Dims / make_dims: the offsets of the layout are stated there, once

namespace sipamd {
namespace vjp {

using residual::Dims;

constexpr int kLanes = 64;
constexpr int kMaxWaves = 8; // wavefronts of a workgroup, at the most
constexpr int kGather = 4;   // entries of sol and of adj a lane has in flight

// One entry of the stage image: s (lambda[ia] z[ib] + z[ia] lambda[ib]); sc: 0 -> 1, 1 -> 1/2, 2 -> -1/2.
struct Entry {
  int ia, ib, sc;
};

// (row, column) of entry t of a dim x dim symmetric block: the full column-major square, or (sym) the lower triangle
// packed by columns.
__host__ __device__ inline void square_entry(int t, const int dim, const int sym, int &r, int &c) {
  if (!sym) {
    c = t / dim, r = t - c * dim;
    return;
  }
  c = 0;
  while (t >= dim - c) // column c holds rows c .. dim - 1
    t -= dim - c, ++c;
  r = c + t;
}

// z of a stage: [0, n) x_i | [n, 2n) y_i | [2n, 2n + m) u_i | [2n + m, 3n + m) x_{i+1} | [3n + m, 4n + m) y_{i+1}
__host__ __device__ inline Entry decode(const Dims &d, const int e) {
  const int n = d.n, m = d.m;
  int r, c;
  if (e < d.oD) {
    square_entry(e, n, d.sym, r, c);
    return {r, c, d.sym && r != c ? 0 : 1};
  }
  if (e < d.oA)
    return {n + (e - d.oD), n + (e - d.oD), 2};
  if (e < d.oB) {
    c = (e - d.oA) / n, r = (e - d.oA) - c * n;
    return {3 * n + m + r, c, 0};
  }
  if (e < d.oM) {
    c = (e - d.oB) / n, r = (e - d.oB) - c * n;
    return {3 * n + m + r, 2 * n + c, 0};
  }
  if (e < d.oR) {
    c = (e - d.oM) / n, r = (e - d.oM) - c * n;
    return {r, 2 * n + c, 0};
  }
  square_entry(e - d.oR, m, d.sym, r, c);
  return {2 * n + r, 2 * n + c, d.sym && r != c ? 0 : 1};
}

// The table's word: ia and ib in 14 bits each (a table that fits the LDS budget has 4 n + m far below 2^14).
__host__ __device__ inline uint32_t pack(const Entry t) {
  return (uint32_t)t.ia | ((uint32_t)t.ib << 14) | ((uint32_t)t.sc << 28);
}
__host__ __device__ inline int table_bytes(const Dims &d) { return (d.stg * 4 + 15) & ~15; }
// Pairs of a run of `run` stages: the stages' slots and x | y of the stage after the last (a run that ends the problem
// has none and uses less).
__host__ __device__ inline size_t operand_bytes(const Dims &d, const int run) {
  return ((size_t)run * d.vstg + 2 * d.n) * 16;
}

// dst[e] = value(e) for e in [0, len), e = first, first + step, ... in units of 16-byte pieces of the ADDRESS: a piece
// that lies inside [dst, dst + len) is one 16-byte store, what is left at either end goes scalar by scalar.
template <typename S, typename F>
__device__ __forceinline__ void emit(S *__restrict__ dst, const int len, const int first, const int step, F value) {
  constexpr int PIECE = 16 / (int)sizeof(S);
  typedef S Vec __attribute__((ext_vector_type(PIECE)));
  const int off = (int)(((uintptr_t)dst / sizeof(S)) & (PIECE - 1)); // scalars from the 16-byte boundary up to dst
  const int pieces = (off + len + PIECE - 1) / PIECE;
  for (int k = first; k < pieces; k += step) {
    const int e0 = k * PIECE - off;
    if (e0 >= 0 && e0 + PIECE <= len) {
      Vec v;
#pragma unroll
      for (int j = 0; j < PIECE; ++j)
        v[j] = value(e0 + j);
      *(Vec *)(dst + e0) = v;
    } else {
#pragma unroll
      for (int j = 0; j < PIECE; ++j)
        if (e0 + j >= 0 && e0 + j < len)
          dst[e0 + j] = value(e0 + j);
    }
  }
}

// S: scalar of sol, adj and grad.  Dynamic LDS: the table (TABLE), then operand_bytes(d, run).
template <typename S, bool TABLE>
__global__ void __launch_bounds__(kLanes * kMaxWaves)
    chain_vjp_kernel(const Dims d, const S *__restrict__ sol, const S *__restrict__ adj,
                     const int32_t *__restrict__ status, S *__restrict__ grad, const int run) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int n = d.n, T = d.T;
  const long p = blockIdx.x;
  const int lane = threadIdx.x & (kLanes - 1), wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kLanes);
  const int waves = blockDim.x / kLanes;
  const int i0 = blockIdx.y * run, i1 = i0 + run < T + 1 ? i0 + run : T + 1; // the stages of this workgroup
  S *pg = grad + p * d.mats_len;

  if (status != nullptr && status[p] != 0) { // a branch, the same in every lane: sol and adj may hold anything
    for (int i = i0 + wave; i < i1; i += waves)
      emit(pg + (long)i * d.stg, i < T ? d.stg : d.node, lane, kLanes, [](int) { return (S)0; });
    return;
  }

  const uint32_t *table = (const uint32_t *)lds;
  double2 *pairs = (double2 *)(lds + (TABLE ? table_bytes(d) : 0));
  // z and lambda of stages i0 .. i1 - 1: slots x | y | u of each, and x | y of stage i1 (the last stage has x | y only)
  const long first = (long)i0 * d.vstg;
  const int count = (int)((long)(i1 < T ? i1 : T) * d.vstg + 2 * n - first);
  const S *ps = sol + p * d.vecs_len + first, *pa = adj + p * d.vecs_len + first;
  // A thread past the end loads and stores the last entry again: in bounds, the same value to the same place, and no
  // branch between the loads and the stores, which would leave one load in flight at a time.
  for (int base = 0; base < count; base += (int)blockDim.x * kGather) {
    S rz[kGather], ra[kGather];
    int k[kGather];
#pragma unroll
    for (int j = 0; j < kGather; ++j) {
      const int at = base + j * (int)blockDim.x + (int)threadIdx.x;
      k[j] = at < count ? at : count - 1;
      rz[j] = ps[k[j]], ra[j] = pa[k[j]];
    }
#pragma unroll
    for (int j = 0; j < kGather; ++j)
      pairs[k[j]] = make_double2((double)rz[j], (double)ra[j]);
  }
  if constexpr (TABLE)
    for (int e = threadIdx.x; e < d.stg; e += blockDim.x)
      ((uint32_t *)lds)[e] = pack(decode(d, e));
  __syncthreads();

  for (int i = i0 + wave; i < i1; i += waves) {
    const bool edge = i < T;
    const double2 *zl = pairs + (i - i0) * d.vstg;
    emit(pg + (long)i * d.stg, edge ? d.stg : d.node, lane, kLanes, [&](const int e) {
      int ia, ib, sc;
      if constexpr (TABLE) {
        const uint32_t w = table[e];
        ia = w & 0x3fff, ib = (w >> 14) & 0x3fff, sc = w >> 28;
      } else {
        const Entry t = decode(d, e);
        ia = t.ia, ib = t.ib, sc = t.sc;
      }
      const double2 a = zl[ia], b = zl[ib]; // (z, lambda)
      const double v = __builtin_fma(a.y, b.x, a.x * b.y);
      return (S)(v * (sc == 0 ? 1.0 : (sc == 1 ? 0.5 : -0.5)));
    });
  }
}

// vec[p][0 .. len) = 0 where status[p] != SIP_LQR_SUCCESS (= 0); one workgroup per problem
template <typename S>
__global__ void __launch_bounds__(256)
    vjp_mask_kernel(const long len, const int32_t *__restrict__ status, S *__restrict__ vec) {
  const long p = blockIdx.x;
  if (status[p] == 0)
    return;
  for (long k = threadIdx.x; k < len; k += blockDim.x)
    vec[p * len + k] = (S)0;
}

} // namespace vjp
} // namespace sipamd
