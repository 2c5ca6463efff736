// chain_vjp_cols.hpp -- the gradient kernel of the chain KKT solve (chain_vjp.hpp) for several columns: NC solutions
// z_c and adjoints lambda_c against one `mats`, and ONE gradient, the sum over the columns of the single kernel's
// outer products.  The entry form s (lambda[ia] z[ib] + z[ia] lambda[ib]), decode / pack / the table in LDS, emit with
// its 16-byte pieces of the address, the status branch and the layout's offsets are those of chain_vjp.hpp, used from
// there and not restated.
//
// Shape: blockIdx.x is the problem, blockIdx.y a run of stages, as there.  The workgroup gathers (z_c[k], lambda_c[k])
// of its run for all NC columns into LDS -- kGather loads per lane in flight over the flattened (column, entry) index,
// no branch between loads and stores -- and synchronises once.  Then a lane reads the table word of an entry once and
// walks the columns in ascending order, in fp64:
//   column 0 of the CALL   v = fma(lambda[ia], z[ib], z[ia] * lambda[ib])           (the single kernel's expression)
//   every further column   v = fma(lambda[ia], z[ib], fma(z[ia], lambda[ib], v))
// then v * s (exact) is rounded once to the output scalar, so one column gives the bits of chain_vjp_kernel.
// ACC (the groups of a call after its first): v starts from the scalar already in `grad`, widened and divided by s
// (times 1, 2 or -2: exact), and every column of the group is chained onto it.  With double output the result
// therefore does not depend on how the columns were grouped (barring underflow in the halving); with float output a
// group boundary costs one rounding to float.  The first group never reads `grad`.
//
// LDS order: pairs[c][k], a column's run contiguous, the columns `slots` pairs apart.  The lanes of a wavefront hold
// consecutive entries of a column-major block, so ia runs over consecutive k while ib (the block's column) is the
// same in most lanes.  With [c][k] the 16-byte reads at ia of the 16 lanes that share an LDS cycle fall on 16
// consecutive slots of the 256-byte bank row: no conflict, for any NC; the reads at ib broadcast.  [k][c] would put
// those lanes NC * 16 bytes apart -- at NC = 8 every second lane on the same banks, 8 addresses per bank -- and its
// one advantage, a constant offset from one address per operand, costs [c][k] one integer add per column and operand.
//
// A problem whose status is not SIP_LQR_SUCCESS gets zeros from the first group and is left alone by the later ones;
// its sol and adj are never read.  NC = 0 is the empty sum: zeros everywhere.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "chain_vjp.hpp"

namespace sipamd {
namespace vjp {

// S: scalar of sol, adj and grad.  sol / adj: column c of the group at c * col_stride scalars.  Dynamic LDS: the table
// (TABLE), then NC * operand_bytes(d, run).
template <typename S, bool TABLE, int NC, bool ACC>
__global__ void __launch_bounds__(kLanes * kMaxWaves)
    chain_vjp_cols_kernel(const Dims d, const S *__restrict__ sol, const S *__restrict__ adj, const long col_stride,
                          const int32_t *__restrict__ status, S *grad, const int run) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int n = d.n, T = d.T;
  const long p = blockIdx.x;
  const int lane = threadIdx.x & (kLanes - 1), wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kLanes);
  const int waves = blockDim.x / kLanes;
  const int i0 = blockIdx.y * run, i1 = i0 + run < T + 1 ? i0 + run : T + 1; // the stages of this workgroup
  S *pg = grad + p * d.mats_len;

  if (NC == 0 || (status != nullptr && status[p] != 0)) { // the same in every lane: sol and adj may hold anything
    if constexpr (!ACC)
      for (int i = i0 + wave; i < i1; i += waves)
        emit(pg + (long)i * d.stg, i < T ? d.stg : d.node, lane, kLanes, [](int) { return (S)0; });
    return;
  }
  if constexpr (NC > 0) {
    const uint32_t *table = (const uint32_t *)lds;
    double2 *pairs = (double2 *)(lds + (TABLE ? table_bytes(d) : 0));
    // z and lambda of stages i0 .. i1 - 1 of every column: slots x | y | u of each stage, and x | y of stage i1
    const long first = (long)i0 * d.vstg;
    const int count = (int)((long)(i1 < T ? i1 : T) * d.vstg + 2 * n - first); // entries of one column
    const int slots = run * d.vstg + 2 * n;                                     // pairs from a column to the next
    const S *ps = sol + p * d.vecs_len + first, *pa = adj + p * d.vecs_len + first;
    // A thread past the end loads and stores the last entry again: in bounds, the same value to the same place, and
    // no branch between the loads and the stores, which would leave one load in flight at a time.
    const int total = NC * count;
    for (int base = 0; base < total; base += (int)blockDim.x * kGather) {
      S rz[kGather], ra[kGather];
      int to[kGather];
#pragma unroll
      for (int j = 0; j < kGather; ++j) {
        const int at = base + j * (int)blockDim.x + (int)threadIdx.x;
        const int t = at < total ? at : total - 1;
        const int c = t / count, k = t - c * count;
        const long from = c * col_stride + k;
        to[j] = c * slots + k;
        rz[j] = ps[from], ra[j] = pa[from];
      }
#pragma unroll
      for (int j = 0; j < kGather; ++j)
        pairs[to[j]] = make_double2((double)rz[j], (double)ra[j]);
    }
    if constexpr (TABLE)
      for (int e = threadIdx.x; e < d.stg; e += blockDim.x)
        ((uint32_t *)lds)[e] = pack(decode(d, e));
    __syncthreads();

    for (int i = i0 + wave; i < i1; i += waves) {
      const bool edge = i < T;
      const double2 *zl = pairs + (i - i0) * d.vstg;
      S *dst = pg + (long)i * d.stg;
      emit(dst, edge ? d.stg : d.node, lane, kLanes, [&](const int e) {
        int ia, ib, sc;
        if constexpr (TABLE) {
          const uint32_t w = table[e];
          ia = w & 0x3fff, ib = (w >> 14) & 0x3fff, sc = w >> 28;
        } else {
          const Entry t = decode(d, e);
          ia = t.ia, ib = t.ib, sc = t.sc;
        }
        const double2 *za = zl + ia, *zb = zl + ib; // (z, lambda) of column 0; column c is c * slots further
        double v;
        if constexpr (ACC) {
          v = (double)dst[e] * (sc == 0 ? 1.0 : (sc == 1 ? 2.0 : -2.0));
        } else {
          const double2 a = za[0], b = zb[0];
          v = __builtin_fma(a.y, b.x, a.x * b.y);
        }
#pragma unroll
        for (int c = ACC ? 0 : 1; c < NC; ++c) {
          const double2 a = za[c * slots], b = zb[c * slots];
          v = __builtin_fma(a.y, b.x, __builtin_fma(a.x, b.y, v));
        }
        return (S)(v * (sc == 0 ? 1.0 : (sc == 1 ? 0.5 : -0.5)));
      });
    }
  }
}

// vec[c][p][0 .. len) = 0 where status[p] != SIP_LQR_SUCCESS (= 0); blockIdx.x the problem, blockIdx.y the column
template <typename S>
__global__ void __launch_bounds__(256) vjp_mask_cols_kernel(const long len, const long col_stride,
                                                            const int32_t *__restrict__ status, S *__restrict__ vec) {
  const long p = blockIdx.x;
  if (status[p] == 0)
    return;
  S *v = vec + (long)blockIdx.y * col_stride + p * len;
  for (long k = threadIdx.x; k < len; k += blockDim.x)
    v[k] = (S)0;
}

} // namespace vjp
} // namespace sipamd
