// tree_vjp_cols.hpp -- the gradient kernel of the tree KKT solve (tree_vjp.hpp) for several columns: NC solutions z_c
// and adjoints lambda_c against one input arena, and ONE gradient, the sum over the columns of the single kernel's
// outer products.  The table word (tree_vjp_table.hpp), emit with its 16-byte pieces of the address and kGather
// (chain_vjp.hpp) are used from there and not restated.  fp64.
//
// Shape: blockIdx.x is the problem, blockIdx.y a run of consecutive entries of the input arena, as in tree_vjp_kernel.
// STAGED: the workgroup gathers (z_c[k], lambda_c[k]) of its problem -- the whole output arena of every column -- into
// LDS, kGather loads of each operand per lane in flight over the flattened (column, entry) index, no branch between
// the loads and their LDS stores (a lane past the end repeats the last entry), and synchronises once.  The other form
// reads z_c and lambda_c in place.  Then a lane reads the table word of an entry once and walks the columns in
// ascending order:
//   column 0 of the CALL   v = fma(lambda[ia], z[ib], z[ia] * lambda[ib])           (tree_vjp_kernel's expression)
//   every further column   v = fma(lambda[ia], z[ib], fma(z[ia], lambda[ib], v))
// then v * s (1, 1/2, -1/2: exact) and one store.  The column loop is unrolled, so the 2 NC LDS reads of an entry are
// issued before the first fma; NC is the group's own count, 3 or 7 included: a zero-filled column would not be
// bit-neutral (-0 + 0 = +0).
// ACC (the groups of a call after its first): v starts from the scalar already in `grad`, with s undone exactly (times
// 1, 2 or -2), and every column of the group is chained onto it, so the result does not depend on how the columns were
// grouped (barring underflow in the halving).  The same lane reads and writes a scalar, in the same pieces.  The first
// group never reads `grad`.
//
// The kCopy entries (the q, c, r slots of the input arena) are written +0.0, by every group: sip_lqr_tree_solve_multi
// ignores the arena's q, c, r -- its right-hand sides are the columns -- so the true gradient there is zero, and
// dL/db_c is lambda_c itself, which the caller has as the adjoint columns.  One column therefore gives the bits of
// tree_vjp_kernel on every other entry and +0.0 on these.
//
// LDS order: pairs[c][k], a column's arena contiguous, the columns out_len pairs apart: the order chain_vjp_cols.hpp
// derives as free of bank conflicts for the 16-byte reads of the lanes of a column-major block ([k][c] is not).
//
// A problem whose status is not SIP_LQR_SUCCESS gets zeros from the first group, by a branch that is the same in every
// lane, and is left alone by the later ones; its columns are never read.  NC = 0 is the empty sum: zeros everywhere.
// Every scalar of the gradient is written exactly once per group, nothing else is written, and there are no atomics:
// two launches give the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "chain_vjp.hpp" // vjp::emit, vjp::kGather
#include "tree_vjp_table.hpp"

namespace sipamd {
namespace tree_vjp {

// sol / adj: column c of the group at c * col_stride doubles.  Dynamic LDS: STAGED, NC * out_len pairs.  run: entries
// per workgroup (Shape::run).
template <bool STAGED, int NC, bool ACC>
__global__ void __launch_bounds__(kLanes * kMaxWaves)
    tree_vjp_cols_kernel(const Word *__restrict__ table, const long in_len, const int out_len,
                         const double *__restrict__ sol, const double *__restrict__ adj, const long col_stride,
                         const int32_t *__restrict__ status, double *grad, const long run) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const long p = blockIdx.x;
  const long e0 = (long)blockIdx.y * run;
  if (e0 >= in_len)
    return;
  const int len = (int)(in_len - e0 < run ? in_len - e0 : run);
  double *pg = grad + p * in_len + e0;

  if (NC == 0 || (status != nullptr && status[p] != 0)) { // the same in every lane: sol and adj may hold anything
    if constexpr (!ACC)
      vjp::emit(pg, len, (int)threadIdx.x, (int)blockDim.x, [](int) { return 0.0; });
    return;
  }
  if constexpr (NC > 0) {
    const double *ps = sol + p * (long)out_len, *pa = adj + p * (long)out_len;
    double2 *pairs = (double2 *)lds;
    if constexpr (STAGED) {
      // A thread past the end loads and stores the last entry again: in bounds, the same value to the same place, and
      // no branch between the loads and the stores, which would leave one load in flight at a time.
      const int total = NC * out_len;
      for (int base = 0; base < total; base += (int)blockDim.x * vjp::kGather) {
        double rz[vjp::kGather], ra[vjp::kGather];
        int to[vjp::kGather];
#pragma unroll
        for (int j = 0; j < vjp::kGather; ++j) {
          const int at = base + j * (int)blockDim.x + (int)threadIdx.x;
          to[j] = at < total ? at : total - 1; // = c * out_len + k: the place in pairs[c][k]
          const int c = to[j] / out_len, k = to[j] - c * out_len;
          const long from = c * col_stride + k;
          rz[j] = ps[from], ra[j] = pa[from];
        }
#pragma unroll
        for (int j = 0; j < vjp::kGather; ++j)
          pairs[to[j]] = make_double2(rz[j], ra[j]);
      }
      __syncthreads();
    }

    const Word *tb = table + e0;
    vjp::emit(pg, len, (int)threadIdx.x, (int)blockDim.x, [&](const int e) {
      const Word w = tb[e];
      const uint32_t ia = word_ia(w), ib = word_ib(w), code = word_code(w);
      // (z, lambda) of column c at both places
      auto at = [&](const int c, double2 &a, double2 &b) {
        if constexpr (STAGED) {
          a = pairs[c * out_len + ia], b = pairs[c * out_len + ib];
        } else {
          const double *cs = ps + c * col_stride, *ca = pa + c * col_stride;
          a = make_double2(cs[ia], ca[ia]), b = make_double2(cs[ib], ca[ib]);
        }
      };
      double2 a[NC], b[NC];
#pragma unroll
      for (int c = 0; c < NC; ++c)
        at(c, a[c], b[c]);
      double v;
      if constexpr (ACC)
        v = pg[e] * (code == kOne ? 1.0 : (code == kHalf ? 2.0 : -2.0));
      else
        v = __builtin_fma(a[0].y, b[0].x, a[0].x * b[0].y);
#pragma unroll
      for (int c = ACC ? 0 : 1; c < NC; ++c)
        v = __builtin_fma(a[c].y, b[c].x, __builtin_fma(a[c].x, b[c].y, v));
      const double s = code == kOne ? 1.0 : (code == kHalf ? 0.5 : -0.5);
      return code == kCopy ? 0.0 : v * s;
    });
  }
}

} // namespace tree_vjp
} // namespace sipamd
