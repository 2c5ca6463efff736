// tree_vjp.hpp -- the gradient of a scalar loss L(z) with respect to the input arena of a tree plan, through the tree
// KKT system K z + b = 0 (the mathematics and the table: tree_vjp_table.hpp).  The twin of chain_vjp.hpp on the tree
// arenas: a streaming kernel, fp64.
//
// Shape: blockIdx.x is the problem, blockIdx.y a run of consecutive entries of the input arena.  STAGED: the workgroup
// first brings z and lambda of its problem -- the whole output arena, once -- into LDS as pairs (z[k], lambda[k]),
// kGather loads per lane in flight and no branch between the loads and their LDS stores; after the barrier nothing is
// read but the table and LDS.  A lane takes 16-byte pieces of the gradient array, consecutive lanes consecutive pieces
// (vjp::emit of chain_vjp.hpp: the pieces are those of the address, what is left at either end of a run goes scalar by
// scalar, so an odd input_len and an output one scalar off 16 bytes are exact); per entry one table word and two LDS
// reads.  Where the pairs of a problem do not fit the LDS budget, the other form reads z and lambda in place.
// Arithmetic: fma(lambda[ia], z[ib], z[ia] * lambda[ib]) -- two roundings, the operand order of the chain kernel, so a
// chain written as a tree gives what chain_vjp_kernel gives -- times s (exact); a copy is lambda[ia] as it stands.
// Every scalar of the gradient is written exactly once, nothing else is written, and there are no atomics: two
// launches give the same bits.  A problem whose status is not SIP_LQR_SUCCESS gets zeros by a branch that is the
// same in every lane: its z and lambda are not read.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "chain_vjp.hpp" // vjp::emit, vjp::kGather
#include "tree_vjp_table.hpp"

namespace sipamd {
namespace tree_vjp {

// Dynamic LDS: STAGED, out_len pairs.  run: entries per workgroup (Shape::run).
template <bool STAGED>
__global__ void __launch_bounds__(kLanes * kMaxWaves)
    tree_vjp_kernel(const Word *__restrict__ table, const long in_len, const int out_len,
                    const double *__restrict__ sol, const double *__restrict__ adj,
                    const int32_t *__restrict__ status, double *__restrict__ grad, const long run) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const long p = blockIdx.x;
  const long e0 = (long)blockIdx.y * run;
  if (e0 >= in_len)
    return;
  const int len = (int)(in_len - e0 < run ? in_len - e0 : run);
  double *pg = grad + p * in_len + e0;

  if (status != nullptr && status[p] != 0) { // a branch, the same in every lane: sol and adj may hold anything
    vjp::emit(pg, len, (int)threadIdx.x, (int)blockDim.x, [](int) { return 0.0; });
    return;
  }

  const double *ps = sol + p * (long)out_len, *pa = adj + p * (long)out_len;
  double2 *pairs = (double2 *)lds;
  if constexpr (STAGED) {
    // A thread past the end loads and stores the last entry again: in bounds, the same value to the same place, and
    // no branch between the loads and the stores, which would leave one load in flight at a time.
    for (int base = 0; base < out_len; base += (int)blockDim.x * vjp::kGather) {
      double rz[vjp::kGather], ra[vjp::kGather];
      int k[vjp::kGather];
#pragma unroll
      for (int j = 0; j < vjp::kGather; ++j) {
        const int at = base + j * (int)blockDim.x + (int)threadIdx.x;
        k[j] = at < out_len ? at : out_len - 1;
        rz[j] = ps[k[j]], ra[j] = pa[k[j]];
      }
#pragma unroll
      for (int j = 0; j < vjp::kGather; ++j)
        pairs[k[j]] = make_double2(rz[j], ra[j]);
    }
    __syncthreads();
  }

  const Word *tb = table + e0;
  vjp::emit(pg, len, (int)threadIdx.x, (int)blockDim.x, [&](const int e) {
    const Word w = tb[e];
    const uint32_t ia = word_ia(w), ib = word_ib(w), code = word_code(w);
    double2 a, b; // (z, lambda)
    if constexpr (STAGED) {
      a = pairs[ia], b = pairs[ib];
    } else {
      a = make_double2(ps[ia], pa[ia]), b = make_double2(ps[ib], pa[ib]);
    }
    const double v = __builtin_fma(a.y, b.x, a.x * b.y);
    const double s = code == kOne ? 1.0 : (code == kHalf ? 0.5 : -0.5);
    return code == kCopy ? a.y : v * s;
  });
}

} // namespace tree_vjp
} // namespace sipamd
