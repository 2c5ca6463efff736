// chain_vjp_cols.hip -- instantiations and launchers of the multi-column gradient kernel of the chain KKT solve
// (chain_vjp_cols.hpp), declared in vjp_cols_launch.hpp.  A translation unit of its own: compiled in parallel with the
// others.
#include "chain_vjp_cols.hpp"
#include "vjp_cols_launch.hpp"

#include <algorithm>

namespace sipamd {
namespace vjp {

static_assert(kColsMaxWaves == kMaxWaves, "vjp_cols_shape.hpp states the wavefronts of chain_vjp.hpp");

namespace {
// One group: `sol` and `adj` point at its first column.
struct Group {
  const void *sol, *adj;
  bool accumulate;
};

template <typename S, bool TABLE, int NC, bool ACC>
hipError_t launch_as(const Args &a, const Group &g, const Dims &d, const ColsShape &sh, hipStream_t stream) {
  hipLaunchKernelGGL((chain_vjp_cols_kernel<S, TABLE, NC, ACC>), dim3((unsigned)a.batch, (unsigned)sh.chunks),
                     dim3(kLanes * sh.waves), sh.lds_bytes, stream, d, (const S *)g.sol, (const S *)g.adj,
                     a.batch * d.vecs_len, a.status, (S *)a.grad, sh.run);
  return hipGetLastError();
}

template <typename S, bool TABLE, bool ACC>
hipError_t launch_columns(const int nc, const Args &a, const Group &g, const Dims &d, const ColsShape &sh,
                          hipStream_t stream) {
  switch (nc) {
  case 1: return launch_as<S, TABLE, 1, ACC>(a, g, d, sh, stream);
  case 2: return launch_as<S, TABLE, 2, ACC>(a, g, d, sh, stream);
  case 3: return launch_as<S, TABLE, 3, ACC>(a, g, d, sh, stream);
  case 4: return launch_as<S, TABLE, 4, ACC>(a, g, d, sh, stream);
  case 5: return launch_as<S, TABLE, 5, ACC>(a, g, d, sh, stream);
  case 6: return launch_as<S, TABLE, 6, ACC>(a, g, d, sh, stream);
  case 7: return launch_as<S, TABLE, 7, ACC>(a, g, d, sh, stream);
  case 8: return launch_as<S, TABLE, 8, ACC>(a, g, d, sh, stream);
  default: return hipErrorInvalidValue;
  }
}

template <typename S>
hipError_t launch_group(const int nc, const Args &a, const Group &g, const Dims &d, const ColsShape &sh,
                        hipStream_t stream) {
  if (nc == 0) // the empty sum: the table is not read, so either form will do
    return launch_as<S, false, 0, false>(a, g, d, sh, stream);
  if (g.accumulate)
    return sh.table ? launch_columns<S, true, true>(nc, a, g, d, sh, stream)
                    : launch_columns<S, false, true>(nc, a, g, d, sh, stream);
  return sh.table ? launch_columns<S, true, false>(nc, a, g, d, sh, stream)
                  : launch_columns<S, false, false>(nc, a, g, d, sh, stream);
}
} // namespace

hipError_t launch_vjp_cols(const Args &a, const int num_rhs, hipStream_t stream) {
  if (num_rhs < 0 || a.batch < 1 || a.batch > 0x7fffffffL)
    return hipErrorInvalidValue;
  const Dims d = residual::make_dims(a.n, a.m, a.T, a.symmetric);
  const ColsWish wish = cols_wish_from_env();
  int cap = cols_per_launch(a.n, a.m);
  if (wish.columns > 0)
    cap = std::min(cap, wish.columns);
  if (cap < 1)
    return hipErrorInvalidValue;
  const size_t column = (size_t)a.batch * (size_t)d.vecs_len * (a.f32 ? 4 : 8);
  int col0 = 0;
  do { // once for the empty sum
    const int nc = std::min(cap, num_rhs - col0);
    const ColsShape sh = cols_shape(a.n, a.m, a.T, a.symmetric, nc, wish);
    // what the shape header states from n and m is what the kernel lays out from Dims
    if (sh.columns < 1 ||
        sh.lds_bytes != (sh.table ? (size_t)table_bytes(d) : 0) + (size_t)sh.columns * operand_bytes(d, sh.run) ||
        sh.lds_bytes > kColsLdsBudget || (nc > 0 && sh.columns != nc))
      return hipErrorInvalidValue;
    const Group g{(const char *)a.sol + (size_t)col0 * column, (const char *)a.adj + (size_t)col0 * column, col0 > 0};
    const hipError_t e = a.f32 ? launch_group<float>(nc, a, g, d, sh, stream)
                               : launch_group<double>(nc, a, g, d, sh, stream);
    if (e != hipSuccess)
      return e;
    col0 += nc;
  } while (col0 < num_rhs);
  return hipSuccess;
}

hipError_t launch_mask_cols(const int num_rhs, const long batch, const long len, const bool f32,
                            const int32_t *status, void *vec, hipStream_t stream) {
  if (num_rhs < 0 || batch < 1 || batch > 0x7fffffffL)
    return hipErrorInvalidValue;
  const size_t column = (size_t)batch * (size_t)len * (f32 ? 4 : 8);
  for (int col0 = 0; col0 < num_rhs; col0 += kColsMaxChunks) { // gridDim.y
    const unsigned cols = (unsigned)std::min(kColsMaxChunks, num_rhs - col0);
    void *at = (char *)vec + (size_t)col0 * column;
    if (f32)
      hipLaunchKernelGGL((vjp_mask_cols_kernel<float>), dim3((unsigned)batch, cols), dim3(256), 0, stream, len,
                         batch * len, status, (float *)at);
    else
      hipLaunchKernelGGL((vjp_mask_cols_kernel<double>), dim3((unsigned)batch, cols), dim3(256), 0, stream, len,
                         batch * len, status, (double *)at);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess)
      return e;
  }
  return hipSuccess;
}

} // namespace vjp
} // namespace sipamd
