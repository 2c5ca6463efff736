// tree_vjp_cols.hip -- instantiations and launcher of the multi-column gradient kernel of the tree KKT solve
// (tree_vjp_cols.hpp), declared in tree_vjp_cols_launch.hpp.  A translation unit of its own: compiled in parallel with
// the others.
#include "tree_vjp_cols.hpp"
#include "tree_vjp_cols_launch.hpp"

#include <algorithm>

namespace sipamd {
namespace tree_vjp {

namespace {
// One group: `sol` and `adj` point at its first column.
struct Group {
  const double *sol, *adj;
  bool accumulate;
};

template <bool STAGED, int NC, bool ACC>
hipError_t launch_as(const Args &a, const Group &g, const Shape &sh, hipStream_t stream) {
  const auto kernel = tree_vjp_cols_kernel<STAGED, NC, ACC>;
  if (sh.lds_bytes > kLdsBudget) { // beyond the default limit of dynamic LDS: raised for this instantiation
    const hipError_t e = hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)sh.lds_bytes);
    if (e != hipSuccess)
      return e;
  }
  hipLaunchKernelGGL(kernel, dim3((unsigned)a.batch, (unsigned)sh.runs), dim3(kLanes * sh.waves), sh.lds_bytes, stream,
                     a.table, a.in_len, (int)a.out_len, g.sol, g.adj, a.batch * a.out_len, a.status, a.grad, sh.run);
  return hipGetLastError();
}

template <bool STAGED, bool ACC>
hipError_t launch_columns(const int nc, const Args &a, const Group &g, const Shape &sh, hipStream_t stream) {
  switch (nc) {
  case 1: return launch_as<STAGED, 1, ACC>(a, g, sh, stream);
  case 2: return launch_as<STAGED, 2, ACC>(a, g, sh, stream);
  case 3: return launch_as<STAGED, 3, ACC>(a, g, sh, stream);
  case 4: return launch_as<STAGED, 4, ACC>(a, g, sh, stream);
  case 5: return launch_as<STAGED, 5, ACC>(a, g, sh, stream);
  case 6: return launch_as<STAGED, 6, ACC>(a, g, sh, stream);
  case 7: return launch_as<STAGED, 7, ACC>(a, g, sh, stream);
  case 8: return launch_as<STAGED, 8, ACC>(a, g, sh, stream);
  default: return hipErrorInvalidValue;
  }
}

hipError_t launch_group(const int nc, const Args &a, const Group &g, const Shape &sh, hipStream_t stream) {
  if (nc == 0) { // the empty sum: nothing is staged and the table is not read
    Shape zeros = sh;
    zeros.lds_bytes = 0;
    return launch_as<false, 0, false>(a, g, zeros, stream);
  }
  if (g.accumulate)
    return sh.staged ? launch_columns<true, true>(nc, a, g, sh, stream)
                     : launch_columns<false, true>(nc, a, g, sh, stream);
  return sh.staged ? launch_columns<true, false>(nc, a, g, sh, stream)
                   : launch_columns<false, false>(nc, a, g, sh, stream);
}
} // namespace

hipError_t launch_tree_vjp_cols(const Args &a, const int num_rhs, hipStream_t stream) {
  if (num_rhs < 0)
    return hipErrorInvalidValue;
  if (a.in_len < 1)
    return hipSuccess;
  if (a.batch < 1 || a.batch > 0x7fffffffL || a.table == nullptr || a.in_len > kMaxInputLen ||
      a.out_len > kMaxOutputLen)
    return hipErrorInvalidValue;
  const ColsWish wish = cols_wish_from_env();
  const int cap = cols_per_launch(a.out_len, wish.columns, wish.lds_kib);
  const size_t column = (size_t)a.batch * (size_t)a.out_len;
  int col0 = 0;
  do { // once for the empty sum
    const int nc = std::min(cap, num_rhs - col0);
    const ColsShape sh = cols_shape(a.in_len, a.out_len, a.batch, nc, wish);
    // what the shape header states is what the kernel lays out, and a staged launch fits a workgroup
    if (sh.at.waves < 1 || sh.at.lds_bytes != (sh.at.staged ? (size_t)sh.columns * (size_t)a.out_len * 16 : 0) ||
        sh.at.lds_bytes > kColsLdsMost || (nc > 0 && sh.columns != nc))
      return hipErrorInvalidValue;
    const Group g{a.sol + (size_t)col0 * column, a.adj + (size_t)col0 * column, col0 > 0};
    const hipError_t e = launch_group(nc, a, g, sh.at, stream);
    if (e != hipSuccess)
      return e;
    col0 += nc;
  } while (col0 < num_rhs);
  return hipSuccess;
}

} // namespace tree_vjp
} // namespace sipamd
