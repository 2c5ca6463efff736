// tree_vjp.hip -- instantiations and launcher of the gradient kernel of the tree KKT solve (tree_vjp.hpp), declared in
// tree_vjp_launch.hpp.  A translation unit of its own: compiled in parallel with the others.
#include "tree_vjp.hpp"
#include "tree_vjp_launch.hpp"

#include <cstdio>
#include <cstdlib>

namespace sipamd {
namespace tree_vjp {

namespace {
template <bool STAGED>
hipError_t launch_as(const Args &a, const Shape &sh, hipStream_t stream) {
  hipLaunchKernelGGL((tree_vjp_kernel<STAGED>), dim3((unsigned)a.batch, (unsigned)sh.runs), dim3(kLanes * sh.waves),
                     sh.lds_bytes, stream, a.table, a.in_len, (int)a.out_len, a.sol, a.adj, a.status, a.grad, sh.run);
  return hipGetLastError();
}
} // namespace

Shape shape_of_launch(const long in_len, const long out_len, const long batch) {
  int waves = 0;
  long run = 0;
  if (const char *env = std::getenv("SIP_LQR_TREE_VJP_SHAPE"))
    (void)std::sscanf(env, "%d,%ld", &waves, &run);
  return launch_shape(in_len, out_len, batch, waves, run);
}

hipError_t launch_tree_vjp(const Args &a, hipStream_t stream) {
  if (a.in_len < 1)
    return hipSuccess;
  if (a.batch < 1 || a.batch > 0x7fffffffL || a.table == nullptr || a.in_len > kMaxInputLen ||
      a.out_len > kMaxOutputLen)
    return hipErrorInvalidValue;
  const Shape sh = shape_of_launch(a.in_len, a.out_len, a.batch);
  if (sh.waves < 1)
    return hipErrorInvalidValue;
  return sh.staged ? launch_as<true>(a, sh, stream) : launch_as<false>(a, sh, stream);
}

} // namespace tree_vjp
} // namespace sipamd
