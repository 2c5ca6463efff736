// chain_vjp.hip -- instantiations and launchers of the gradient kernel of the chain KKT solve (chain_vjp.hpp),
// declared in vjp_launch.hpp.  A translation unit of its own: compiled in parallel with the others.
#include "chain_vjp.hpp"
#include "vjp_launch.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>

namespace sipamd {
namespace vjp {

namespace {
// Dynamic LDS a launch may ask for without raising the kernel's limit.
constexpr size_t kLdsBudget = 64 * 1024;
// The launch shape kept after the measurement of DESIGN 4.11: wavefronts of a workgroup, and the bytes of z and lambda
// a workgroup's run of stages may take in LDS (the run is the longest that fits, the runs of a problem then evened out).
constexpr int kWaves = 8;
constexpr size_t kOperandBytes = 16 * 1024;

template <typename S, bool TABLE>
hipError_t launch_as(const Args &a, const Dims &d, const Shape &sh, hipStream_t stream) {
  hipLaunchKernelGGL((chain_vjp_kernel<S, TABLE>), dim3((unsigned)a.batch, (unsigned)sh.chunks),
                     dim3(kLanes * sh.waves), sh.lds_bytes, stream, d, (const S *)a.sol, (const S *)a.adj, a.status,
                     (S *)a.grad, sh.run);
  return hipGetLastError();
}

template <typename S>
hipError_t launch_table_or_not(const Args &a, const Dims &d, const Shape &sh, hipStream_t stream) {
  return sh.table ? launch_as<S, true>(a, d, sh, stream) : launch_as<S, false>(a, d, sh, stream);
}
} // namespace

Shape launch_shape(const Args &a) {
  const Dims d = residual::make_dims(a.n, a.m, a.T, a.symmetric);
  const int stages = a.T + 1;
  int waves = kWaves, run = 0; // run = 0: by kOperandBytes
  if (const char *env = std::getenv("SIP_LQR_VJP_SHAPE"))
    (void)std::sscanf(env, "%d,%d", &waves, &run);
  // the longest run whose z and lambda fit `bytes` (0: not even one stage's)
  auto longest = [&](size_t bytes) {
    const size_t fixed = operand_bytes(d, 0), stage = operand_bytes(d, 1) - fixed;
    return bytes < fixed + stage ? 0 : (int)std::min<size_t>((bytes - fixed) / stage, (size_t)stages);
  };
  const size_t tb = (size_t)table_bytes(d);
  const bool table = tb + operand_bytes(d, 1) <= kLdsBudget;
  const int most = longest(kLdsBudget - (table ? tb : 0));
  if (most < 1)
    return {0, 0, 0, false, 0};
  if (run < 1)
    run = std::max(1, longest(kOperandBytes));
  run = std::min(run, most);
  int chunks = (stages + run - 1) / run;
  if (chunks > 65535) // gridDim.y
    return {0, 0, 0, false, 0};
  run = (stages + chunks - 1) / chunks; // the same number of workgroups, runs of even length
  chunks = (stages + run - 1) / run;
  waves = waves < 1 ? 1 : (waves > kMaxWaves ? kMaxWaves : waves);
  waves = run < waves ? run : waves; // no more wavefronts than stages
  return {waves, chunks, run, table, (table ? tb : 0) + operand_bytes(d, run)};
}

hipError_t launch_vjp(const Args &a, hipStream_t stream) {
  const Shape sh = launch_shape(a);
  if (sh.waves < 1 || a.batch < 1 || a.batch > 0x7fffffffL)
    return hipErrorInvalidValue;
  const Dims d = residual::make_dims(a.n, a.m, a.T, a.symmetric);
  return a.f32 ? launch_table_or_not<float>(a, d, sh, stream) : launch_table_or_not<double>(a, d, sh, stream);
}

hipError_t launch_mask(long batch, long len, bool f32, const int32_t *status, void *vec, hipStream_t stream) {
  if (batch < 1 || batch > 0x7fffffffL)
    return hipErrorInvalidValue;
  if (f32)
    hipLaunchKernelGGL((vjp_mask_kernel<float>), dim3((unsigned)batch), dim3(256), 0, stream, len, status, (float *)vec);
  else
    hipLaunchKernelGGL((vjp_mask_kernel<double>), dim3((unsigned)batch), dim3(256), 0, stream, len, status,
                       (double *)vec);
  return hipGetLastError();
}

} // namespace vjp
} // namespace sipamd
