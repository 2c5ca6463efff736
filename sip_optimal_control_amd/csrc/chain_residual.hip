// chain_residual.hip -- instantiations and launchers of the chain KKT residual and of the refinement update
// (chain_residual.hpp), declared in residual_launch.hpp.  A translation unit of its own: compiled in parallel with the
// others, and the solve kernels keep their modules.
#include "chain_residual.hpp"
#include "residual_launch.hpp"

namespace sipamd {
namespace residual {

namespace {
// Dynamic LDS a launch may ask for without raising the kernel's limit.
constexpr size_t kLdsBudget = 64 * 1024;

template <typename S, typename V, bool STAGED>
hipError_t launch_as(const Args &a, const Dims &d, const Shape &sh, hipStream_t stream) {
  const int wave_bytes = (int)((sh.lds_bytes - kRedBytes) / sh.waves);
  hipLaunchKernelGGL((chain_residual_kernel<S, V, STAGED>), dim3((unsigned)a.batch), dim3(kLanes * sh.waves),
                     sh.lds_bytes, stream, d, (const S *)a.mats, (const V *)a.vecs, (const V *)a.sol, a.res,
                     (S *)a.scaled, a.scale, a.norm, wave_bytes);
  return hipGetLastError();
}

template <typename S, typename V>
hipError_t launch_staged_or_not(const Args &a, const Dims &d, const Shape &sh, hipStream_t stream) {
  return sh.staged ? launch_as<S, V, true>(a, d, sh, stream) : launch_as<S, V, false>(a, d, sh, stream);
}
} // namespace

Shape launch_shape(const Args &a) {
  const Dims d = make_dims(a.n, a.m, a.T, a.symmetric);
  const size_t zb = (size_t)z_doubles(d) * sizeof(double), room = kLdsBudget - kRedBytes;
  const size_t staged_wave = zb + (size_t)image_bytes(d, a.f32 ? 4 : 8);
  // the image is copied by 16-byte pieces from the piece that holds the stage's first scalar: mats must be aligned
  const bool staged = staged_wave <= room && ((uintptr_t)a.mats & 15) == 0;
  const size_t wave_bytes = staged ? staged_wave : zb;
  const int fit = (int)(room / wave_bytes);
  const int waves = fit < 1 ? 0 : (fit < kMaxWaves ? fit : kMaxWaves);
  const int useful = a.T + 1 < waves ? a.T + 1 : waves; // no more wavefronts than stages
  return {useful, staged, kRedBytes + (size_t)useful * wave_bytes};
}

hipError_t launch_residual(const Args &a, hipStream_t stream) {
  const Shape sh = launch_shape(a);
  if (sh.waves < 1 || a.batch < 1 || a.batch > 0x7fffffffL || (a.scaled != nullptr && a.scale == nullptr))
    return hipErrorInvalidValue;
  const Dims d = make_dims(a.n, a.m, a.T, a.symmetric);
  if (!a.f32)
    return launch_staged_or_not<double, double>(a, d, sh, stream);
  return a.wide ? launch_staged_or_not<float, double>(a, d, sh, stream)
                : launch_staged_or_not<float, float>(a, d, sh, stream);
}

hipError_t launch_update(long batch, long len, bool f32, const void *dvec, const double *scale, const int32_t *status,
                         double *sol64, hipStream_t stream) {
  const long blocks = (batch * len + 255) / 256;
  const dim3 grid((unsigned)(blocks < 1 ? 1 : (blocks > 16384 ? 16384 : blocks)));
  if (f32)
    hipLaunchKernelGGL((refine_update_kernel<float>), grid, dim3(256), 0, stream, batch, len, (const float *)dvec, scale,
                       status, sol64);
  else
    hipLaunchKernelGGL((refine_update_kernel<double>), grid, dim3(256), 0, stream, batch, len, (const double *)dvec,
                       scale, status, sol64);
  return hipGetLastError();
}

} // namespace residual
} // namespace sipamd
