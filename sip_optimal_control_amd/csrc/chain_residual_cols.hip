// chain_residual_cols.hip -- instantiations and launchers of the chain KKT residual and of the refinement update
// (chain_residual.hpp), for one column and for several, declared in residual_launch.hpp.  A translation unit of its
// own: compiled in parallel with the others, and the solve kernels keep their modules.
#include "chain_residual.hpp"
#include "residual_launch.hpp"

namespace sipamd {
namespace residual {

namespace {
template <typename S, typename V, bool STAGED, int NC>
hipError_t launch_cols_as(const Args &a, const Dims &d, const ColsShape &sh, int ncols, hipStream_t stream) {
  const int wave_bytes = (int)((sh.lds_bytes - cols_red_bytes(NC)) / sh.waves);
  hipLaunchKernelGGL((chain_residual_kernel<S, V, STAGED, NC>), dim3((unsigned)a.batch), dim3(kLanes * sh.waves),
                     sh.lds_bytes, stream, d, (const S *)a.mats, (const V *)a.vecs, (const V *)a.sol,
                     a.batch * d.vecs_len, a.batch, ncols, a.res, (S *)a.scaled, a.scale, a.norm, wave_bytes);
  return hipGetLastError();
}

template <typename S, typename V, bool STAGED>
hipError_t launch_cols_instance(const Args &a, const Dims &d, const ColsShape &sh, int ncols, hipStream_t stream) {
  switch (sh.columns) {
  case 1: return launch_cols_as<S, V, STAGED, 1>(a, d, sh, ncols, stream);
  case 2: return launch_cols_as<S, V, STAGED, 2>(a, d, sh, ncols, stream);
  case 4: return launch_cols_as<S, V, STAGED, 4>(a, d, sh, ncols, stream);
  case 8: return launch_cols_as<S, V, STAGED, 8>(a, d, sh, ncols, stream);
  default: return hipErrorInvalidValue;
  }
}

template <typename S, typename V>
hipError_t launch_cols_staged_or_not(const Args &a, const Dims &d, const ColsShape &sh, int ncols, hipStream_t stream) {
  return sh.staged ? launch_cols_instance<S, V, true>(a, d, sh, ncols, stream)
                   : launch_cols_instance<S, V, false>(a, d, sh, ncols, stream);
}
} // namespace

ColsShape cols_launch_shape(const Args &a, int requested) {
  return cols_shape(a.n, a.m, a.T, a.f32, a.symmetric, ((uintptr_t)a.mats & 15) == 0, requested);
}

hipError_t launch_residual_cols(const Args &a, int num_cols, hipStream_t stream) {
  if (num_cols < 1 || a.batch < 1 || a.batch > 0x7fffffffL || (a.scaled != nullptr && a.scale == nullptr))
    return hipErrorInvalidValue;
  const Dims d = make_dims(a.n, a.m, a.T, a.symmetric);
  const size_t vec_bytes = a.f32 && !a.wide ? 4 : 8, out_bytes = a.f32 ? 4 : 8;
  const long stride = a.batch * d.vecs_len;
  const int group = cols_launch_shape(a, kColsMax).columns; // what a full launch carries for this plan and mats
  if (group < 1)
    return hipErrorInvalidValue;
  for (int c0 = 0; c0 < num_cols; c0 += group) {
    const int nc = num_cols - c0 < group ? num_cols - c0 : group;
    const ColsShape sh = cols_launch_shape(a, nc);
    if (sh.columns < nc || sh.waves < 1)
      return hipErrorInvalidValue;
    Args g = a;
    g.vecs = (const char *)a.vecs + (size_t)c0 * stride * vec_bytes;
    g.sol = (const char *)a.sol + (size_t)c0 * stride * vec_bytes;
    g.res = a.res ? a.res + (size_t)c0 * stride : nullptr;
    g.scaled = a.scaled ? (char *)a.scaled + (size_t)c0 * stride * out_bytes : nullptr;
    g.scale = a.scale ? a.scale + (size_t)c0 * a.batch : nullptr;
    g.norm = a.norm + (size_t)c0 * a.batch;
    const hipError_t e = !a.f32     ? launch_cols_staged_or_not<double, double>(g, d, sh, nc, stream)
                         : a.wide   ? launch_cols_staged_or_not<float, double>(g, d, sh, nc, stream)
                                    : launch_cols_staged_or_not<float, float>(g, d, sh, nc, stream);
    if (e != hipSuccess)
      return e;
  }
  return hipSuccess;
}

hipError_t launch_update_cols(long cols, long batch, long len, bool f32, const void *dvec, const double *scale,
                              const int32_t *status, double *sol64, hipStream_t stream) {
  const long blocks = (cols * batch * len + 255) / 256;
  const dim3 grid((unsigned)(blocks < 1 ? 1 : (blocks > 16384 ? 16384 : blocks)));
  if (f32)
    hipLaunchKernelGGL((refine_update_kernel<float>), grid, dim3(256), 0, stream, cols, batch, len,
                       (const float *)dvec, scale, status, sol64);
  else
    hipLaunchKernelGGL((refine_update_kernel<double>), grid, dim3(256), 0, stream, cols, batch, len,
                       (const double *)dvec, scale, status, sol64);
  return hipGetLastError();
}

} // namespace residual
} // namespace sipamd
