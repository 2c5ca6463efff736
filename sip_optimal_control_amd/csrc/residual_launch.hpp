// residual_launch.hpp -- the launchers of the KKT residual and of the refinement update on the packed chain layout
// (chain_residual.hpp, instantiated in chain_residual_cols.hip, a translation unit of its own).  No kernel source in
// here: the host code (sip_lqr_amd.hip) includes this header alone.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "residual_cols_shape.hpp"

namespace sipamd {
namespace residual {

// What one launch of the residual kernel is told.  Buffers are whole-batch device pointers in the packed chain layout
// of include/sip_lqr_amd.h; lengths are per problem, in scalars.
struct Args {
  long batch;
  int T, n, m;
  bool f32;       // mats (and the scaled output) are float, else double
  bool wide;      // vecs and sol are double whatever `f32` says
  bool symmetric; // SIP_LQR_LAYOUT_SYMMETRIC: Q and R as packed lower triangles
  const void *mats, *vecs, *sol;
  // plain form (scaled == nullptr): res may be nullptr; scaled form: rho / s in the plan's dtype, s next to norm
  double *res;
  void *scaled;
  double *scale;
  double *norm;
};

// `a` describes column 0: vecs, sol, res and scaled are [num_cols][batch][vecs_len] arrays (sip_lqr_solve_multi's
// layout), norm and scale [num_cols][batch]; the single-column entry points pass num_cols = 1.  The columns go in
// groups of cols_launch_shape(a, kColsMax).columns, one launch per group, a short last group on the least
// instantiation that holds it.
ColsShape cols_launch_shape(const Args &a, int requested);
hipError_t launch_residual_cols(const Args &a, int num_cols, hipStream_t stream);

// sol64[c][p] += scale[c][p] * d[c][p] (d in the plan's dtype, `len` scalars per problem and column) where
// status == nullptr or status[p] == SIP_LQR_SUCCESS (status per problem)
hipError_t launch_update_cols(long cols, long batch, long len, bool f32, const void *d, const double *scale,
                              const int32_t *status, double *sol64, hipStream_t stream);

} // namespace residual
} // namespace sipamd
