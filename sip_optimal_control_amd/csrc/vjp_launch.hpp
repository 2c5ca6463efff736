// vjp_launch.hpp -- the launchers of the gradient kernel of the chain KKT solve (chain_vjp.hpp, instantiated in
// chain_vjp.hip, a translation unit of its own).  No kernel source in here: the host code (sip_lqr_amd.hip) includes
// this header alone.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace sipamd {
namespace vjp {

// What one launch is told.  Buffers are whole-batch device pointers in the packed chain layout of
// include/sip_lqr_amd.h; sol, adj and grad share one scalar type.
struct Args {
  long batch;
  int T, n, m;
  bool f32;       // sol, adj and grad are float, else double
  bool symmetric; // SIP_LQR_LAYOUT_SYMMETRIC: Q and R of grad as packed lower triangles
  const void *sol, *adj;
  const int32_t *status; // nullptr, or per problem: != 0 gets zeros
  void *grad;
};

// Wavefronts of a workgroup, workgroups per problem (each a run of `run` stages) and dynamic LDS bytes of one launch;
// table: the decoded stage image sits in LDS.
struct Shape {
  int waves, chunks, run;
  bool table;
  size_t lds_bytes;
};
// waves == 0: the launch is not possible (z and lambda of one stage do not fit the LDS budget).
// SIP_LQR_VJP_SHAPE=<waves>,<stages per workgroup> (a measuring aid, read per call; 0 stages: the default run)
// replaces the default; a run too long for the LDS budget is cut to the longest that fits.
Shape launch_shape(const Args &a);

hipError_t launch_vjp(const Args &a, hipStream_t stream);

// vec[p] = 0 (`len` scalars per problem) where status[p] != SIP_LQR_SUCCESS
hipError_t launch_mask(long batch, long len, bool f32, const int32_t *status, void *vec, hipStream_t stream);

} // namespace vjp
} // namespace sipamd
