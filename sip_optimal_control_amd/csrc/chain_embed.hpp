// chain_embed.hpp -- the per-problem lengths of the packed chain layout (include/sip_lqr_amd.h) and the embedding of
// an (n, m) chain in the (N, M) chain of a larger fused fp64 kernel: the extra states / controls decouple exactly
// (Q = I, R = I, delta = 1 on their diagonal, zeros elsewhere: x = y = u = 0 there), by a device-side repack before
// and after the sweep.  Included by sip_lqr_amd.hip alone.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/sip_lqr_amd.h"

namespace sipamd {

// Scalars per problem of a chain's arrays; split_mats: mats without A | B (sip_lqr_factor_solve_split).
struct ChainLens {
  long mats, vecs, gains, split_mats;
};
inline ChainLens chain_lens(long n, long m, long T, int layout) {
  const bool sym = layout == SIP_LQR_LAYOUT_SYMMETRIC; // Q and R as packed lower triangles
  const long node = (sym ? n * (n + 1) / 2 : n * n) + n, rlen = sym ? m * (m + 1) / 2 : m * m;
  return {(T + 1) * node + T * (n * n + 2 * n * m + rlen), (T + 1) * 2 * n + T * m, T * (m * n + m),
          (T + 1) * node + T * (n * m + rlen)};
}

namespace embed {

struct PadDims {
  int n, m, N, M, T;
  long mats_len, vecs_len, gains_len, pmats_len, pvecs_len, pgains_len;
};
inline PadDims pad_dims(int n, int m, int N, int M, int T) {
  const ChainLens own = chain_lens(n, m, T, SIP_LQR_LAYOUT_FULL), host = chain_lens(N, M, T, SIP_LQR_LAYOUT_FULL);
  return {n, m, N, M, T, own.mats, own.vecs, own.gains, host.mats, host.vecs, host.gains};
}

// blockIdx.y: problem (strided), blockIdx.x: stage; the threads sweep the padded stage block.
// Small-integer quotients via float reciprocals (exact for the sizes involved, < 2^12).
__device__ __forceinline__ int div_small(const int v, const float inv) { return (int)(((float)v + 0.5f) * inv); }

static __global__ void __launch_bounds__(256)
pad_mats_kernel(const PadDims d, const double *__restrict__ mats, double *__restrict__ pm, long batch) {
  const int n = d.n, m = d.m, N = d.N, M = d.M;
  const int i = blockIdx.x; // stage (the terminal stage has only the node block)
  const int pnode = N * N + N, pstage = pnode + N * N + 2 * N * M + M * M;
  const int stage = n * n + n + n * n + 2 * n * m + m * m;
  const int count = i < d.T ? pstage : pnode;
  const float invN = 1.0f / (float)N, invM = 1.0f / (float)M;
  for (long prob = blockIdx.y; prob < batch; prob += gridDim.y) {
    const double *src = mats + prob * d.mats_len + (long)i * stage;
    double *dst = pm + prob * d.pmats_len + (long)i * pstage;
    for (int at = threadIdx.x; at < count; at += blockDim.x) {
      double v;
      int o = at;
      if (o < N * N) { // Q: identity on the extra diagonal
        const int col = div_small(o, invN), row = o - col * N;
        v = (row < n && col < n) ? src[row + n * col] : (row == col ? 1.0 : 0.0);
      } else if ((o -= N * N) < N) { // delta: 1 on the extra states
        v = o < n ? src[n * n + o] : 1.0;
      } else if ((o -= N) < N * N) { // A
        const int col = div_small(o, invN), row = o - col * N;
        v = (row < n && col < n) ? src[n * n + n + row + n * col] : 0.0;
      } else if ((o -= N * N) < N * M) { // B
        const int col = div_small(o, invN), row = o - col * N;
        v = (row < n && col < m) ? src[2 * n * n + n + row + n * col] : 0.0;
      } else if ((o -= N * M) < N * M) { // M (cross term)
        const int col = div_small(o, invN), row = o - col * N;
        v = (row < n && col < m) ? src[2 * n * n + n + n * m + row + n * col] : 0.0;
      } else { // R: identity on the extra diagonal
        o -= N * M;
        const int col = div_small(o, invM), row = o - col * M;
        v = (row < m && col < m) ? src[2 * n * n + n + 2 * n * m + row + m * col] : (row == col ? 1.0 : 0.0);
      }
      dst[at] = v;
    }
  }
}

// vecs -> padded vecs (zeros on the extras); PAD = false: padded sol -> sol
// (skip != nullptr: problems with skip[problem] != 0 are left alone -- the solve sweep wrote nothing for them)
template <bool PAD>
static __global__ void __launch_bounds__(256)
pad_vecs_kernel(const PadDims d, const double *__restrict__ src_all, double *__restrict__ dst_all, long batch,
                const int32_t *__restrict__ skip = nullptr) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long len = PAD ? d.pvecs_len : d.vecs_len;
  if (idx >= batch * len)
    return;
  const long prob = idx / len;
  if (skip != nullptr && skip[prob] != 0)
    return;
  long at = idx - prob * len;
  const int n = d.n, m = d.m, N = d.N, M = d.M;
  const int a = PAD ? N : n, b = PAD ? M : m;   // dims of the layout this thread indexes
  const int oa = PAD ? n : N, ob = PAD ? m : M; // dims of the other layout
  const int i = (int)(at / (2 * a + b));
  const int o = (int)(at - (long)i * (2 * a + b));
  int other = -1; // offset inside the other layout's stage, -1: an extra (padded) entry
  if (o < a)
    other = o < n ? o : -1;
  else if (o < 2 * a)
    other = (o - a) < n ? oa + (o - a) : -1;
  else
    other = (o - 2 * a) < m ? 2 * oa + (o - 2 * a) : -1;
  const long other_at = prob * (PAD ? d.vecs_len : d.pvecs_len) + (long)i * (2 * oa + ob) + other;
  dst_all[idx] = other >= 0 ? src_all[other_at] : 0.0;
}

// padded gains (K: M x N, k: M) -> gains (K: m x n, k: m)
static __global__ void __launch_bounds__(256)
unpad_gains_kernel(const PadDims d, const double *__restrict__ pg, double *__restrict__ gains, long batch) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= batch * d.gains_len)
    return;
  const long prob = idx / d.gains_len;
  long at = idx - prob * d.gains_len;
  const int n = d.n, m = d.m, N = d.N, M = d.M;
  const int i = (int)(at / (m * n + m));
  const int o = (int)(at - (long)i * (m * n + m));
  const double *src = pg + prob * d.pgains_len + (long)i * (M * N + M);
  if (o < m * n) {
    const int col = o / m, row = o - col * m;
    gains[idx] = src[row + M * col];
  } else {
    gains[idx] = src[M * N + (o - m * n)];
  }
}

inline dim3 grid_of(long count) { return dim3((unsigned)((count + 255) / 256)); }

// Before the sweep: mats and vecs into the host kernel's dimensions.  mats == nullptr: the padded matrices of an
// earlier call are still in place; vecs == nullptr: the caller fills pvecs itself.  Launch errors are left to the
// caller's hipGetLastError.
inline void embed_inputs(const PadDims &d, long B, const void *mats, void *pmats, const void *vecs, void *pvecs,
                         hipStream_t s) {
  if (mats != nullptr)
    hipLaunchKernelGGL(pad_mats_kernel, dim3((unsigned)(d.T + 1), (unsigned)(B < 65535 ? B : 65535)), dim3(256), 0, s,
                       d, (const double *)mats, (double *)pmats, B);
  if (vecs != nullptr)
    hipLaunchKernelGGL(pad_vecs_kernel<true>, grid_of(B * d.pvecs_len), dim3(256), 0, s, d, (const double *)vecs,
                       (double *)pvecs, B, (const int32_t *)nullptr);
}

// After the sweep: the solution (sol != nullptr; problems with skip[problem] != 0 left alone) and the gains
// (gains != nullptr) back in the plan's dimensions.
inline void extract_outputs(const PadDims &d, long B, const void *psol, void *sol, const int32_t *skip,
                            const void *pgains, void *gains, hipStream_t s) {
  if (sol != nullptr)
    hipLaunchKernelGGL(pad_vecs_kernel<false>, grid_of(B * d.vecs_len), dim3(256), 0, s, d, (const double *)psol,
                       (double *)sol, B, skip);
  if (gains != nullptr && d.gains_len > 0)
    hipLaunchKernelGGL(unpad_gains_kernel, grid_of(B * d.gains_len), dim3(256), 0, s, d, (const double *)pgains,
                       (double *)gains, B);
}

} // namespace embed
} // namespace sipamd
