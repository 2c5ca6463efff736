// qw16_launch.hpp -- host-side launchers of the fused fp64 chain kernels and the table entry that
// instantiates them, for the slices of qw16_kernels.hip (which shape goes where: gen_qw16_kernels.py).
#pragma once
#include "qw16_table.hpp"
#include "chain_mrhs.hpp"
#include "chain_qw16.hpp"

namespace sipamd {

#ifndef SIP_MRHS_GROUP
#define SIP_MRHS_GROUP 8 // (measured at (12, 4), 8 columns: groups of 8 / 4 / 2 -> 0.69 / 0.94 / 1.3 ms: the sweep is bandwidth-bound, smaller groups re-fetch the operands)
#endif
constexpr int kMrhsGroup = SIP_MRHS_GROUP; // columns one wavefront carries of the kMrhsColumns of a launch (chain_mrhs.hpp)

template <int N, int M, bool WPACK>
hipError_t launch_mrhs_qw16(long batch, int T, const void *mats, const void *vecs_cols, void *sol_cols,
                            void *gains, void *ws, const void *gfac, void *cws, const int32_t *status, int ncols,
                            long col_stride, hipStream_t stream) {
  if (ncols < 1 || ncols > kMrhsColumns)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL((chain_solve_mrhs_qw16<N, M, WPACK, kMrhsGroup>),
                     dim3((unsigned)((batch + 3) / 4), (unsigned)((ncols + kMrhsGroup - 1) / kMrhsGroup)), dim3(64), 0, stream, (const double *)mats, (const double *)vecs_cols, (double *)sol_cols,
                     (const double *)gains, (const double *)ws, (const double *)gfac, (double *)cws,
                     (const int *)status, batch, T, ncols, col_stride);
  return hipGetLastError();
}

// PARK: the fused sweep (mode 0) runs on the kernel that keeps the spill of its first KEEP nodes in accumulation
// registers (chain_qw16.hpp); the factor and solve sweeps, whose spill IS the factor state later launches read, run on
// the plain kernel of the shape.
template <int N, int M, bool STAGED, bool WPACK, bool SYM = false, bool PARK = false>
hipError_t launch_qw16(long batch, int T, const void *mats, const void *vecs, void *sol, void *gains,
                       int32_t *status, void *ws, hipStream_t stream, int mode, void *gfac) {
  using Cfg = StagedCfg<N, M, WPACK, false, SYM>;
  const unsigned blocks = (unsigned)((batch + 3) / 4);
  const unsigned lds = STAGED ? Cfg::LDS_BYTES : 0;
  if (STAGED) {
    // LDS-DMA moves 16-byte pieces: every base must be 16-byte aligned.
    const uintptr_t bits = (uintptr_t)mats | (uintptr_t)vecs | (uintptr_t)gains | (uintptr_t)ws;
    if (bits & 15)
      return hipErrorInvalidValue;
  }
  if (PARK && mode == 0)
    hipLaunchKernelGGL((chain_factor_solve_qw16<N, M, STAGED, WPACK, false, SYM, PARK>), dim3(blocks), dim3(64), lds,
                       stream, (const double *)mats, (const double *)vecs, (double *)sol, (double *)gains, (double *)ws,
                       (int *)status, batch, T, mode, (double *)gfac, (const double *)nullptr, 0L, 0L SIP_STAMP_PASS);
  else
    hipLaunchKernelGGL((chain_factor_solve_qw16<N, M, STAGED, WPACK, false, SYM>), dim3(blocks), dim3(64), lds, stream,
                       (const double *)mats, (const double *)vecs, (double *)sol, (double *)gains, (double *)ws,
                       (int *)status, batch, T, mode, (double *)gfac, (const double *)nullptr, 0L, 0L SIP_STAMP_PASS);
  return hipGetLastError();
}

// KernelEntry::launch_park of an entry: the parked fused sweep where the manifest lists the shape, else none.
template <int N, int M, bool STAGED, bool SYM>
constexpr launch_fs_t park_launcher() {
  if constexpr (STAGED && QW16_PARKED(N, M))
    return &launch_qw16<N, M, STAGED, STAGED, SYM, true>;
  else
    return nullptr;
}

// The split form of the fused sweep (launch_split_t): A | B stream from where the model callback left them.
template <int N, int M, bool SYM = false>
hipError_t launch_qw16_split(long batch, int T, const void *mats, const void *ab, long ab_pstride, long ab_sstride,
                             const void *vecs, void *sol, void *gains, int32_t *status, void *ws,
                             hipStream_t stream) {
  using Cfg = StagedCfg<N, M, true, true, SYM>;
  // 16-byte aligned arrays of this library's own layouts; A | B -- the caller's -- at any 8-byte aligned place and
  // strides: a stage's A | B is a whole number of 16-byte pieces (AB even, StagedCfg) and the LDS-DMA of gfx950 copies
  // pieces exactly from sources that are only 8-byte aligned (tools/ubench/lds_dma_align.hip), as the odd-length
  // stage blocks of `mats` already rely on
  const uintptr_t bits = (uintptr_t)mats | (uintptr_t)vecs | (uintptr_t)gains | (uintptr_t)ws;
  if ((bits & 15) || ((uintptr_t)ab & 7))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL((chain_factor_solve_qw16<N, M, true, true, true, SYM>), dim3((unsigned)((batch + 3) / 4)), dim3(64),
                     Cfg::LDS_BYTES, stream, (const double *)mats, (const double *)vecs, (double *)sol,
                     (double *)gains, (double *)ws, (int *)status, batch, T, 0, (double *)nullptr,
                     (const double *)ab, ab_pstride, ab_sstride SIP_STAMP_PASS);
  return hipGetLastError();
}

} // namespace sipamd

// One entry of a slice (the manifest's QW16_SLICE_ENTRIES_<s>).  STAGED: LDS-DMA double buffering + packed
// symmetric S spill (n <= 15), else every lane loads its columns from global memory (any n <= 16); SYM: the
// symmetric-packed layout (SIP_LQR_LAYOUT_SYMMETRIC: Q and R as packed lower triangles).  MRHS / SPLIT name
// the macro below that instantiates the multi-right-hand-side solve / the split form, or QW16_NONE.
#define QW16_NONE(...) nullptr
#define QW16_MRHS(N, M, STAGED, SYM) &sipamd::launch_mrhs_qw16<N, M, STAGED>
#define QW16_SPLIT(N, M, STAGED, SYM) &sipamd::launch_qw16_split<N, M, SYM>
// A staged entry of a shape the manifest lists as parked (QW16_PARKED) carries a second launcher, launch_park: the
// fused sweep that parks its first spill slots in registers.  The factor and solve sweeps, the column sweep and the
// split form of the entry stay the plain kernel's.
#define QW16_ENTRY(N, M, STAGED, SYM, TAG, CORE, MRHS, SPLIT)                                                  \
  sipamd::with_park({ SIP_LQR_F64, N, M, "chain_factor_solve_qw16<" #N "," #M "," TAG ">/f64",                 \
    sipamd::StagedCfg<N, M, STAGED, false, SYM>::WSN, &sipamd::launch_qw16<N, M, STAGED, STAGED, SYM>,         \
    SYM ? SIP_LQR_LAYOUT_SYMMETRIC : SIP_LQR_LAYOUT_FULL, CORE, STAGED, /*solve_only*/ true,                   \
    MRHS(N, M, STAGED, SYM), SPLIT(N, M, STAGED, SYM) }, sipamd::park_launcher<N, M, STAGED, SYM>())
