// mt16_launch.hpp -- launchers of the n = 32 matrix-core chain kernels (chain_mt16.hpp), instantiated
// in chain_mt16.hip (a translation unit of its own: compiled in parallel with the others).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace sipamd {

// Same signature as launch_fs_t (qw16_table.hpp); `mode` is ignored: the kernel always runs the full
// sweep (split factor / solve calls re-run it, see sip_lqr_plan::split_on_fused).
template <typename S, int M>
hipError_t launch_mt16(long batch, int T, const void *mats, const void *vecs, void *sol, void *gains,
                       int32_t *status, void *ws, hipStream_t stream, int mode, void *gfac);

constexpr int kMt16SpillPerNode = 3 * 256 + 32; // Layout::WSN: three tiles of the symmetric W | g

// ---- the separate sweeps (sip_lqr_plan_set_separate_sweeps): launch_factor_sweep_t / launch_cols_t of
// qw16_table.hpp, instantiated in chain_mt16_solve.hip (chain_factor_mt16, chain_solve_mt16) ----
constexpr int kMt16SolveColumns = 16; // the columns of a 16 x 16 tile
constexpr long mt16_col_workspace_scalars(int T, int m, int ncols) { return (long)(T + 1) * ncols * (32 + m); }
constexpr char kSeparateSuffix[] = " + chain_factor_mt16 + chain_solve_mt16"; // what the opt-in appends to the name

template <typename S, int M>
hipError_t launch_mt16_factor(long batch, int T, const void *mats, void *gains, int32_t *status, void *ws, void *gfac,
                              hipStream_t stream);
template <typename S, int M>
hipError_t launch_mt16_solve(long batch, int T, const void *mats, const void *vecs_cols, void *sol_cols, void *gains,
                             void *ws, const void *gfac, void *cws, const int32_t *status, int ncols, long col_stride,
                             hipStream_t stream);

} // namespace sipamd

#define MT16_ENTRY(DT, S, TAG, M)                                                                            \
  sipamd::with_separate_sweeps({DT, 32, M, "chain_factor_solve_mt16<32," #M ",mfma16x16x4>/" TAG,            \
                                sipamd::kMt16SpillPerNode, &sipamd::launch_mt16<S, M>},                      \
                               {&sipamd::launch_mt16_factor<S, M>, &sipamd::launch_mt16_solve<S, M>,         \
                                sipamd::kSeparateSuffix, sipamd::kMt16SolveColumns, 32 + M})
