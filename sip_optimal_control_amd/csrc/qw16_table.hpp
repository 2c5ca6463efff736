// qw16_table.hpp -- the table entry of the dedicated chain kernels and the slices of the fp64 fused kernels
// (qw16_kernels.hip), for the host code that looks kernels up (sip_lqr_amd.hip): no kernel source in here.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/sip_lqr_amd.h"
// the manifest of gen_qw16_kernels.py: slice count, slice list, the entries of each slice
#ifndef SIP_QW16_MANIFEST // tools/ab_build.sh, tools/diag_build.sh: a one-slice manifest of their own
#define SIP_QW16_MANIFEST "qw16_kernels_gen.hpp"
#endif
#include SIP_QW16_MANIFEST

#ifdef SIP_LQR_STAMPS
// Diagnostic build: device buffer of 8 x u64 per wave, set by the tool (sip_lqr_amd.hip).
extern unsigned long long *g_sip_lqr_stamps;
#define SIP_STAMP_PASS , g_sip_lqr_stamps
#else
#define SIP_STAMP_PASS
#endif

namespace sipamd {

// mode: 0 fused factor + solve, 1 factor only (+ the G factors to gfac), 2 solve only
typedef hipError_t (*launch_fs_t)(long batch, int T, const void *mats, const void *vecs, void *sol, void *gains,
                                  int32_t *status, void *ws, hipStream_t stream, int mode, void *gfac);

// A column sweep: LQR::solve for `ncols` right-hand sides `col_stride` scalars apart against a kept factor state.
// chain_mrhs.hpp (ncols <= kMrhsColumns; reads gains and ws only) and the solve sweeps of the n = 32 matrix-core kernels
// (mt16_launch.hpp; ncols <= kMt16SolveColumns) and of the fused fp32 kernels (qf32_launch.hpp; ncols <=
// kQf32SolveColumns).  cws != nullptr: the per-column state of the rollout goes through the column workspace;
// cws == nullptr (a solve sweep, ncols == 1): through the spill and the k part of `gains`.
typedef hipError_t (*launch_cols_t)(long batch, int T, const void *mats, const void *vecs_cols, void *sol_cols,
                                    void *gains, void *ws, const void *gfac, void *cws, const int32_t *status,
                                    int ncols, long col_stride, hipStream_t stream);
constexpr int kMrhsColumns = 8; // columns one multi-rhs launch carries

// The split form of the fused sweep (sip_lqr_factor_solve_split): mats carries [Q | delta | M | R] per
// stage, A | B stream from `ab` (scalars: ab + p * ab_pstride + i * ab_sstride).
typedef hipError_t (*launch_split_t)(long batch, int T, const void *mats, const void *ab, long ab_pstride,
                                     long ab_sstride, const void *vecs, void *sol, void *gains, int32_t *status,
                                     void *ws, hipStream_t stream);

// The separate sweeps of the n = 32 matrix-core kernels (sip_lqr_plan_set_separate_sweeps; mt16_launch.hpp).
// Factor sweep: W per node to `ws`, K to `gains`, -G^-1 per edge to `gfac` (M * M + M scalars per edge), the statuses;
// the solve sweep is a launch_cols_t.
typedef hipError_t (*launch_factor_sweep_t)(long batch, int T, const void *mats, void *gains, int32_t *status, void *ws,
                                            void *gfac, hipStream_t stream);

// The first six members every family has; an entry macro names, after them, only what its family adds.
struct KernelEntry {
  int dtype, n, m;
  const char *name;
  int ws_slot; // scalars of workspace per node
  launch_fs_t launch_fs;
  // the fp64 fused kernels (QW16_ENTRY)
  int layout = SIP_LQR_LAYOUT_FULL;      // SIP_LQR_LAYOUT_* of mats the kernel reads
  bool core = false;                     // a slice entry that SIP_LQR_EXTRA=0 leaves visible
  bool staged = false;                   // operands by LDS-DMA: find_embedding_kernel prefers these hosts
  bool solve_only = false;               // launch_fs honours mode 2 (else a split solve re-runs the full sweep)
  launch_cols_t launch_mrhs = nullptr;   // nullptr: this shape solves several right-hand sides column by column
  launch_split_t launch_split = nullptr; // nullptr: no split form of this kernel
  // the n = 32 matrix-core kernels (MT16_ENTRY) and the fused fp32 kernels (QF32_ENTRY); both nullptr: no separate
  // factor / solve sweeps to opt into
  launch_factor_sweep_t launch_factor_sweep = nullptr;
  launch_cols_t launch_solve_sweep = nullptr;
  const char *separate_suffix = "";      // what the opt-in appends to the plan's kernel name
  int sweep_columns = 0;                 // columns one launch of launch_solve_sweep carries
  int sweep_col_scalars = 0;             // scalars of column workspace per node and column
  // the fp64 fused kernels: the fused sweep (mode 0 only) on the kernel that keeps its first spill slots in registers
  // (chain_qw16.hpp, PARK); nullptr: the shape has none.  A plan of the shape itself runs sip_lqr_factor_solve on it
  // unless SIP_LQR_PARK=0 at its creation; embedded shapes and every other sweep stay on launch_fs.
  launch_fs_t launch_park = nullptr;
};
constexpr KernelEntry with_park(KernelEntry k, launch_fs_t launch_park) {
  k.launch_park = launch_park;
  return k;
}
// The separate sweeps of a row, and how its solve sweep carries columns.
struct SeparateSweeps {
  launch_factor_sweep_t factor;
  launch_cols_t solve;
  const char *suffix;
  int columns, col_scalars;
};
constexpr KernelEntry with_separate_sweeps(KernelEntry k, SeparateSweeps s) {
  k.launch_factor_sweep = s.factor, k.launch_solve_sweep = s.solve;
  k.separate_suffix = s.suffix, k.sweep_columns = s.columns, k.sweep_col_scalars = s.col_scalars;
  return k;
}

// slice s of qw16_kernels.hip defines qw16_slice_<s>: its share of the manifest's entries
#define SIP_QW16_DECLARE_SLICE(S) const KernelEntry *qw16_slice_##S(int *count);
QW16_FOR_EACH_SLICE(SIP_QW16_DECLARE_SLICE)
#undef SIP_QW16_DECLARE_SLICE

} // namespace sipamd
