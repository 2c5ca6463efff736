// qf32_launch.hpp -- the rows, the layout and the launchers of the fused fp32 chain kernel (chain_qf32.hpp, instantiated
// in chain_qf32.hip) and of its separate sweeps (chain_qf32_sweeps.hpp, instantiated in chain_qf32_sweeps.hip), each a
// translation unit of its own.  No kernel source in here: the host code that looks kernels up (sip_lqr_amd.hip)
// includes this header alone.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

// (n, m) of every instantiation: the Newton-KKT / benchmark grid n in {4, 6, 8, 12} x m in {1, 2, 3, 4}, then the
// smallest shape, two odd ones and the largest one the kernel holds.  A row with a dimension that is new to this list
// also adds it to the fp32 sizes of gen_dpp_blocks.py.
#define SIP_QF32_ROWS(X)                                                                                     \
  X(4, 1) X(4, 2) X(4, 3) X(4, 4) X(6, 1) X(6, 2) X(6, 3) X(6, 4) X(8, 1) X(8, 2) X(8, 3) X(8, 4)            \
  X(12, 1) X(12, 2) X(12, 3) X(12, 4) X(1, 1) X(5, 3) X(9, 2) X(15, 8)

namespace sipamd {
namespace qf32 {

// Scalars per stage block of the packed chain layout (include/sip_lqr_amd.h) and of the kernel's workspace.
template <int N, int M>
struct Layout {
  static constexpr int NODE = N * N + N;                 // Q | delta
  static constexpr int EDGE = N * N + 2 * N * M + M * M; // A | B | M | R
  static constexpr int STG = NODE + EDGE;                // mats stage stride
  static constexpr int VNODE = 2 * N;                    // q | c   (x | y)
  static constexpr int VEDGE = M;                        // r       (u)
  static constexpr int VSTG = VNODE + VEDGE;             // vecs / sol stage stride
  static constexpr int GAIN = M * N + M;                 // K | k
  // The spill per node: [S | g | h] with the symmetric S = F^-1 in full (N * N scalars, column per lane as the
  // backward sweep holds it: whole-column stores, and the rollout reads row r as column r).  The packed triangle
  // would save N (N - 1) / 2 of the N^2 + 2 N scalars at the price of ragged stores; this kernel keeps the plain form.
  static constexpr int WG = N * N;          // offset of g in a slot; h follows at WG + N
  static constexpr int WSN = N * N + 2 * N; // ws_slot of the plan
};

// launch_fs_t of qw16_table.hpp; `mode` and `gfac` are ignored: the kernel always runs the full sweep (split
// factor / solve calls re-run it, see sip_lqr_plan::split_on_fused, unless the plan opted into the sweeps below).
template <int N, int M>
hipError_t launch_qf32(long batch, int T, const void *mats, const void *vecs, void *sol, void *gains, int32_t *status,
                       void *ws, hipStream_t stream, int mode, void *gfac);

// ---- the separate sweeps (sip_lqr_plan_set_separate_sweeps after sip_lqr_plan_set_fused_f32): launch_factor_sweep_t /
// launch_cols_t of qw16_table.hpp (chain_factor_qf32, chain_solve_cols_qf32) ----
constexpr int kQf32SolveColumns = 8; // columns one solve sweep carries
// cws[node][column][g (n) | h (n) | k (m)] of one problem
constexpr long qf32_col_workspace_scalars(int T, int n, int m, int ncols) { return (long)(T + 1) * ncols * (2 * n + m); }
constexpr char kQf32SeparateSuffix[] = " + chain_factor_qf32 + chain_solve_qf32";

template <int N, int M>
hipError_t launch_qf32_factor(long batch, int T, const void *mats, void *gains, int32_t *status, void *ws, void *gfac,
                              hipStream_t stream);
template <int N, int M>
hipError_t launch_qf32_solve(long batch, int T, const void *mats, const void *vecs_cols, void *sol_cols, void *gains,
                             void *ws, const void *gfac, void *cws, const int32_t *status, int ncols, long col_stride,
                             hipStream_t stream);

} // namespace qf32
} // namespace sipamd

// One row of the opt-in table (sip_lqr_plan_set_fused_f32): never part of find_kernel's search.
#define QF32_ENTRY(N, M)                                                                                     \
  sipamd::with_separate_sweeps({SIP_LQR_F32, N, M, "chain_factor_solve_qf32<" #N "," #M ",direct>/f32",      \
                                sipamd::qf32::Layout<N, M>::WSN, &sipamd::qf32::launch_qf32<N, M>},          \
                               {&sipamd::qf32::launch_qf32_factor<N, M>, &sipamd::qf32::launch_qf32_solve<N, M>, \
                                sipamd::qf32::kQf32SeparateSuffix, sipamd::qf32::kQf32SolveColumns, 2 * N + M}),
