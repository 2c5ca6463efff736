// tree_qw16_launch.hpp -- table entry of the fused tree kernels (tree_qw16.hip) for the tree C ABI.  No kernel is
// included here: what the host needs to know about a size class, the class reports.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "tree_schedule.hpp"

namespace sipamd {

struct TreeClass {
  int n, m; // padded state / control dimension of the class
  // scalars per problem of the fused scratch: padded gains of one edge, spill slot of one node (TreeLayout<n, m>)
  int gain_scalars, spill_scalars;
  const char *name;
  hipError_t (*launch)(const TreeSchedule &ts, const double *input, double *output, double *work, double *pgains,
                       double *spill, int32_t *status, long batch, hipStream_t s);
  // the same sweep that also writes every LQR::Workspace field into the work arena (sip_lqr_tree_factor_solve_workspace)
  hipError_t (*launch_export)(const TreeSchedule &ts, const double *input, double *output, double *work, double *pgains,
                              double *spill, int32_t *status, long batch, hipStream_t s);
  // several right-hand sides against the factor state of the work arena (tree_mrhs_qw16.hpp,
  // sip_lqr_tree_solve_multi): `cols` per column and problem TreeColLayout<n, m>::len scalars
  const char *multi_name;
  hipError_t (*launch_multi)(const TreeSchedule &ts, const double *input, const double *work, const double *rhs_cols,
                             double *out_cols, double *cols, const int32_t *status, long batch, int num_rhs,
                             hipStream_t s);
  long (*cols_len)(const TreeSchedule &ts);
  // the two halves of LQR::factor_with_status + LQR::solve as separate sweeps (sip_lqr_tree_factor_fused /
  // sip_lqr_tree_solve_fused): the factorization alone (FACTOR_ONLY instantiation of tree_qw16.hpp), and one
  // right-hand side from the input arena against the factor state of the work arena, v and k written into it
  // (SINGLE instantiation of tree_mrhs_qw16.hpp)
  const char *split_name;
  hipError_t (*launch_factor)(const TreeSchedule &ts, const double *input, double *work, double *pgains,
                              double *spill, int32_t *status, long batch, hipStream_t s);
  hipError_t (*launch_solve)(const TreeSchedule &ts, const double *input, double *work, double *output,
                             const int32_t *status, long batch, hipStream_t s);
};

// Smallest size class that holds a tree whose largest state / control dimensions are max_n / max_m;
// nullptr: none (max_n > 15 or max_m > 8): the general engine serves it.
const TreeClass *find_tree_class(int max_n, int max_m);

} // namespace sipamd
