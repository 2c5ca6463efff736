// tree_vjp_cols_shape.hpp -- the launch shape of the multi-column tree gradient kernel (tree_vjp_cols.hpp): how many
// columns one launch carries, whether their (z, lambda) pairs go through LDS, how many wavefronts a workgroup has, how
// many entries of the input arena its run spans, and the dynamic LDS that takes.  Host arithmetic only: no HIP call and
// no kernel in here, so a host program can print the decisions (tests/cpp/test_tree_vjp_cols_shape.cpp).
//
// LDS of a staged workgroup: per column the pairs (z[k], lambda[k]) of the whole output arena of its problem, out_len
// pairs of 16 bytes, column after column (pairs[c][k]).
//
// THE RULE (stated here and nowhere else).  A plan is staged where one column fits kColsLdsBudget = 64 KiB, the dynamic
// LDS a launch may ask for without raising the kernel's limit; where not even one fits (16 out_len > 64 KiB) the launch
// is the direct form, which reads z and lambda in place, with 8 columns.  A staged launch carries
// min(8, kColsLdsColumns / (16 out_len)) columns with kColsLdsColumns = 160 KiB, what a gfx950 workgroup may declare:
// where a group needs more than 64 KiB the launcher raises the limit of that instantiation (one workgroup per compute
// unit then).  Measured on the reference's variable-shape trees (out_len = 1148, 8 columns): 8 columns
// in 144 KiB take 0.61-0.70 of the time of 3 + 3 + 2 columns within 64 KiB and 0.36-0.43 of the direct form with 8, at
// batch 4096 and at 1024, far beyond the spread over blocks; groups of 4 in 72 KiB lie between (level at batch 1024).
// Those two candidates stay reachable through the third field of SIP_LQR_TREE_VJP_COLS_SHAPE for measurement.
// Wavefronts and run: tree_vjp::launch_shape of tree_vjp_table.hpp, 8 wavefronts and one run per problem unless the
// batch is below 256.  waves == 0: nothing to launch (an empty input arena).
#pragma once
#include <cstddef>
#include <cstdio>
#include <cstdlib>

#include "tree_vjp_table.hpp"

namespace sipamd {
namespace tree_vjp {

constexpr int kColsMax = 8;                    // columns of the widest instantiation; the instantiations are 0 .. 8
constexpr size_t kColsLdsBudget = 64 * 1024;   // one column must fit this for the plan to be staged
constexpr size_t kColsLdsMost = 160 * 1024;    // what a gfx950 workgroup may declare
constexpr size_t kColsLdsColumns = kColsLdsMost; // what the columns of one staged launch may take together (the rule)
constexpr size_t kColsPairBytes = 16;          // (z[k], lambda[k])

// What the measuring aids ask for (0, or lds_kib < 0: the default).
struct ColsWish {
  int waves = 0;     // SIP_LQR_TREE_VJP_COLS_SHAPE=<wavefronts>,<entries per run>[,<KiB of LDS; 0: the direct form>]
  long run = 0;
  long lds_kib = -1; // the one budget in place of the rule's two
  int columns = 0;   // SIP_LQR_TREE_VJP_MULTI_COLUMNS=<cap on columns per launch, 1..8>
};
inline ColsWish cols_wish_from_env() {
  ColsWish w;
  if (const char *env = std::getenv("SIP_LQR_TREE_VJP_COLS_SHAPE"))
    (void)std::sscanf(env, "%d,%ld,%ld", &w.waves, &w.run, &w.lds_kib);
  if (const char *env = std::getenv("SIP_LQR_TREE_VJP_MULTI_COLUMNS"))
    (void)std::sscanf(env, "%d", &w.columns);
  if (w.columns < 1 || w.columns > kColsMax)
    w.columns = 0;
  return w;
}

// Columns that go through LDS together; 0: not even one (the direct form).  lds_kib < 0: the rule.
inline int cols_staged_fit(const long out_len, const long lds_kib = -1) {
  if (out_len < 1)
    return kColsMax;
  const size_t column = kColsPairBytes * (size_t)out_len;
  size_t room = kColsLdsColumns;
  if (lds_kib >= 0)
    room = (size_t)lds_kib * 1024 < kColsLdsMost ? (size_t)lds_kib * 1024 : kColsLdsMost;
  else if (column > kColsLdsBudget)
    return 0;
  const size_t fit = room / column;
  return (int)(fit < (size_t)kColsMax ? fit : (size_t)kColsMax);
}

// Columns one launch carries on this plan: what fits, or 8 in the direct form; `cap` (0: none) on top.
inline int cols_per_launch(const long out_len, const int cap = 0, const long lds_kib = -1) {
  const int fit = cols_staged_fit(out_len, lds_kib);
  const int cols = fit > 0 ? fit : kColsMax;
  return cap >= 1 && cap < cols ? cap : cols;
}

struct ColsShape {
  int columns = 0; // of this launch (the group's)
  Shape at;        // staged, waves (0: nothing to launch), run, runs, lds_bytes
};

// The shape of the launch that carries `requested` columns (1 .. cols_per_launch; 0 is the launch of the empty sum and
// is shaped like one column).
inline ColsShape cols_shape(const long in_len, const long out_len, const long batch, const int requested,
                            const ColsWish wish = ColsWish()) {
  ColsShape s;
  const int nc = requested < 1 ? 1 : requested;
  s.columns = nc;
  s.at = launch_shape(in_len, out_len, batch, wish.waves, wish.run);
  if (s.at.waves < 1)
    return s;
  s.at.staged = cols_staged_fit(out_len, wish.lds_kib) >= nc;
  s.at.lds_bytes = s.at.staged ? (size_t)nc * (size_t)out_len * kColsPairBytes : 0;
  return s;
}

} // namespace tree_vjp
} // namespace sipamd
