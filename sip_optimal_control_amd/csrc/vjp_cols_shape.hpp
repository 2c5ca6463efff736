// vjp_cols_shape.hpp -- the launch shape of the multi-column chain gradient kernel (chain_vjp_cols.hpp): how many
// columns one launch carries, how many wavefronts a workgroup has, how many stages its run spans, whether the decoded
// stage image sits in LDS, and the dynamic LDS that takes.  Host arithmetic only: no HIP call and no kernel in here, so
// a host program can print the decisions (tests/cpp/test_vjp_cols_shape.cpp).
//
// LDS of a workgroup: the table (one word per scalar of the stage image, padded to 16 bytes; only with `table`), then
// per column the pairs (z[k], lambda[k]) of the run: run (2 n + m) + 2 n pairs of 16 bytes, column after column.
//
// Rules: never more than 64 KiB.  Columns come first: a plan carries min(8, what fits without the table) columns per
// launch, and a group has the table exactly when the table and ONE stage of the group's columns fit together (a short
// group may have it where a full one has not).  The run is the longest whose columns fit the operand budget; where
// that is fewer than kColsMinRun stages the budget is dropped and the run is the longest the 64 KiB leave (a wavefront
// takes a stage at a time, so a run of 2 stages is a workgroup of 2 wavefronts: measured at n = 32).
// The runs of a problem are then evened out; gridDim.y <= 65535; no more wavefronts than stages of a run.
// columns == 0: nothing fits, and nothing is launched.
#pragma once
#include <cstddef>
#include <cstdio>
#include <cstdlib>

#include "residual_cols_shape.hpp" // cols_stage_scalars: the scalars of one stage of `mats`, stated there

// Bytes of LDS the pairs of one workgroup (all its columns) may take by default.  Measured at 16, 32 and 64 KiB
// (DESIGN 4.11.2); a build with another value here gives the other rows of that table.
#ifndef SIP_VJP_COLS_OPERAND_BYTES
#define SIP_VJP_COLS_OPERAND_BYTES (32 * 1024)
#endif
#ifndef SIP_VJP_COLS_WAVES
#define SIP_VJP_COLS_WAVES 8
#endif

namespace sipamd {
namespace vjp {

constexpr int kColsMax = 8;      // columns of the widest instantiation; the instantiations are 0 .. 8
constexpr int kColsMaxWaves = 8; // wavefronts of a workgroup, at the most (kMaxWaves of chain_vjp.hpp)
constexpr int kColsWaves = SIP_VJP_COLS_WAVES;
constexpr size_t kColsLdsBudget = 64 * 1024;
constexpr size_t kColsOperandBytes = SIP_VJP_COLS_OPERAND_BYTES;
constexpr int kColsMaxChunks = 65535; // gridDim.y
constexpr int kColsMinRun = 4;        // stages the operand budget must leave a run, or it does not apply

struct ColsShape {
  int columns; // of this launch (the group's); 0: nothing fits
  int waves, chunks, run;
  bool table;
  size_t lds_bytes;
};

// What the measuring aids ask for (0: the default).
struct ColsWish {
  int waves = 0, run = 0; // SIP_LQR_VJP_COLS_SHAPE=<wavefronts>,<stages>
  int columns = 0;        // SIP_LQR_VJP_MULTI_COLUMNS=<cap on columns per launch, 1..8>
};
inline ColsWish cols_wish_from_env() {
  ColsWish w;
  if (const char *env = std::getenv("SIP_LQR_VJP_COLS_SHAPE"))
    (void)std::sscanf(env, "%d,%d", &w.waves, &w.run);
  if (const char *env = std::getenv("SIP_LQR_VJP_MULTI_COLUMNS"))
    (void)std::sscanf(env, "%d", &w.columns);
  if (w.columns < 1 || w.columns > kColsMax)
    w.columns = 0;
  return w;
}

// table_bytes and operand_bytes of chain_vjp.hpp, from n, m and the layout (chain_vjp_cols.hip checks that they agree)
inline size_t cols_table_bytes(const int n, const int m, const bool sym) {
  return ((size_t)residual::cols_stage_scalars(n, m, sym) * 4 + 15) & ~(size_t)15;
}
inline size_t cols_operand_bytes(const int n, const int m, const int run) {
  return ((size_t)run * (2 * n + m) + 2 * (size_t)n) * 16;
}

// Columns one launch carries on this shape: 8, or fewer where 8 columns of one stage do not fit; 0: not even one.
inline int cols_per_launch(const int n, const int m) {
  const size_t fit = kColsLdsBudget / cols_operand_bytes(n, m, 1);
  return (int)(fit < (size_t)kColsMax ? fit : (size_t)kColsMax);
}

// The shape of the launch that carries `requested` columns (1 .. cols_per_launch; 0 is the launch of the empty sum and
// is shaped like one column).
inline ColsShape cols_shape(const int n, const int m, const int T, const bool sym, const int requested,
                            const ColsWish wish = ColsWish(), const size_t operand_budget = kColsOperandBytes) {
  const ColsShape none = {0, 0, 0, 0, false, 0};
  const int nc = requested < 1 ? 1 : requested;
  if (nc > cols_per_launch(n, m))
    return none;
  const size_t stages = (size_t)T + 1;
  const size_t fixed = (size_t)nc * cols_operand_bytes(n, m, 0);
  const size_t stage = (size_t)nc * cols_operand_bytes(n, m, 1) - fixed;
  const size_t tb = cols_table_bytes(n, m, sym);
  const bool table = tb + fixed + stage <= kColsLdsBudget;
  // the longest run whose pairs fit `bytes` (0: not even one stage's)
  auto longest = [&](const size_t bytes) {
    if (bytes < fixed + stage)
      return (size_t)0;
    const size_t r = (bytes - fixed) / stage;
    return r < stages ? r : stages;
  };
  const size_t most = longest(kColsLdsBudget - (table ? tb : 0));
  if (most < 1)
    return none;
  size_t run = wish.run >= 1 ? (size_t)wish.run : longest(operand_budget);
  if (wish.run < 1 && run < (size_t)kColsMinRun)
    run = most;
  run = run < 1 ? 1 : (run > most ? most : run);
  size_t chunks = (stages + run - 1) / run;
  if (chunks > (size_t)kColsMaxChunks)
    return none;
  run = (stages + chunks - 1) / chunks; // the same number of workgroups, runs of even length
  chunks = (stages + run - 1) / run;
  int waves = wish.waves >= 1 ? wish.waves : kColsWaves;
  waves = waves > kColsMaxWaves ? kColsMaxWaves : waves;
  waves = run < (size_t)waves ? (int)run : waves; // no more wavefronts than stages
  return {nc, waves, (int)chunks, (int)run, table,
          (table ? tb : 0) + (size_t)nc * cols_operand_bytes(n, m, (int)run)};
}

} // namespace vjp
} // namespace sipamd
