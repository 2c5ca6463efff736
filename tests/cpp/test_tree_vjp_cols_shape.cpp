// Prints the launch shape of the multi-column tree gradient kernel (csrc/tree_vjp_cols_shape.hpp) for a fixed list of
// (in_len, out_len, batch, cap, requested, wish), one line each: the inputs, then the columns a launch carries on the
// plan (per_launch, with the cap), and of the launch of `requested` columns: columns, staged, waves (0: nothing to
// launch), runs, run and dynamic LDS bytes.  Host only; tests/test_tree_vjp_cols_shape.py checks every line against
// the rule the header states.
#include <cstdio>

#include "tree_vjp_cols_shape.hpp"

namespace {
struct Case {
  long in_len, out_len, batch;
  int cap, requested, wish_waves;
  long wish_run, wish_kib; // wish_kib < 0: the rule's budget
};
} // namespace

int main() {
  using namespace sipamd::tree_vjp;
  const Case cases[] = {
      // around out_len = 512 and 513 (8 columns fit 64 KiB, and do not), 1280 and 1281 (fit 160 KiB, and do not), 4096
      // (one column fills 64 KiB) and 4097 (the direct form with 8)
      {3000, 100, 4096, 0, 8, 0, 0, -1},   {20000, 512, 4096, 0, 8, 0, 0, -1},  {20000, 513, 4096, 0, 7, 0, 0, -1},
      {20000, 636, 4096, 0, 6, 0, 0, -1},  {40000, 1148, 4096, 0, 3, 0, 0, -1}, {40000, 1148, 1024, 0, 2, 0, 0, -1},
      {40000, 1280, 4096, 0, 8, 0, 0, -1}, {40000, 1281, 4096, 0, 7, 0, 0, -1}, {40000, 1148, 4096, 0, 8, 0, 0, -1},
      {90000, 4096, 300, 0, 1, 0, 0, -1},  {90000, 4097, 300, 0, 8, 0, 0, -1},  {66840, 4476, 3, 0, 8, 0, 0, -1},
      {66840, 4476, 3, 0, 1, 0, 0, -1},
      // short groups and the launch of the empty sum
      {20000, 512, 4096, 0, 1, 0, 0, -1},  {20000, 512, 4096, 0, 3, 0, 0, -1},  {20000, 512, 4096, 0, 0, 0, 0, -1},
      {20000, 636, 4096, 0, 1, 0, 0, -1},  {66840, 4476, 3, 0, 0, 0, 0, -1},
      // the cap
      {20000, 512, 4096, 3, 3, 0, 0, -1},  {20000, 512, 4096, 1, 1, 0, 0, -1},  {40000, 1148, 4096, 2, 2, 0, 0, -1},
      {40000, 1148, 4096, 5, 3, 0, 0, -1}, {66840, 4476, 3, 3, 3, 0, 0, -1},    {20000, 512, 4096, 8, 8, 0, 0, -1},
      // a batch below 256: several runs per problem
      {20000, 512, 3, 0, 8, 0, 0, -1},     {20000, 512, 255, 0, 8, 0, 0, -1},   {20000, 512, 256, 0, 8, 0, 0, -1},
      {151, 40, 3, 0, 8, 0, 0, -1},        {5001, 300, 100, 0, 8, 0, 0, -1},
      // an empty arena: nothing to launch
      {0, 0, 7, 0, 8, 0, 0, -1},           {0, 0, 7, 0, 0, 0, 0, -1},
      // the measuring aids: wavefronts and run, the raised limit, the direct form asked for
      {20000, 512, 4096, 0, 8, 4, 0, -1},  {20000, 512, 4096, 0, 8, 99, 64, -1}, {20000, 512, 3, 0, 8, 2, 1001, -1},
      {40000, 1148, 4096, 0, 8, 0, 0, 147}, {40000, 1148, 4096, 0, 8, 0, 0, 160}, {40000, 1148, 4096, 0, 8, 0, 0, 999},
      {40000, 1148, 4096, 0, 8, 0, 0, 0},   {40000, 1148, 4096, 4, 4, 0, 0, 147},
  };
  std::printf("budget %zu columns_budget %zu most %zu pair %zu max_columns %d max_waves %d lanes %d piece %d "
              "compute_units %ld min_run %ld max_runs %ld\n",
              kColsLdsBudget, kColsLdsColumns, kColsLdsMost, kColsPairBytes, kColsMax, kMaxWaves, kLanes, kPiece,
              kComputeUnits, kMinRun, kMaxRuns);
  for (const Case &c : cases) {
    ColsWish wish;
    wish.waves = c.wish_waves, wish.run = c.wish_run, wish.lds_kib = c.wish_kib, wish.columns = c.cap;
    const ColsShape s = cols_shape(c.in_len, c.out_len, c.batch, c.requested, wish);
    std::printf("in_len %ld out_len %ld batch %ld cap %d requested %d wish_waves %d wish_run %ld wish_kib %ld "
                "per_launch %d -> columns %d staged %d waves %d runs %ld run %ld lds %zu\n",
                c.in_len, c.out_len, c.batch, c.cap, c.requested, c.wish_waves, c.wish_run, c.wish_kib,
                cols_per_launch(c.out_len, c.cap, c.wish_kib), s.columns, s.at.staged ? 1 : 0, s.at.waves,
                s.at.runs, s.at.run, s.at.lds_bytes);
  }
  return 0;
}
