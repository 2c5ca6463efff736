// Prints the launch shape of the multi-column chain gradient kernel (csrc/vjp_cols_shape.hpp) for a fixed list of
// shapes, one line each: the inputs, then columns, waves, chunks, run, table and dynamic LDS bytes (columns 0: nothing
// fits).  Host only; tests/test_vjp_cols_shape.py checks every line against the rules the header states.
#include <cstdio>

#include "vjp_cols_shape.hpp"

namespace {
struct Case {
  int n, m, T, sym, requested, wish_waves, wish_run;
  long budget; // 0: the default operand budget
};
} // namespace

int main() {
  using namespace sipamd::vjp;
  const Case cases[] = {
      // full groups on the shapes of the tests and of the benchmark
      {1, 1, 0, 0, 8, 0, 0, 0},    {1, 1, 1, 0, 8, 0, 0, 0},    {3, 2, 3, 0, 8, 0, 0, 0},
      {4, 2, 20, 0, 8, 0, 0, 0},   {12, 4, 5, 0, 8, 0, 0, 0},   {12, 4, 5, 1, 8, 0, 0, 0},
      {12, 4, 50, 0, 8, 0, 0, 0},  {16, 8, 3, 0, 8, 0, 0, 0},   {32, 8, 2, 0, 8, 0, 0, 0},
      {32, 8, 100, 0, 8, 0, 0, 0}, {33, 17, 2, 0, 8, 0, 0, 0},  {64, 8, 12, 0, 8, 0, 0, 0},
      // 8 columns of one stage do not fit: 7 at (128, 1), 3 at (256, 4), 1 at (600, 8); 8 asked for is refused
      {128, 1, 1, 0, 7, 0, 0, 0},  {128, 1, 1, 0, 8, 0, 0, 0},  {256, 4, 3, 0, 3, 0, 0, 0},
      {600, 8, 2, 0, 1, 0, 0, 0},  {600, 8, 2, 0, 2, 0, 0, 0},
      // not even one column of one stage fits
      {1400, 8, 2, 0, 1, 0, 0, 0},
      // short groups, and the launch of the empty sum; at (64, 8) a short group has the table and a full one has not
      {12, 4, 50, 0, 1, 0, 0, 0},  {12, 4, 50, 0, 3, 0, 0, 0},  {12, 4, 50, 0, 0, 0, 0, 0},
      {32, 8, 100, 0, 1, 0, 0, 0}, {64, 8, 12, 0, 1, 0, 0, 0},  {64, 8, 12, 0, 4, 0, 0, 0},
      // the other operand budgets of the measurement
      {12, 4, 50, 0, 8, 0, 0, 16384}, {12, 4, 50, 0, 8, 0, 0, 65536}, {32, 8, 100, 0, 8, 0, 0, 16384},
      {4, 2, 20, 0, 8, 0, 0, 16384},
      // the measuring aids: wavefronts and run, a run too long for 64 KiB, more wavefronts than there are
      {12, 4, 50, 0, 8, 4, 9, 0},  {12, 4, 50, 0, 8, 2, 1000, 0}, {32, 8, 100, 0, 8, 99, 1, 0},
      {12, 4, 50, 0, 8, 4, 0, 0},
      // gridDim.y: 65535 runs of one stage are the limit
      {600, 8, 65534, 0, 1, 0, 1, 0}, {600, 8, 65535, 0, 1, 0, 1, 0}, {1, 1, 70000, 0, 8, 0, 1, 0},
      {1, 1, 65534, 0, 8, 0, 1, 0},
  };
  std::printf("budget %zu operand_budget %zu max_columns %d max_waves %d waves %d max_chunks %d min_run %d\n",
              kColsLdsBudget, kColsOperandBytes, kColsMax, kColsMaxWaves, kColsWaves, kColsMaxChunks, kColsMinRun);
  for (const Case &c : cases) {
    ColsWish wish;
    wish.waves = c.wish_waves, wish.run = c.wish_run;
    const ColsShape s = c.budget ? cols_shape(c.n, c.m, c.T, c.sym != 0, c.requested, wish, (size_t)c.budget)
                                 : cols_shape(c.n, c.m, c.T, c.sym != 0, c.requested, wish);
    std::printf("n %d m %d T %d sym %d requested %d wish_waves %d wish_run %d budget %ld per_launch %d -> columns %d "
                "waves %d chunks %d run %d table %d lds %zu\n",
                c.n, c.m, c.T, c.sym, c.requested, c.wish_waves, c.wish_run, c.budget, cols_per_launch(c.n, c.m),
                s.columns, s.waves, s.chunks, s.run, s.table ? 1 : 0, s.lds_bytes);
  }
  return 0;
}
