// Prints the launch shape of the multi-column chain residual (csrc/residual_cols_shape.hpp) for a fixed list of
// shapes, one line each: the inputs, then columns, waves, staged and dynamic LDS bytes.  Host only;
// tests/test_residual_cols_shape.py recomputes every line from the rules the header states.
#include <cstdio>

#include "residual_cols_shape.hpp"

namespace {
struct Case {
  int n, m, T, f32, sym, aligned, requested;
};
} // namespace

int main() {
  using namespace sipamd::residual;
  const Case cases[] = {
      {1, 1, 1, 0, 0, 1, 8},    {1, 1, 1, 1, 0, 1, 8},   {5, 3, 12, 0, 0, 1, 8},  {5, 3, 12, 1, 0, 1, 8},
      {12, 4, 50, 0, 0, 1, 8},  {12, 4, 50, 1, 0, 1, 8}, {16, 8, 50, 0, 0, 1, 8}, {16, 8, 50, 1, 0, 1, 8},
      {32, 8, 100, 0, 0, 1, 8}, {32, 8, 100, 1, 0, 1, 8}, {8, 4, 12, 0, 1, 1, 8}, {8, 4, 12, 1, 1, 1, 8},
      {35, 3, 12, 0, 0, 1, 8},  {60, 8, 12, 0, 0, 1, 8}, {64, 8, 12, 0, 0, 1, 8},
      // a `mats` that is not 16-byte aligned
      {12, 4, 50, 0, 0, 0, 8},  {32, 8, 100, 0, 0, 0, 8}, {5, 3, 12, 1, 0, 0, 8},
      // fewer stages than wavefronts
      {12, 4, 2, 0, 0, 1, 8},   {12, 4, 0, 0, 0, 1, 8},  {5, 3, 1, 1, 0, 1, 8},
      // short groups
      {12, 4, 50, 0, 0, 1, 1},  {12, 4, 50, 0, 0, 1, 3}, {12, 4, 50, 0, 0, 1, 5}, {32, 8, 100, 0, 0, 1, 1},
      {32, 8, 100, 0, 0, 1, 2}, {32, 8, 100, 1, 0, 1, 3}, {64, 8, 12, 0, 0, 1, 2},
  };
  std::printf("budget %zu max_columns %d max_waves %d want_waves %d\n", kColsLdsBudget, kColsMax, kColsMaxWaves,
              kColsWantWaves);
  for (const Case &c : cases) {
    const ColsShape s = cols_shape(c.n, c.m, c.T, c.f32 != 0, c.sym != 0, c.aligned != 0, c.requested);
    std::printf("n %d m %d T %d f32 %d sym %d aligned %d requested %d -> columns %d waves %d staged %d lds %zu\n", c.n,
                c.m, c.T, c.f32, c.sym, c.aligned, c.requested, s.columns, s.waves, s.staged ? 1 : 0, s.lds_bytes);
  }
  return 0;
}
