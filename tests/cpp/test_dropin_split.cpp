// test_dropin_split.cpp -- the drop-in `LQR` with the split fused sweeps on (set_split_fused /
// SIP_LQR_DROPIN_SPLIT=1): factor_with_status() runs sip_lqr_tree_factor_fused and solve() runs
// sip_lqr_tree_solve_fused against the factor state factor left on the device, without refactoring.
//
// The reference's tests (tests/cpp/test_dropin.cpp, its fixtures and harness included below) run once with the
// switch on, then the cases of this file: a solve sees the factorization of the matrices at FACTOR time (a Q
// changed between factor and solve does not reach it, as in lqr.cpp, where solve() reads only the factor state,
// A, B, delta and the vectors), and one factor serves several right-hand sides (lqr_test.cpp:431-450).
//
// Build (also done by __graft_entry__.build()):
//   g++ -std=c++17 -O2 -D__HIP_PLATFORM_AMD__ tests/cpp/test_dropin_split.cpp -I include -I /opt/rocm/include \
//     -L sip_optimal_control_amd/lib -lsip_lqr_amd -L /opt/rocm/lib -lamdhip64 \
//     -Wl,-rpath,'$ORIGIN/../../sip_optimal_control_amd/lib' -Wl,-rpath,/opt/rocm/lib -o tests/cpp/test_dropin_split
#define main reference_suite_main
#include "test_dropin.cpp"
#undef main

namespace {

// factor, then solve, on a fresh object whose input is `p`; the split switch as given
Solution factor_then_solve(Problem &p, bool split, const std::function<void(Problem &)> &between = nullptr) {
  auto input = p.input();
  LQR::Workspace ws;
  ws.reserve(input.dimensions, input.topology);
  Solution s(p);
  {
    auto lqr = LQR(input, ws);
    lqr.set_split_fused(split);
    CHECK(lqr.uses_fused_tree_kernel());
    CHECK(lqr.factor_with_status() == Status::SUCCESS);
    if (between)
      between(p);
    auto out = s.output();
    lqr.solve(out);
  }
  ws.free(p.E());
  return s;
}

double max_diff(const Solution &a, const Solution &b) {
  double d = 0.0;
  auto cmp = [&](const std::vector<Vec> &x, const std::vector<Vec> &y) {
    for (size_t i = 0; i < x.size(); ++i)
      for (size_t j = 0; j < x[i].size(); ++j)
        d = std::fmax(d, std::fabs(x[i][j] - y[i][j]));
  };
  cmp(a.x, b.x), cmp(a.u, b.u), cmp(a.y, b.y);
  return d;
}

void change_Q(Problem &p) { // a different, still positive definite cost on every node
  for (auto &Q : p.Q)
    for (int i = 0; i < Q.rows; ++i)
      Q(i, i) += 3.0;
}

} // namespace

int main() {
  LQR::default_split_fused() = true; // the objects the reference's tests construct run split
  const int suite = reference_suite_main();
  LQR::default_split_fused() = false;
  struct Case { const char *name; std::function<void()> run; };
  std::vector<Case> cases = {
      {"LQRSplit.SolveUsesTheFactorizationOfFactorTime", [] {
         for (auto make : {branch_tree, variable_dimension_branch, five_node_tree}) {
           auto p = make();
           const Solution want = factor_then_solve(p, true); // Q unchanged: the plain split path
           auto p2 = make();
           const Solution got = factor_then_solve(p2, true, change_Q);
           CHECK(max_diff(got, want) == 0.0);
           // and the solve is the one of the original problem (the reference's residual)
           auto p3 = make();
           Solution s = factor_then_solve(p3, true, change_Q);
           CHECK(kkt_residual(make(), s) < 1e-12);
           // the default refactors at solve time: the changed Q does reach the solution there
           auto p4 = make();
           const Solution refactored = factor_then_solve(p4, false, change_Q);
           CHECK(max_diff(refactored, want) > 1e-6);
         }
       }},
      {"LQRSplit.OneFactorSeveralRightHandSides", [] {
         auto p = five_node_tree();
         auto input = p.input();
         LQR::Workspace ws;
         ws.reserve(input.dimensions, input.topology);
         {
           auto lqr = LQR(input, ws);
           lqr.set_split_fused(true);
           CHECK(lqr.factor_with_status() == Status::SUCCESS);
           for (int rep = 0; rep < 3; ++rep) {
             for (size_t i = 0; i < p.q.size(); ++i)
               for (size_t j = 0; j < p.q[i].size(); ++j)
                 p.q[i][j] = std::sin(0.7 * (rep + 1) + i + 0.3 * j), p.c[i][j] = std::cos(0.9 * rep + 2 * i + j);
             for (size_t e = 0; e < p.r.size(); ++e)
               for (size_t j = 0; j < p.r[e].size(); ++j)
                 p.r[e][j] = 0.5 * std::sin(1.3 * rep + e - j);
             Solution s(p);
             auto out = s.output();
             lqr.solve(out);
             CHECK(kkt_residual(p, s) < 1e-12);
           }
         }
         ws.free(p.E());
       }},
  };
  for (auto &c : cases) {
    const int before = g_failures;
    c.run();
    std::printf("[%s] %s\n", g_failures == before ? "  OK  " : "FAILED", c.name);
  }
  std::printf("split: %d checks, %d failures\n", g_checks, g_failures);
  return (suite == 0 && g_failures == 0) ? 0 : 1;
}
