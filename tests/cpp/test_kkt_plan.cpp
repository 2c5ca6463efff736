// The layouts of a Newton-KKT plan (csrc/kkt_plan.hpp: the arena tables and walk_arena, vector_layout), printed for a
// fixed list of dimension sets: tests/test_kkt_plan.py holds every offset against the oracle's tables and the
// first-order arena against the order include/sip_kkt_amd.h documents.  Needs no device.
//
// Build (also done by __graft_entry__.build()):
//   hipcc -x hip --offload-arch=gfx950 -std=c++17 -O1 tests/cpp/test_kkt_plan.cpp -o build/test_kkt_plan
#define SIP_KKT_CHAIN_UNIT // the structs and descriptions only
#include "../../sip_optimal_control_amd/csrc/kkt_plan.hpp"

#include <cstdio>

using namespace sipamd::kkt;

sip_kkt_plan::~sip_kkt_plan() {} // the plans of this program own no back end and no device memory

namespace {

struct DimSet {
  const char *name;
  int root;
  std::vector<int> parents, children, sd, cd, ncd, ngd, ecd, egd;
};

DimSet chain(const char *name, int n, int m, int T, int cn, int gn, int cT, int gT, int ce, int ge) {
  DimSet d{name, 0, {}, {}, std::vector<int>(T + 1, n), std::vector<int>(T, m), std::vector<int>(T + 1, cn),
           std::vector<int>(T + 1, gn), std::vector<int>(T, ce), std::vector<int>(T, ge)};
  for (int e = 0; e < T; ++e)
    d.parents.push_back(e), d.children.push_back(e + 1);
  d.ncd[T] = cT, d.ngd[T] = gT;
  return d;
}

const DimSet sets[] = {
    chain("family (4, 1), T = 3", 4, 1, 3, 0, 0, 2, 2, 2, 2),
    chain("uniform chain with interior constraints", 5, 3, 4, 1, 2, 3, 2, 2, 3),
    chain("one-edge chain", 3, 2, 1, 1, 0, 2, 1, 1, 2),
    {"single node", 0, {}, {}, {3}, {}, {2}, {1}, {}, {}},
    // the two of tests/test_gpu_first_order.py: odd dimensions and zero constraint dimensions; root 2, a node without
    // a state, an edge without a control
    {"non-uniform chain", 0, {0, 1, 2, 3, 4, 5}, {1, 2, 3, 4, 5, 6}, {4, 6, 5, 3, 6, 4, 5}, {2, 3, 1, 2, 3, 2},
     {1, 0, 2, 0, 1, 0, 2}, {0, 2, 0, 1, 0, 0, 3}, {1, 2, 0, 1, 1, 0}, {2, 0, 1, 1, 0, 2}},
    {"branching tree", 2, {2, 0, 2, 0}, {0, 3, 1, 4}, {3, 5, 4, 0, 2}, {2, 0, 3, 1}, {1, 0, 2, 1, 0}, {0, 2, 1, 0, 3},
     {1, 0, 2, 1}, {2, 1, 0, 1}},
};

void print_list(const char *what, const std::vector<int> &v) {
  std::printf("dims %s", what);
  for (const int x : v)
    std::printf(" %d", x);
  std::printf("\n");
}

template <size_t B>
void print_offsets(const char *arena, const sip_kkt_plan &p, const std::vector<long> (&off)[B], const int node_blocks) {
  for (size_t b = 0; b < B; ++b)
    for (int i = 0; i < ((int)b < node_blocks ? p.N : p.E); ++i)
      std::printf("off %s %zu %d %ld\n", arena, b, i, off[b][i]);
}

int print_set(const DimSet &d, const int th) {
  sip_kkt_plan p;
  const int E = (int)d.cd.size();
  set_dims(p, 3, E, d.root, d.parents.data(), d.children.data(), d.sd.data(), d.cd.data(), d.ncd.data(), d.ngd.data(),
           d.ecd.data(), d.egd.data(), 0);
  std::printf("set %s | theta %d | root %d\n", d.name, th, d.root);
  print_list("parents", p.parents), print_list("children", p.children), print_list("sd", p.sd), print_list("cd", p.cd);
  print_list("ncd", p.ncd), print_list("ngd", p.ngd), print_list("ecd", p.ecd), print_list("egd", p.egd);
  if (!validate(p, true))
    return 1;
  p.model_len = walk_arena(p, MODEL_ARENA, 0, p.moff);
  vector_layout(p);
  p.first_len = walk_arena(p, FIRST_ORDER_ARENA, th, p.foff);
  p.theta_len = th > 0 ? walk_arena(p, THETA_ARENA, th, p.toff) : 0;
  std::printf("len x %d y %d z %d model %ld first %ld theta %ld\n", p.x_dim, p.y_dim, p.z_dim, p.model_len,
              p.first_len, p.theta_len);
  print_offsets("model", p, p.moff, N_JG + 1);
  for (int t = 0; t < 7; ++t) {
    const bool per_edge = t == SIP_KKT_X_CONTROL || t == SIP_KKT_Y_EDGE_C || t == SIP_KKT_Z_EDGE;
    for (int i = 0; i < (per_edge ? p.E : p.N); ++i)
      std::printf("off vector %d %d %d\n", t, i, p.voff[t][i]);
  }
  print_offsets("first", p, p.foff, FO_N_G + 1);
  if (th > 0)
    print_offsets("theta", p, p.toff, TH_N_TT + 1);
  return 0;
}

} // namespace

int main() {
  int failures = 0;
  for (const DimSet &d : sets)
    for (const int th : {0, 3})
      failures += print_set(d, th);
  return failures == 0 ? 0 : 1;
}
