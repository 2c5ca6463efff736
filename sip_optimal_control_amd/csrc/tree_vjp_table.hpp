// tree_vjp_table.hpp -- what a tree plan decides on the host for the gradient kernel of the tree KKT solve
// (tree_vjp.hpp): the table that says, for every scalar of the input arena, which two places of the output arena its
// gradient is made from, and the launch shape.  Host arithmetic only: no kernel and no HIP call in here, so a host
// program can print both (tests/cpp/test_tree_vjp_table.cpp).  The kernel header includes it for the word it shares.
//
// The mathematics (include/sip_lqr_amd.h, sip_lqr_tree_vjp): the tree entry points solve K z + b = 0 with
// z = (x_i, y_i per node; u_e per edge), b = (q_i, c_i; r_e) and K symmetric.  With g = dL/dz the adjoint l solves
// K l + g = 0; dL/db = l and dL/dK = l z^T, so for node i and for edge e with parent p and child c
//
//   Q_i (n x n)    (r, col)  1/2 (lx_i[r] x_i[col] + x_i[r] lx_i[col]), the whole square
//   q_i, c_i       j         lx_i[j], ly_i[j]
//   delta_i        j         -ly_i[j] y_i[j]
//   A_e (nc x np)  (r, col)  ly_c[r] x_p[col] + y_c[r] lx_p[col]
//   B_e (nc x m)   (r, col)  ly_c[r] u_e[col] + y_c[r] lu_e[col]
//   M_e (np x m)   (r, col)  lx_p[r] u_e[col] + x_p[r] lu_e[col]
//   R_e (m x m)    (r, col)  1/2 (lu_e[r] u_e[col] + u_e[r] lu_e[col])
//   r_e            j         lu_e[j]
//
// Every entry is s (l[ia] z[ib] + z[ia] l[ib]) with ia, ib offsets into the output arena and s one of 1, 1/2, -1/2
// (delta: ia = ib, s = -1/2; the diagonal of Q or R: ia = ib, s = 1/2), or the plain copy l[ia] (q, c, r).  One word
// per input-arena scalar holds (ia, ib, code); the offsets come from the plan's own tables (oQ .. orr, ox, oy, ou,
// parents, children), so the layout is not stated here a second time, and the table is the same for every problem.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define SIP_TREE_VJP_HD __host__ __device__
#else
#define SIP_TREE_VJP_HD
#endif

namespace sipamd {
namespace tree_vjp {

// code of a word: the factor s of the pair form, or the copy
enum : uint32_t { kOne = 0, kHalf = 1, kMinusHalf = 2, kCopy = 3 };

// 8 bytes per input-arena scalar: ia, then ib in the low 30 bits with the code above them.
struct Word {
  uint32_t a, b;
};
constexpr long kMaxOutputLen = 1L << 30; // ib has 30 bits
constexpr long kMaxInputLen = 0x7fffffffL; // a run of entries is counted in an int

SIP_TREE_VJP_HD inline uint32_t word_ia(const Word w) { return w.a; }
SIP_TREE_VJP_HD inline uint32_t word_ib(const Word w) { return w.b & 0x3fffffffu; }
SIP_TREE_VJP_HD inline uint32_t word_code(const Word w) { return w.b >> 30; }
inline Word make_word(const long ia, const long ib, const uint32_t code) {
  return {(uint32_t)ia, (uint32_t)ib | (code << 30)};
}

// The table of a plan with the tree-native layout (GenericPlan::layout_tree_native): in0_len words.  Empty where the
// arenas are beyond what a word or a run can count (no launch is possible then).
template <class Plan>
std::vector<Word> build_table(const Plan &g) {
  if (g.out_len > kMaxOutputLen || g.in0_len > kMaxInputLen)
    return {};
  std::vector<Word> t((size_t)g.in0_len, Word{0, 0});
  // a rows x cols block at `at`, column-major: entry (r, col) pairs row place ra + r with column place cb + col
  auto block = [&](const long at, const long rows, const long cols, const long ra, const long cb, const uint32_t code) {
    for (long col = 0; col < cols; ++col)
      for (long r = 0; r < rows; ++r)
        t[(size_t)(at + r + rows * col)] = make_word(ra + r, cb + col, code);
  };
  auto diagonal = [&](const long at, const long len, const long place, const uint32_t code) {
    for (long j = 0; j < len; ++j)
      t[(size_t)(at + j)] = make_word(place + j, place + j, code);
  };
  for (int i = 0; i < g.N; ++i) {
    const long n = g.state_dims[i], x = g.ox[i], y = g.oy[i];
    block(g.oQ[i], n, n, x, x, kHalf);
    diagonal(g.oq[i], n, x, kCopy);
    diagonal(g.oc[i], n, y, kCopy);
    diagonal(g.od[i], n, y, kMinusHalf);
  }
  for (int e = 0; e < g.E; ++e) {
    const int p = g.parents[e], c = g.children[e];
    const long np = g.state_dims[p], nc = g.state_dims[c], m = g.control_dims[e], u = g.ou[e];
    block(g.oA[e], nc, np, g.oy[c], g.ox[p], kOne);
    block(g.oB[e], nc, m, g.oy[c], u, kOne);
    block(g.oM[e], np, m, g.ox[p], u, kOne);
    block(g.oR[e], m, m, u, u, kHalf);
    diagonal(g.orr[e], m, u, kCopy);
  }
  return t;
}

// ---- the launch shape ------------------------------------------------------------------------------------------------
constexpr int kLanes = 64;
constexpr int kMaxWaves = 8;              // wavefronts of a workgroup, at the most, and the default
constexpr size_t kLdsBudget = 64 * 1024;  // dynamic LDS a launch may ask for without raising the kernel's limit
constexpr int kPiece = 2;                 // doubles of a 16-byte piece
// A problem is split into several runs only where one workgroup per problem would leave compute units idle: a batch
// below the compute units of the device the kernel is written for, and then no run shorter than kMinRun entries (what
// 8 wavefronts store in 4 pieces per lane).
constexpr long kComputeUnits = 256;
constexpr long kMinRun = (long)kMaxWaves * kLanes * kPiece * 4;
constexpr long kMaxRuns = 65535; // gridDim.y

struct Shape {
  bool staged = false; // z and lambda of a problem go through LDS as pairs (else they are read in place)
  int waves = 0;       // 0: nothing to launch (an empty input arena)
  long run = 0;        // entries of the input arena per workgroup
  long runs = 0;       // workgroups per problem
  size_t lds_bytes = 0;
};

// waves, run: 0 for the default, else what SIP_LQR_TREE_VJP_SHAPE asks for (cut to what is possible).
inline Shape launch_shape(const long in_len, const long out_len, const long batch, int waves = 0, long run = 0) {
  Shape s;
  s.staged = (size_t)out_len * 16 <= kLdsBudget;
  if (in_len < 1 || batch < 1)
    return s;
  if (run < 1) {
    long runs = 1;
    if (batch < kComputeUnits) {
      const long idle = (kComputeUnits + batch - 1) / batch, most = (in_len + kMinRun - 1) / kMinRun;
      runs = idle < most ? idle : most;
    }
    run = (in_len + runs - 1) / runs;
  }
  run = run > in_len ? in_len : run;
  if ((in_len + run - 1) / run > kMaxRuns)
    run = (in_len + kMaxRuns - 1) / kMaxRuns;
  run = (run + kPiece - 1) / kPiece * kPiece; // whole pieces, so that a run starts where the pieces of the arena do
  s.run = run;
  s.runs = (in_len + run - 1) / run;
  waves = waves < 1 || waves > kMaxWaves ? kMaxWaves : waves;
  const long pieces = (run + kPiece - 1) / kPiece + 1, fill = (pieces + kLanes - 1) / kLanes;
  s.waves = (int)(fill < waves ? fill : waves); // no more wavefronts than have a piece to store
  s.lds_bytes = s.staged ? (size_t)out_len * 16 : 0;
  return s;
}

inline const char *kernel_name(const Shape &s) { return s.staged ? "tree_vjp<staged>/f64" : "tree_vjp<direct>/f64"; }

} // namespace tree_vjp
} // namespace sipamd
