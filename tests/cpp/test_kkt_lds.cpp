// The derived sizes and LDS partitions of the Newton-KKT chain kernels (csrc/kkt_chain_kernels.hpp,
// kkt_theta_chain_kernels.hpp), checked on the host: the kernels take their LDS pointers, and sip_kkt_amd.hip the
// bytes of every launch, from the same descriptions, so what holds here holds for both.  Needs no device.
//
// Build (also done by __graft_entry__.build()):
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 tests/cpp/test_kkt_lds.cpp -o build/test_kkt_lds
#define SIP_KKT_CHAIN_UNIT // the structs and descriptions only: none of the kernels that are no templates
#include "../../sip_optimal_control_amd/csrc/kkt_chain_launch.hpp"

#include <cstdio>
#include <initializer_list>

using namespace sipamd::kkt;

namespace {

constexpr ChainKkt primaries(int n, int m, int cn, int gn, int cT, int gT, int ce, int ge, int split, int sym) {
  ChainKkt ck{};
  ck.n = n, ck.m = m, ck.T = 7, ck.cn = cn, ck.gn = gn, ck.cT = cT, ck.gT = gT, ck.ce = ce, ck.ge = ge;
  ck.split = split, ck.sym = sym;
  return ck;
}

// (c) family_dims<FN, FM> yields what the derivation gives for the family's primaries, in every layout
constexpr bool same(const ChainKkt &a, const ChainKkt &b) {
  return a.n == b.n && a.m == b.m && a.T == b.T && a.cn == b.cn && a.gn == b.gn && a.cT == b.cT && a.gT == b.gT &&
         a.ce == b.ce && a.ge == b.ge && a.node_len == b.node_len && a.edge_len == b.edge_len &&
         a.mats_stage == b.mats_stage && a.vecs_stage == b.vecs_stage && a.lds_item == b.lds_item &&
         a.lds_tail == b.lds_tail && a.lds_rows == b.lds_rows && a.split == b.split && a.sym == b.sym;
}
template <int FN, int FM>
constexpr bool family_agrees() {
  for (int layout = 0; layout < 3; ++layout) { // full, split, split + packed
    const int split = layout > 0, sym = layout > 1;
    ChainKkt in{}; // what a plan of other dimensions would hand the kernel: all of it is overwritten but T and the layout
    in.n = 31, in.m = 17, in.T = 7, in.cn = 3, in.gn = 5, in.cT = 1, in.gT = 9, in.ce = 4, in.ge = 2;
    in.split = split, in.sym = sym;
    const int c = family_c(FN), g = family_g(FM);
    if (!same(family_dims<FN, FM>(in), chain_kkt_derive(primaries(FN, FM, 0, 0, c, g, c, g, split, sym))))
      return false;
  }
  return true;
}
#define CHECK_FAMILY_SHAPE(N, M) static_assert(family_agrees<N, M>(), "family_dims<" #N ", " #M ">");
#define CHECK_FAMILY_N(N) SIP_KKT_FAMILY_SHAPES(CHECK_FAMILY_SHAPE, N)
SIP_KKT_FAMILY_N(CHECK_FAMILY_N)
static_assert(same(family_dims<0, 0>(primaries(5, 3, 1, 2, 3, 2, 2, 3, 0, 0)), primaries(5, 3, 1, 2, 3, 2, 2, 3, 0, 0)),
              "the generic instantiation takes the plan's ChainKkt as it is");

int failures = 0;
void expect(const bool ok, const char *what, const int row, const long got, const long want) {
  if (!ok) {
    std::printf("[FAILED] row %d: %s: got %ld, expected %ld\n", row, what, got, want);
    ++failures;
  }
}

// (a) a partition is a row of regions of the given lengths, each starting where the one before it ends: no region
// shorter than what the kernel keeps in it (`needs`, same order), and total() the end of the last one.
// (b) `even_start`: bit k set = region k is read or written in 16-byte pieces and so has to start on an even double.
void expect_partition(const char *what, const int row, std::initializer_list<long> lengths,
                      std::initializer_list<long> needs, const long total, const unsigned even_start) {
  long at = 0;
  int k = 0;
  auto need = needs.begin();
  for (const long len : lengths) {
    expect(len >= *need && len >= 0, what, row, len, *need);
    if (even_start >> k & 1)
      expect((at & 1) == 0, what, row, at, at & ~1L);
    at += len, ++k, ++need;
  }
  expect(at == total, what, row, total, at);
}

// (d) bytes of every launch, worked by hand from the formulas the host used before the descriptions existed:
//   lds_item = even(n n + cgn n + edge_len), lds_tail = even(cgn n + cge (n + m)), lds_rows = even(cgn + cge) with
//   cgn = max(cn + gn, cT + gT), cge = ce + ge;  condense = 8 (lds_item + 2 lds_rows + even(n + m) + mats_stage);
//   rhs(k columns) = 8 (lds_tail + 2 lds_rows) + 8 lds_rows (k - 1);  recover(k) = 8 (lds_tail + n + m) + 8 (n + m) (k - 1);
//   apply = 8 (lds_item + 3 n + m + lds_rows);  theta item = even(max(node + edge, (n + cT + gT + p) p));
//   theta_rhs = 8 (lds_tail + item + R + p R);  theta_recover = 8 (lds_tail + item + p (n + m) + p n + p R + R);
//   theta_dot = 8 (item + 2 n + m + R);  apply_theta per wavefront = 8 (item + even(2 n + m) + R + 2 even(p));
//   wavefronts = max(1, min(8, 65536 / per wavefront, N));  columns per launch = 1 + min(p - 1, (65536 - one) / each)
struct Row {
  int d[8]; // n, m, cn, gn, cT, gT, ce, ge
  int p, ncols, nodes;
  int lds_item, lds_tail, lds_rows;
  long condense, condense_split, condense_packed, rhs_1, rhs_n, recover_1, recover_n, apply;
  int theta_item;
  long theta_rhs, theta_recover, theta_dot, apply_theta_wave;
  int apply_waves, rhs_cols, recover_cols;
};
const Row rows[] = {
    {{12, 4, 0, 0, 6, 8, 6, 8}, 8, 1, 51, 936, 392, 28, 11360, 9824, 9248, 3584, 3584, 3264, 3264, 8032, 560, 9632, 11424, 4928, 5056, 8, 8, 8},
    {{12, 4, 0, 0, 6, 8, 6, 8}, 13, 2, 51, 936, 392, 28, 11360, 9824, 9248, 3584, 3808, 3264, 3392, 8032, 1040, 14592, 17504, 8768, 8992, 7, 13, 13},
    // more columns than one launch of the right-hand-side kernel holds; a theta item beyond LDS (one wavefront)
    {{12, 4, 0, 0, 6, 8, 6, 8}, 300, 5, 51, 936, 392, 28, 11360, 9824, 9248, 3584, 4480, 3264, 3776, 8032, 196200, 1640160, 1707360, 1570048, 1574848, 1, 277, 300},
    // odd n, m, theta_dim, constraints at interior nodes too
    {{5, 3, 1, 2, 3, 2, 2, 3}, 3, 2, 8, 180, 66, 10, 2416, 2096, 1992, 688, 768, 592, 656, 1664, 96, 1616, 1928, 952, 1024, 8, 3, 3},
    // the smallest family shape, fewer nodes than wavefronts
    {{4, 1, 0, 0, 2, 2, 2, 2}, 4, 4, 3, 94, 36, 8, 1288, 1128, 1080, 416, 608, 328, 448, 920, 100, 1408, 1696, 936, 1008, 3, 4, 4},
    // interior nodes with more rows than the terminal one, no equality rows on the edges
    {{7, 2, 3, 4, 1, 0, 0, 5}, 5, 3, 2, 274, 94, 12, 3560, 3056, 2880, 944, 1136, 824, 968, 2472, 226, 3136, 3776, 2032, 2128, 2, 5, 5},
    // beyond the 48 KiB of the chain kernels; more columns than one launch of the recovery holds
    {{32, 8, 0, 0, 16, 16, 16, 16}, 33, 2, 11, 5952, 2304, 64, 70208, 59968, 55776, 19456, 19968, 18752, 19072, 48960, 6666, 89168, 108176, 54416, 54960, 1, 33, 33},
    {{32, 32, 0, 0, 4, 4, 4, 4}, 200, 3, 5, 6912, 768, 16, 97280, 80896, 72960, 6400, 6656, 6656, 7680, 56448, 107200, 889472, 1043072, 858496, 861696, 1, 200, 116},
};

void check_row(const int r, const Row &w) {
  const int *d = w.d;
  const ChainKkt full = chain_kkt_derive(primaries(d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], 0, 0));
  const ChainKkt split = chain_kkt_derive(primaries(d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], 1, 0));
  const ChainKkt packed = chain_kkt_derive(primaries(d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], 1, 1));
  ChainTheta ct{};
  ct.p = w.p;
  ct = chain_theta_derive(full, ct);
  expect(full.lds_item == w.lds_item, "lds_item", r, full.lds_item, w.lds_item);
  expect(full.lds_tail == w.lds_tail, "lds_tail", r, full.lds_tail, w.lds_tail);
  expect(full.lds_rows == w.lds_rows, "lds_rows", r, full.lds_rows, w.lds_rows);
  expect(ct.lds_item == w.theta_item, "theta lds_item", r, ct.lds_item, w.theta_item);
  expect(chain_mats_len(full) == 7L * full.mats_stage + d[0] * d[0] + d[0], "mats_len", r, chain_mats_len(full), 0);
  expect(chain_mats_len(packed) == 7L * packed.mats_stage + d[0] * (d[0] + 1) / 2 + d[0], "mats_len, packed", r,
         chain_mats_len(packed), 0);

  auto bytes = [&](const char *what, const size_t got, const long want) { expect((long)got == want, what, r, (long)got, want); };
  bytes("condense, full mats", lds_bytes(condense_lds(full, true, 1)), w.condense);
  bytes("condense, split", lds_bytes(condense_lds(split, true, 1)), w.condense_split);
  bytes("condense, split + packed", lds_bytes(condense_lds(packed, true, 1)), w.condense_packed);
  bytes("rhs, one column", lds_bytes(condense_lds(full, false, 1)), w.rhs_1);
  bytes("rhs, columns", lds_bytes(condense_lds(full, false, w.ncols)), w.rhs_n);
  bytes("recover, one column", lds_bytes(recover_lds(full, 1)), w.recover_1);
  bytes("recover, columns", lds_bytes(recover_lds(full, w.ncols)), w.recover_n);
  bytes("apply", lds_bytes(apply_lds(full)), w.apply);
  bytes("theta_rhs", lds_bytes(theta_rhs_lds(full, ct)), w.theta_rhs);
  bytes("theta_recover", lds_bytes(theta_recover_lds(full, ct)), w.theta_recover);
  bytes("theta_dot", lds_bytes(theta_dot_lds(full, ct)), w.theta_dot);
  bytes("apply_theta, one wavefront", lds_bytes(apply_theta_lds(full, ct, 1)), w.apply_theta_wave);
  bytes("apply_theta, three wavefronts", lds_bytes(apply_theta_lds(full, ct, 3)), 3 * w.apply_theta_wave);
  // what fits in 64 KiB, asked as sip_kkt_amd.hip asks
  const int fit = lds_count_that_fits(apply_theta_lds(full, ct, 1), APPLY_THETA_MAX_WAVES);
  const int waves = fit < w.nodes ? fit : w.nodes;
  expect(waves == w.apply_waves, "apply_theta wavefronts", r, waves, w.apply_waves);
  const int rhs_cols = lds_count_that_fits(condense_lds(full, false, 1), w.p);
  expect(rhs_cols == w.rhs_cols, "rhs columns per launch", r, rhs_cols, w.rhs_cols);
  const int rec_cols = lds_count_that_fits(recover_lds(full, 1), w.p);
  expect(rec_cols == w.recover_cols, "recover columns per launch", r, rec_cols, w.recover_cols);

  const int n = d[0], m = d[1], P = w.p;
  const int rows_max = (d[2] + d[3] > d[4] + d[5] ? d[2] + d[3] : d[4] + d[5]) + d[6] + d[7]; // of a stage
  const int tail_max = (d[2] + d[3] > d[4] + d[5] ? d[2] + d[3] : d[4] + d[5]) * n + (d[6] + d[7]) * (n + m);
  for (const ChainKkt &ck : {full, split, packed}) {
    for (const int ncols : {1, w.ncols}) {
      // image (16-byte copies, the pipelined kernel's register -> LDS stores) | weights | weighted rows (dot_seq reads
      // both in pairs) | r1 of the stage | the block of mats
      const CondenseLds c = condense_lds(ck, true, ncols), v = condense_lds(ck, false, ncols);
      expect_partition("condense", r, {c.buf, c.wl, c.wr, c.r1s, c.obuf},
                       {ck.node_len + ck.edge_len, rows_max, rows_max, n + m, ck.mats_stage}, c.total(), 0x17);
      expect_partition("rhs", r, {v.buf, v.wl, v.wr}, {tail_max, rows_max, (long)ncols * ck.lds_rows}, v.total(), 0x7);
      expect(v.each == ck.lds_rows && condense_lds(ck, false, ncols + 1).total() - v.total() == v.each,
             "rhs: doubles per column", r, v.each, ck.lds_rows);
      const RecoverLds rc = recover_lds(ck, ncols);
      expect_partition("recover", r, {rc.jn, rc.xs}, {tail_max, ncols * (n + m)}, rc.total(), 0x1);
      expect(recover_lds(ck, ncols + 1).total() - rc.total() == rc.each, "recover: doubles per column", r, rc.each, n + m);
    }
    const ApplyLds ap = apply_lds(ck); // image | x_i | u_i | ydyn_i | ydyn_{i+1} | the constraint rows of a stage
    expect_partition("apply", r, {ap.buf, ap.v}, {ck.node_len + ck.edge_len, 3 * n + m + rows_max}, ap.total(), 0x1);
  }
  // the Jacobians and the theta item arrive as 16-byte copies
  const int item = ct.node_len + ct.edge_len > (n + d[4] + d[5] + P) * P ? ct.node_len + ct.edge_len : (n + d[4] + d[5] + P) * P;
  const ThetaRhsLds tr = theta_rhs_lds(full, ct);
  expect_partition("theta_rhs", r, {tr.jn, tr.th, tr.wl, tr.wr}, {tail_max, item, rows_max, P * full.lds_rows}, tr.total(), 0x3);
  const ThetaRecoverLds tc = theta_recover_lds(full, ct);
  expect_partition("theta_recover", r, {tc.jn, tc.th, tc.xs, tc.ys, tc.ms, tc.wl},
                   {tail_max, item, P * (n + m), P * n, P * full.lds_rows, rows_max}, tc.total(), 0x3);
  const ThetaDotLds td = theta_dot_lds(full, ct);
  expect_partition("theta_dot", r, {td.th, td.vx, td.vd, td.vr}, {item, n + m, n, rows_max}, td.total(), 0x1);
  // one wavefront's part: x_i | u_i and the dynamics rows share the padded region vxd; every part starts like the first
  const ApplyThetaLds at = apply_theta_lds(full, ct, 2);
  expect_partition("apply_theta", r, {at.th, at.vxd, at.vr, at.tv, at.yacc}, {item, 2 * n + m, rows_max, P, P}, at.each, 0x1);
  expect(at.vx == n + m && at.vxd - at.vx >= n, "apply_theta: dynamics rows", r, at.vxd - at.vx, n);
  expect((at.each & 1) == 0 && at.total() == 2 * at.each, "apply_theta: wavefront parts", r, at.total(), 2 * at.each);
}

} // namespace

int main() {
  int r = 0;
  for (const Row &w : rows)
    check_row(r++, w);
  std::printf("%d rows, %d failures\n", r, failures);
  return failures == 0 ? 0 : 1;
}
