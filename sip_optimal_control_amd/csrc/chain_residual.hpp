// chain_residual.hpp -- the residual of the chain KKT system on the packed chain layout (include/sip_lqr_amd.h), in
// fp64, for NC right-hand sides and iterates against one `mats`, and the update of the iterative refinement built on
// it (sip_lqr_residual, sip_lqr_refine: one column; sip_lqr_residual_multi, sip_lqr_refine_multi: several, laid out as
// sip_lqr_solve_multi lays its columns out, column c of a whole-batch array at c * col_stride scalars).  One kernel
// template serves both: the single-column entry points launch its NC = 1 instantiation.
//
//   rho_q[i] = Q_i x_i - y_i + q_i  (+ M_i u_i + A_i^T y_{i+1}           if i < T)
//   rho_c[0] = -x_0 - delta_0 o y_0 + c_0
//   rho_c[i] = A_{i-1} x_{i-1} + B_{i-1} u_{i-1} - x_i - delta_i o y_i + c_i     (i >= 1)
//   rho_r[i] = M_i^T x_i + R_i u_i + B_i^T y_{i+1} + r_i                  (i < T)
//
// in the vecs layout (slot q_i, slot c_i, slot r_i): a solve whose right-hand side is rho returns d with
// K (z + d) + b = 0.
//
// Shape: one workgroup per problem, its wavefronts taking stages in turn (no recursion ties the stages).  The wavefront
// of stage i computes what reads stage i's blocks -- rho_q[i], rho_r[i] and rho_c[i + 1] (stage 0: rho_c[0] too) -- so
// every block of `mats` is fetched once: one contiguous image [Q | delta | A | B | M | R] by 16-byte loads into LDS,
// from the piece that holds the stage's first scalar (the transposed products A^T y, B^T y, M^T x then read columns out
// of LDS, not out of memory).  Next to it, per wavefront (residual_cols_shape.hpp), the LDS holds as doubles
//   z[k][c]  k over x_i | y_i | u_i | x_{i+1} | y_{i+1},  e[k][c]  k over q_i | r_i | c_{i+1},  delta_{i+1}[k]
// with the NC columns of one entry adjacent: a term's NC operands are one or more 16-byte LDS reads.  The gather deals
// (k, c) pairs to lanes with c fastest, so that its LDS writes are contiguous.
// A wavefront that waits for one load at a time is bound by the latency of memory, not by its rate: the loads of a
// stage are issued kCopyUnroll (image) and kGatherUnroll (vectors) per lane before the first of them is waited for, and
// nothing after the staging reads memory.  A stage image that does not fit the LDS budget (or a `mats` that is not
// 16-byte aligned) is read in place instead (STAGED = false).
//
// Every row of the three results is one dot product against z; kParts lanes share a row, each taking its terms in
// order through the same three segments, and their partial sums meet by two shuffle adds.  A lane loads a matrix entry
// once, widens it once (fp32 blocks: exact) and issues NC fp64 FMAs into NC accumulators; what the kernel is otherwise
// bound by (addresses, per-row descriptors, loop control) does not depend on the right-hand side.  After
// the shuffles the kParts lanes of a row hold the same sums; lane `part` closes and stores the columns c with
// c % kParts == part, by (acc - y) + q, acc + r, fma(-delta, y, acc - x) + c and fma(-delta_0, y_0, -x_0) + c_0.
// Column c is the same bits whatever NC it is computed at.
//
// A launch of the NC instantiation may carry ncols < NC columns: a masked column reads the last real column again
// (in bounds, and no branch among the loads) and stores nothing.
//
// The max-norm of a problem and column stays in its workgroup: lanes, then wavefronts through LDS; max is
// order-independent, so the result is deterministic.  The scaled form needs the norm before it can store anything: it
// walks the stages twice (norm, then rho / s), the second walk served by the caches (a problem's mats are 83 KB at
// n = 12, m = 4, T = 50 in fp32).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "residual_cols_shape.hpp"

namespace sipamd {
namespace residual {

constexpr int kLanes = 64;
constexpr int kParts = 4;        // lanes per row of the result; divides kLanes, so a row's lanes share a wavefront
constexpr int kCopyUnroll = 8;   // 16-byte pieces of the stage image a lane has in flight
constexpr int kGatherUnroll = 4; // vector entries a lane has in flight
constexpr int kDotUnroll = 4;    // terms of a dot product a lane reads out of LDS before it uses the first

// Offsets, in scalars, inside one stage of `mats` and the strides of the three per-problem arrays.
struct Dims {
  int n, m, T;
  int oD, oA, oB, oM, oR; // Q is at 0
  int node, stg;          // [Q | delta], [Q | delta | A | B | M | R]
  int vstg;               // 2 n + m: stage stride of vecs / sol
  int sym;                // Q, R as lower triangles packed by columns
  long mats_len, vecs_len;
};

inline Dims make_dims(int n, int m, int T, bool sym) {
  Dims d;
  d.n = n, d.m = m, d.T = T, d.sym = sym ? 1 : 0;
  const int nq = sym ? n * (n + 1) / 2 : n * n, nr = sym ? m * (m + 1) / 2 : m * m;
  d.oD = nq;
  d.node = d.oA = nq + n;
  d.oB = d.oA + n * n;
  d.oM = d.oB + n * m;
  d.oR = d.oM + n * m;
  d.stg = d.oR + nr;
  d.vstg = 2 * n + m;
  d.mats_len = (long)T * d.stg + d.node;
  d.vecs_len = (long)T * d.vstg + 2 * n;
  return d;
}

// max that keeps a NaN once it has seen one
__device__ __forceinline__ double nan_max(const double a, const double b) { return (b > a || b != b) ? b : a; }

// The scale of a refinement round: the power of two with s <= norm < 2 s; 1 for a norm that is 0 or not finite.
__device__ __forceinline__ double pow2_scale(const double norm) {
  return (norm > 0.0 && norm < __builtin_huge_val()) ? ldexp(1.0, ilogb(norm)) : 1.0;
}

// (row, col) of a lower triangle packed by columns, row >= col
__device__ __forceinline__ int tri(const int row, const int col, const int dim) {
  return col * dim - col * (col - 1) / 2 + (row - col);
}

// LDS instructions of one wavefront execute in order; this keeps the compiler from moving them across the point.
__device__ __forceinline__ void lds_order() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Terms of a dot product a lane reads out of LDS before it uses the first: NC accumulators and kDotUnroll x NC staged
// z values (two VGPRs each) do not fit next to the rest at NC = 8.
template <int NC>
constexpr int cols_dot_unroll() {
  return NC >= 8 ? 2 : kDotUnroll;
}

// out[c] = p[c], c < NC; p is 16-byte aligned for NC >= 2
template <int NC>
__device__ __forceinline__ void load_cols(const double *p, double (&out)[NC]) {
  if constexpr (NC == 1) {
    out[0] = p[0];
  } else {
#pragma unroll
    for (int c = 0; c < NC; c += 2) {
      const double2 t = *(const double2 *)(p + c);
      out[c] = t.x, out[c + 1] = t.y;
    }
  }
}

// S: scalar of mats and of the scaled output; V: scalar of vecs and sol (S, or double: the wide form).  vecs, sol, res
// and scaled point at column 0 of the launch, column c at c * col_stride scalars; norm and scale at column 0, column c
// at c * batch.  res != nullptr or scaled == nullptr: plain form (res may be nullptr: norms only); scaled != nullptr:
// scaled form, one scale per problem and column.
template <typename S, typename V, bool STAGED, int NC>
__global__ void __launch_bounds__(kLanes *kColsMaxWaves)
    chain_residual_kernel(const Dims d, const S *__restrict__ mats, const V *__restrict__ vecs,
                          const V *__restrict__ sol, const long launch_col_stride, const long batch,
                          const int launch_ncols, double *__restrict__ res, S *__restrict__ scaled,
                          double *__restrict__ scale, double *__restrict__ norm, const int wave_bytes) {
  static_assert(NC == 1 || NC == 2 || NC == 4 || NC == 8, "columns of an instantiation");
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  constexpr int LOG = NC == 1 ? 0 : (NC == 2 ? 1 : (NC == 4 ? 2 : 3));
  constexpr int DU = cols_dot_unroll<NC>();
  // One column: there is one column and no stride to it, known at compile time, so the clamps to the last column, the
  // products with the stride and the tests against ncols below are folded away.
  const int ncols = NC == 1 ? 1 : launch_ncols;
  const long col_stride = NC == 1 ? 0 : launch_col_stride;
  const int n = d.n, m = d.m, T = d.T, vstg = d.vstg;
  const long p = blockIdx.x;
  // (the wavefront's number through readfirstlane: the compiler then knows that it, the stage and everything that
  // follows from them is the same in every lane, and keeps it in scalar registers and scalar branches)
  const int lane = threadIdx.x & (kLanes - 1), wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kLanes);
  const int waves = blockDim.x / kLanes;
  double *red = (double *)lds;
  unsigned char *mine = lds + cols_red_bytes(NC) + (size_t)wave * wave_bytes;
  double *z = (double *)mine;                      // z[k][c]
  double *e = z + (size_t)NC * (4 * n + m);        // e[k][c]
  double *dl = e + (size_t)NC * (2 * n + m);       // delta_{i+1}[k]
  S *img = (S *)(mine + cols_z_doubles(n, m, NC) * sizeof(double));
  const S *pm = mats + p * d.mats_len;
  const V *pv = vecs + p * d.vecs_len, *ps = sol + p * d.vecs_len; // column 0
  constexpr int PIECE = 16 / (int)sizeof(S); // scalars per 16-byte piece
  const int part = lane & (kParts - 1);
  const int last_col = ncols - 1;

  const int passes = scaled != nullptr ? 2 : 1;
  double s_pc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c)
    s_pc[c] = 1.0;
  for (int pass = 0; pass < passes; ++pass) {
    const bool want_norm = pass == 0, store = pass == passes - 1;
    double nrm[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c)
      nrm[c] = 0.0;
    // (c is a constant wherever this is called: the loops over columns are unrolled)
    auto emit = [&](const int c, const int idx, const double v) {
      if (want_norm)
        nrm[c] = nan_max(nrm[c], __builtin_fabs(v));
      if (store) {
        const long at = c * col_stride + p * d.vecs_len + idx;
        if (scaled != nullptr)
          scaled[at] = (S)(v / s_pc[c]);
        else if (res != nullptr)
          res[at] = v;
      }
    };
    for (int i = wave; i <= T; i += waves) {
      const bool edge = i < T;
      const long v0 = (long)i * vstg; // stage i in vecs / sol
      lds_order();                    // the previous stage's reads of z and the image are done
      // Item t = k * NC + c of a list is entry k of column c, and lands at [t]: lanes write LDS contiguously.  A lane
      // past the end of a list loads and stores the list's last item again: in bounds, the same value to the same
      // place, and no branch between the loads and the stores, which would leave one load in flight at a time.  A
      // masked column reads the last column.
      const int zl = (edge ? 4 * n + m : 2 * n) << LOG, el = (edge ? 2 * n + m : n) << LOG;
      const S *delta_src = pm + (long)(edge ? i + 1 : i) * d.stg + d.oD; // (the last stage has no use for it)
      for (int base = 0; base < zl; base += kLanes * kGatherUnroll) {   // zl >= el, n
        double rz[kGatherUnroll], re[kGatherUnroll], rd[kGatherUnroll];
        int tz[kGatherUnroll], te[kGatherUnroll], kd[kGatherUnroll];
#pragma unroll
        for (int j = 0; j < kGatherUnroll; ++j) {
          const int t = base + j * kLanes + lane;
          tz[j] = t < zl ? t : zl - 1, te[j] = t < el ? t : el - 1, kd[j] = t < n ? t : n - 1;
          const int cz = tz[j] & (NC - 1), ce = te[j] & (NC - 1), ke = te[j] >> LOG;
          rz[j] = (double)ps[(cz < last_col ? cz : last_col) * col_stride + v0 + (tz[j] >> LOG)];
          // q_i, r_i: slots 0 and 2 of stage i; c_{i+1}: slot 1 of stage i + 1
          re[j] = (double)pv[(ce < last_col ? ce : last_col) * col_stride + v0 + ke +
                             (ke < n ? 0 : (ke < n + m ? n : 2 * n))];
          rd[j] = (double)delta_src[kd[j]];
        }
#pragma unroll
        for (int j = 0; j < kGatherUnroll; ++j)
          z[tz[j]] = rz[j], e[te[j]] = re[j], dl[kd[j]] = rd[j];
      }
      const S *stage = pm + (long)i * d.stg;
      const int len = edge ? d.stg : d.node;
      const S *blk; // element e of the stage is blk[e]
      if constexpr (STAGED) {
        const int lead = (int)(((uintptr_t)stage & 15) / sizeof(S));
        const S *from = stage - lead; // 16-byte aligned, inside the buffer: mats itself is aligned
        const int total = lead + len, pieces = total / PIECE;
        for (int base = 0; base < pieces; base += kLanes * kCopyUnroll) { // (as above for a lane past the end)
          uint4 r[kCopyUnroll];
          int k[kCopyUnroll];
#pragma unroll
          for (int j = 0; j < kCopyUnroll; ++j) {
            k[j] = base + j * kLanes + lane < pieces ? base + j * kLanes + lane : pieces - 1;
            r[j] = ((const uint4 *)from)[k[j]];
          }
#pragma unroll
          for (int j = 0; j < kCopyUnroll; ++j)
            ((uint4 *)img)[k[j]] = r[j];
        }
        for (int k = pieces * PIECE + lane; k < total; k += kLanes) // what is left of the last piece: never past the end
          img[k] = from[k];
        blk = img + lead;
      } else {
        blk = stage;
      }
      lds_order();

      // rows [0, n) rho_q[i] | [n, n + m) rho_r[i] | [n + m, 2n + m) rho_c[i + 1]; the last stage has the first n only.
      // Every row is three segments against x_i (n terms), u_i (m) and y_{i+1} (n): only where a segment's matrix
      // entries start and how far apart they lie differs from row to row, so the lanes of a wavefront walk the same
      // loops whatever rows they hold.  A term is one matrix entry against the NC columns of z[kk]; DU terms of a lane
      // are loaded before the first is used.
      auto segment = [&](auto TRI, double(&acc)[NC], const int base, const int stride, const int count, const int zoff,
                         const bool tri_lane, const int r, const int dim) {
        for (int k = part; k < count; k += kParts * DU) {
          S a[DU];
          double zz[DU][NC];
#pragma unroll
          for (int j = 0; j < DU; ++j) {
            const int kk = k + j * kParts < count ? k + j * kParts : k; // past the end: the first term again, unused
            int at = base + stride * kk;
            if constexpr (decltype(TRI)::value)
              at = tri_lane ? base + (kk < r ? tri(r, kk, dim) : tri(kk, r, dim)) : at;
            a[j] = blk[at];
            load_cols<NC>(z + ((size_t)(zoff + kk) << LOG), zz[j]);
          }
#pragma unroll
          for (int j = 0; j < DU; ++j) {
            const bool on = k + j * kParts < count;
            const double aj = (double)a[j];
#pragma unroll
            for (int c = 0; c < NC; ++c)
              acc[c] = on ? __builtin_fma(aj, zz[j][c], acc[c]) : acc[c];
          }
        }
      };
      const int rows = edge ? 2 * n + m : n, items = rows * kParts;
      for (int w0 = 0; w0 < items; w0 += kLanes) {
        const int w = w0 + lane;
        const bool active = w < items;
        const int row = w / kParts;
        const bool q_row = row < n, r_row = !q_row && row < n + m;
        const int j = row - n, r = row - n - m; // the row inside rho_r, inside rho_c
        // (base, stride) of the row in: Q | M^T | A;  M | R | B;  A^T | B^T | nothing
        const int b0 = q_row ? row : (r_row ? d.oM + n * j : d.oA + r), s0 = r_row ? 1 : n;
        const int b1 = q_row ? d.oM + row : (r_row ? d.oR + j : d.oB + r), s1 = r_row ? m : n;
        const int b2 = q_row ? d.oA + n * row : d.oB + n * j;
        const int c0 = active ? n : 0, c1 = active && edge ? m : 0, c2 = active && edge && (q_row || r_row) ? n : 0;
        double acc[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c)
          acc[c] = 0.0;
        if (d.sym) { // Q (rho_q) and R (rho_r) are packed triangles: Q at 0, R at oR
          segment(std::true_type{}, acc, q_row ? 0 : b0, s0, c0, 0, q_row, row, n);
          segment(std::true_type{}, acc, r_row ? d.oR : b1, s1, c1, 2 * n, r_row, j, m);
        } else {
          segment(std::false_type{}, acc, b0, s0, c0, 0, false, 0, 0);
          segment(std::false_type{}, acc, b1, s1, c1, 2 * n, false, 0, 0);
        }
        segment(std::false_type{}, acc, b2, 1, c2, 3 * n + m, false, 0, 0);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          acc[c] += __shfl_xor(acc[c], 1);
          acc[c] += __shfl_xor(acc[c], 2);
        }
        if (active) {
#pragma unroll
          for (int c = 0; c < NC; ++c) {
            if ((c & (kParts - 1)) != part || c >= ncols)
              continue;
            if (row < n) {
              emit(c, (int)v0 + row, (acc[c] - z[((n + row) << LOG) + c]) + e[(row << LOG) + c]);
            } else if (row < n + m) {
              emit(c, (int)v0 + row + n, acc[c] + e[(row << LOG) + c]); // slot r_i starts at 2n
            } else {
              const double t =
                  __builtin_fma(-dl[r], z[((3 * n + m + r) << LOG) + c], acc[c] - z[((2 * n + m + r) << LOG) + c]);
              emit(c, (int)v0 + vstg + n + r, t + e[((n + m + r) << LOG) + c]);
            }
          }
        }
      }
      if (i == 0)
        for (int r = lane; r < n; r += kLanes) {
          const double d0 = (double)blk[d.oD + r];
#pragma unroll
          for (int c = 0; c < NC; ++c)
            if (c < ncols)
              emit(c, n + r,
                   __builtin_fma(-d0, z[((n + r) << LOG) + c], -z[(r << LOG) + c]) +
                       (double)pv[c * col_stride + n + r]);
        }
    }
    if (want_norm) {
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        for (int off = kLanes / 2; off > 0; off >>= 1)
          nrm[c] = nan_max(nrm[c], __shfl_xor(nrm[c], off));
        if (lane == 0)
          red[wave * NC + c] = nrm[c];
      }
      __syncthreads();
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        double all = red[c];
        for (int k = 1; k < waves; ++k)
          all = nan_max(all, red[k * NC + c]);
        s_pc[c] = pow2_scale(all);
        if (threadIdx.x == c && c < ncols) {
          norm[c * batch + p] = all;
          if (scaled != nullptr)
            scale[c * batch + p] = s_pc[c];
        }
      }
    }
  }
}

// sol64[c][p] += scale[c][p] * d[c][p] over `len` scalars per problem and column, the arrays [cols][batch][len] and
// [cols][batch]; skipped where status[p] != SIP_LQR_SUCCESS (= 0): status is per problem, not per column
template <typename S>
__global__ void __launch_bounds__(256)
    refine_update_kernel(const long cols, const long batch, const long len, const S *__restrict__ dvec,
                         const double *__restrict__ scale, const int32_t *__restrict__ status,
                         double *__restrict__ sol64) {
  const long total = cols * batch * len;
  for (long k = (long)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += (long)gridDim.x * blockDim.x) {
    const long cp = k / len; // c * batch + p
    if (status == nullptr || status[cp % batch] == 0)
      sol64[k] = __builtin_fma(scale[cp], (double)dvec[k], sol64[k]);
  }
}

} // namespace residual
} // namespace sipamd
