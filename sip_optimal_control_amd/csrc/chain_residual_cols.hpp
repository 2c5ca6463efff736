// chain_residual_cols.hpp -- the column form of the chain KKT residual (chain_residual.hpp): NC right-hand sides and
// iterates against one `mats`, laid out as sip_lqr_solve_multi lays its columns out (column c of a whole-batch array
// at c * col_stride scalars), and the column form of the refinement update (sip_lqr_residual_multi,
// sip_lqr_refine_multi).
//
// The single-column kernel is bound by instruction issue: addresses, per-row descriptors, loop control
// and the widening of every fp32 entry, none of which depends on the right-hand side.  Here a stage's image is staged
// once, a lane loads a matrix entry once, widens it once and issues NC fp64 FMAs into NC accumulators.
//
// Same shape as the single-column kernel: one workgroup per problem, wavefronts taking stages in turn, the wavefront
// of stage i computing rho_q[i], rho_r[i] and rho_c[i + 1] (stage 0: rho_c[0] too), the image [Q | delta | A | B | M |
// R] copied into LDS by 16-byte pieces from the piece that holds the stage's first scalar (tail by scalars, no load
// leaving the buffer, kCopyUnroll pieces in flight).  Per stage and wavefront the LDS holds (residual_cols_shape.hpp)
//   z[k][c]  k over x_i | y_i | u_i | x_{i+1} | y_{i+1},  e[k][c]  k over q_i | r_i | c_{i+1},  delta_{i+1}[k]
// with the NC columns of one entry adjacent: a term's NC operands are one or more 16-byte LDS reads.  The gather
// deals (k, c) pairs to lanes with c fastest, so that its LDS writes are contiguous.
//
// Column c is bit for bit what chain_residual_kernel computes on that column: kParts lanes per row, the terms of a
// lane in the same order through the same three segments, the two shuffle adds, and the closing expressions
// (acc - y) + q, acc + r, fma(-delta, y, acc - x) + c and fma(-delta_0, y_0, -x_0) + c_0.  After the shuffles the
// kParts lanes of a row hold the same sums; lane `part` closes and stores the columns c with c % kParts == part.
//
// A launch of the NC instantiation may carry ncols < NC columns: a masked column reads the last real column again
// (in bounds, and no branch among the loads) and stores nothing.
#pragma once
#include "chain_residual.hpp"
#include "residual_cols_shape.hpp"

namespace sipamd {
namespace residual {

// Terms of a dot product a lane reads out of LDS before it uses the first: NC accumulators and kDotUnroll x NC staged
// z values (two VGPRs each) do not fit next to the rest at NC = 8.
template <int NC>
constexpr int cols_dot_unroll() {
  return NC >= 8 ? 2 : 4;
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

// S, V as in chain_residual_kernel.  vecs, sol, res and scaled point at column 0 of the launch, column c at
// c * col_stride scalars; norm and scale at column 0, column c at c * batch.  res != nullptr or scaled == nullptr:
// plain form (res may be nullptr: norms only); scaled != nullptr: scaled form, one scale per problem and column.
template <typename S, typename V, bool STAGED, int NC>
__global__ void __launch_bounds__(kLanes *kColsMaxWaves)
    chain_residual_cols_kernel(const Dims d, const S *__restrict__ mats, const V *__restrict__ vecs,
                               const V *__restrict__ sol, const long col_stride, const long batch, const int ncols,
                               double *__restrict__ res, S *__restrict__ scaled, double *__restrict__ scale,
                               double *__restrict__ norm, const int wave_bytes) {
  static_assert(NC == 1 || NC == 2 || NC == 4 || NC == 8, "columns of an instantiation");
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  constexpr int LOG = NC == 1 ? 0 : (NC == 2 ? 1 : (NC == 4 ? 2 : 3));
  constexpr int DU = cols_dot_unroll<NC>();
  const int n = d.n, m = d.m, T = d.T, vstg = d.vstg;
  const long p = blockIdx.x;
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
  constexpr int PIECE = 16 / (int)sizeof(S);
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
      const long v0 = (long)i * vstg;
      lds_order(); // the previous stage's reads of z and the image are done
      // Item t = k * NC + c of a list is entry k of column c, and lands at [t]: lanes write LDS contiguously.  A lane
      // past the end of a list loads and stores the list's last item again; a masked column reads the last column.
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
        for (int k = pieces * PIECE + lane; k < total; k += kLanes) // what is left of the last piece
          img[k] = from[k];
        blk = img + lead;
      } else {
        blk = stage;
      }
      lds_order();

      // Rows and segments as in chain_residual_kernel; a term is one matrix entry against the NC columns of z[kk].
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
    refine_update_cols_kernel(const long cols, const long batch, const long len, const S *__restrict__ dvec,
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
