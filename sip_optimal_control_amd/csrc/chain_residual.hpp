// chain_residual.hpp -- the residual of the chain KKT system on the packed chain layout (include/sip_lqr_amd.h), in
// fp64, and the update of the iterative refinement built on it (sip_lqr_residual, sip_lqr_refine).
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
// every block of `mats` is fetched once: one contiguous image [Q | delta | A | B | M | R] by 16-byte loads into LDS
// (the transposed products A^T y, B^T y, M^T x then read columns out of LDS, not out of memory), next to the stage's
// part of z = (x_i, y_i, u_i, x_{i+1}, y_{i+1}) and the vector entries the rows end with (q_i, r_i, c_{i+1},
// delta_{i+1}) as doubles.  A wavefront that waits for one load at a time is bound by the latency of memory, not by
// its rate: the loads of a stage are issued kCopyUnroll (image) and kGatherUnroll (vectors) per lane before the first
// of them is waited for, and nothing after the staging reads memory.  Every row of the three results is one dot
// product against z; kParts lanes share a row and their partial sums meet by two shuffles.  A stage image that does
// not fit the LDS budget (or a `mats` that is not 16-byte aligned) is read in place instead (STAGED = false).
// Everything is summed in fp64 (FMA); fp32 blocks are widened on load, which is exact.
// The max-norm of a problem stays in its workgroup: lanes, then wavefronts through LDS; max is order-independent, so
// the result is deterministic.  The scaled form needs the norm before it can store anything: it walks the stages
// twice (norm, then rho / s), the second walk served by the caches (a problem's mats are 83 KB at n = 12, m = 4,
// T = 50 in fp32).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

namespace sipamd {
namespace residual {

constexpr int kLanes = 64;
constexpr int kParts = 4;    // lanes per row of the result; divides kLanes, so a row's lanes share a wavefront
constexpr int kMaxWaves = 4; // wavefronts of a workgroup
constexpr int kRedBytes = 32; // front of the dynamic LDS: one double per wavefront for the norm
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

// LDS of one wavefront: z (4 n + m doubles) and the row ends q_i | r_i | c_{i+1} | delta_{i+1} (3 n + m doubles),
// padded to a whole number of 16-byte pieces, then, when staged, the stage image: stg scalars behind up to
// 16 / sizeof(S) - 1 scalars of lead-in (the image starts at the 16-byte piece that holds the stage's first scalar),
// padded likewise.
__host__ __device__ inline int z_doubles(const Dims &d) { return (7 * d.n + 2 * d.m + 1) & ~1; }
__host__ __device__ inline int image_bytes(const Dims &d, int scalar_bytes) {
  return (d.stg * scalar_bytes + 16 + 15) & ~15;
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

// S: scalar of mats and of the scaled output; V: scalar of vecs and sol (S, or double: the wide form).
// res != nullptr or scaled == nullptr: plain form (res may be nullptr: norms only); scaled != nullptr: scaled form.
template <typename S, typename V, bool STAGED>
__global__ void __launch_bounds__(kLanes * kMaxWaves)
    chain_residual_kernel(const Dims d, const S *__restrict__ mats, const V *__restrict__ vecs,
                          const V *__restrict__ sol, double *__restrict__ res, S *__restrict__ scaled,
                          double *__restrict__ scale, double *__restrict__ norm, const int wave_bytes) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int n = d.n, m = d.m, T = d.T, vstg = d.vstg;
  const long p = blockIdx.x;
  // (the wavefront's number through readfirstlane: the compiler then knows that it, the stage and everything that
  // follows from them is the same in every lane, and keeps it in scalar registers and scalar branches)
  const int lane = threadIdx.x & (kLanes - 1), wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kLanes);
  const int waves = blockDim.x / kLanes;
  double *red = (double *)lds;
  unsigned char *mine = lds + kRedBytes + (size_t)wave * wave_bytes;
  double *z = (double *)mine;
  S *img = (S *)(mine + z_doubles(d) * sizeof(double));
  const S *pm = mats + p * d.mats_len;
  const V *pv = vecs + p * d.vecs_len, *ps = sol + p * d.vecs_len;
  constexpr int PIECE = 16 / (int)sizeof(S); // scalars per 16-byte piece
  const int part = lane & (kParts - 1);

  const int passes = scaled != nullptr ? 2 : 1;
  double s_p = 1.0;
  for (int pass = 0; pass < passes; ++pass) {
    const bool want_norm = pass == 0, store = pass == passes - 1;
    double nrm = 0.0;
    auto emit = [&](const int idx, const double v) {
      if (want_norm)
        nrm = nan_max(nrm, __builtin_fabs(v));
      if (store) {
        if (scaled != nullptr)
          scaled[p * d.vecs_len + idx] = (S)(v / s_p);
        else if (res != nullptr)
          res[p * d.vecs_len + idx] = v;
      }
    };
    for (int i = wave; i <= T; i += waves) {
      const bool edge = i < T;
      const long v0 = (long)i * vstg; // stage i in vecs / sol
      lds_order();                    // the previous stage's reads of z and the image are done
      // z[0, n) x_i | [n, 2n) y_i | [2n, 2n + m) u_i | [2n + m, 3n + m) x_{i+1} | [3n + m, 4n + m) y_{i+1}
      // then the row ends: e[0, n) q_i | [n, n + m) r_i | [n + m, 2n + m) c_{i+1} | [2n + m, 3n + m) delta_{i+1}
      double *e = z + 4 * n + m;
      // A lane past the end of a list loads and stores the list's last entry again: in bounds, the same value to the
      // same place, and no branch between the loads and the stores, which would leave one load in flight at a time.
      const int zl = edge ? 4 * n + m : 2 * n, el = edge ? 2 * n + m : n;
      const S *delta_src = pm + (long)(edge ? i + 1 : i) * d.stg + d.oD; // (the last stage has no use for it)
      for (int base = 0; base < zl; base += kLanes * kGatherUnroll) {   // zl >= el, n
        double rz[kGatherUnroll], re[kGatherUnroll], rd[kGatherUnroll];
        int kz[kGatherUnroll], ke[kGatherUnroll], kd[kGatherUnroll];
#pragma unroll
        for (int j = 0; j < kGatherUnroll; ++j) {
          const int k = base + j * kLanes + lane;
          kz[j] = k < zl ? k : zl - 1, ke[j] = k < el ? k : el - 1, kd[j] = k < n ? k : n - 1;
          rz[j] = (double)ps[v0 + kz[j]];
          // q_i, r_i: slots 0 and 2 of stage i; c_{i+1}: slot 1 of stage i + 1
          re[j] = (double)pv[v0 + ke[j] + (ke[j] < n ? 0 : (ke[j] < n + m ? n : 2 * n))];
          rd[j] = (double)delta_src[kd[j]];
        }
#pragma unroll
        for (int j = 0; j < kGatherUnroll; ++j)
          z[kz[j]] = rz[j], e[ke[j]] = re[j], e[2 * n + m + kd[j]] = rd[j];
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
      // loops whatever rows they hold.  kDotUnroll terms of a lane are loaded before the first is used.
      auto segment = [&](auto TRI, double acc, const int base, const int stride, const int count, const int zoff,
                         const bool tri_lane, const int r, const int dim) {
        for (int k = part; k < count; k += kParts * kDotUnroll) {
          S a[kDotUnroll];
          double zz[kDotUnroll];
#pragma unroll
          for (int j = 0; j < kDotUnroll; ++j) {
            const int kk = k + j * kParts < count ? k + j * kParts : k; // past the end: the first term again, unused
            int at = base + stride * kk;
            if constexpr (decltype(TRI)::value)
              at = tri_lane ? base + (kk < r ? tri(r, kk, dim) : tri(kk, r, dim)) : at;
            a[j] = blk[at], zz[j] = z[zoff + kk];
          }
#pragma unroll
          for (int j = 0; j < kDotUnroll; ++j)
            acc = k + j * kParts < count ? __builtin_fma((double)a[j], zz[j], acc) : acc;
        }
        return acc;
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
        double acc = 0.0;
        if (d.sym) { // Q (rho_q) and R (rho_r) are packed triangles: Q at 0, R at oR
          acc = segment(std::true_type{}, acc, q_row ? 0 : b0, s0, c0, 0, q_row, row, n);
          acc = segment(std::true_type{}, acc, r_row ? d.oR : b1, s1, c1, 2 * n, r_row, j, m);
        } else {
          acc = segment(std::false_type{}, acc, b0, s0, c0, 0, false, 0, 0);
          acc = segment(std::false_type{}, acc, b1, s1, c1, 2 * n, false, 0, 0);
        }
        acc = segment(std::false_type{}, acc, b2, 1, c2, 3 * n + m, false, 0, 0);
        acc += __shfl_xor(acc, 1);
        acc += __shfl_xor(acc, 2);
        if (active && part == 0) {
          if (row < n) {
            emit((int)v0 + row, (acc - z[n + row]) + e[row]);
          } else if (row < n + m) {
            emit((int)v0 + row + n, acc + e[row]); // slot r_i starts at 2n
          } else {
            const int r = row - n - m;
            const double t = __builtin_fma(-e[2 * n + m + r], z[3 * n + m + r], acc - z[2 * n + m + r]);
            emit((int)v0 + vstg + n + r, t + e[n + m + r]);
          }
        }
      }
      if (i == 0)
        for (int r = lane; r < n; r += kLanes)
          emit(n + r, __builtin_fma(-(double)blk[d.oD + r], z[n + r], -z[r]) + (double)pv[n + r]);
    }
    if (want_norm) {
      for (int off = kLanes / 2; off > 0; off >>= 1)
        nrm = nan_max(nrm, __shfl_xor(nrm, off));
      if (lane == 0)
        red[wave] = nrm;
      __syncthreads();
      double all = red[0];
      for (int k = 1; k < waves; ++k)
        all = nan_max(all, red[k]);
      s_p = pow2_scale(all);
      if (threadIdx.x == 0) {
        norm[p] = all;
        if (scaled != nullptr)
          scale[p] = s_p;
      }
    }
  }
}

// sol64[p] += scale[p] * d[p] over `len` scalars per problem, skipped where status[p] != SIP_LQR_SUCCESS (= 0)
template <typename S>
__global__ void __launch_bounds__(256)
    refine_update_kernel(const long batch, const long len, const S *__restrict__ dvec, const double *__restrict__ scale,
                         const int32_t *__restrict__ status, double *__restrict__ sol64) {
  const long total = batch * len;
  for (long k = (long)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += (long)gridDim.x * blockDim.x) {
    const long p = k / len;
    if (status == nullptr || status[p] == 0)
      sol64[k] = __builtin_fma(scale[p], (double)dvec[k], sol64[k]);
  }
}

} // namespace residual
} // namespace sipamd
