// residual_cols_shape.hpp -- the launch shape of the chain residual (chain_residual.hpp), for one column and for
// several: how many columns one launch carries, how many wavefronts a workgroup has, whether the stage image goes
// through LDS, and the dynamic LDS that takes.  The constants and sizes of the kernel's LDS are stated here and nowhere
// else.  Host arithmetic only: no HIP call and no kernel in here, so a host program can print the decisions
// (tests/cpp/test_residual_cols_shape.cpp).  The kernel header includes it for the sizes it shares.
//
// LDS of a workgroup: NC doubles per wavefront slot for the norms (kColsMaxWaves slots), then per wavefront
//   z[k][c]   (4 n + m) NC doubles   x_i | y_i | u_i | x_{i+1} | y_{i+1}, the NC columns of one entry adjacent
//   e[k][c]   (2 n + m) NC doubles   the row ends q_i | r_i | c_{i+1}
//   delta     n doubles              delta_{i+1}, once: it belongs to mats, not to a column
// padded to 16 bytes, then, when staged, the stage image: the stage's scalars behind up to 16 / sizeof(S) - 1 scalars of
// lead-in (the image starts at the 16-byte piece that holds the stage's first scalar), padded likewise.
//
// Rules: never more than 64 KiB; staged needs `mats` 16-byte aligned and the image plus NC vector sets to fit; staged
// with fewer columns is preferred over unstaged with more; among the staged (or, failing those, the unstaged) column
// counts the largest one that still leaves kColsWantWaves wavefronts (or one per stage, if the chain has fewer
// stages) wins, and where none does the largest that fits at all; no more wavefronts than stages.
#pragma once
#include <cstddef>

#if defined(__HIPCC__)
#define SIP_COLS_HD __host__ __device__
#else
#define SIP_COLS_HD
#endif

// Wavefronts a workgroup should keep before the column count is cut for them.  1: columns come first.  Measured at
// n = 32, m = 8 in fp64: 8 columns x 1 wavefront beats 4 x 2, which a build with 2 here gives.
#ifndef SIP_RESIDUAL_COLS_WANT_WAVES
#define SIP_RESIDUAL_COLS_WANT_WAVES 1
#endif

namespace sipamd {
namespace residual {

constexpr int kColsMax = 8;      // columns of the widest instantiation; the instantiations are 1, 2, 4 and 8
constexpr int kColsMaxWaves = 4; // wavefronts of a workgroup
constexpr int kColsWantWaves = SIP_RESIDUAL_COLS_WANT_WAVES;
constexpr size_t kColsLdsBudget = 64 * 1024; // dynamic LDS a launch may ask for without raising the kernel's limit

struct ColsShape {
  int columns; // of the instantiation that is launched: 1, 2, 4 or 8 (a shorter group masks the rest); 0: nothing fits
  int waves;
  bool staged;
  size_t lds_bytes;
};

// front of the dynamic LDS: NC doubles per wavefront for the norms
SIP_COLS_HD inline int cols_red_bytes(const int nc) { return nc * 8 * kColsMaxWaves; }
// doubles of one wavefront's vectors, padded to a whole number of 16-byte pieces
SIP_COLS_HD inline int cols_z_doubles(const int n, const int m, const int nc) {
  return (nc * (6 * n + 2 * m) + n + 1) & ~1;
}
// scalars of one stage of `mats`: [Q | delta | A | B | M | R]
inline int cols_stage_scalars(const int n, const int m, const bool sym) {
  const int nq = sym ? n * (n + 1) / 2 : n * n, nr = sym ? m * (m + 1) / 2 : m * m;
  return nq + n + n * n + 2 * n * m + nr;
}
// the image behind up to one 16-byte piece of lead-in, padded to whole pieces
inline size_t cols_image_bytes(const int stage_scalars, const int scalar_bytes) {
  return ((size_t)stage_scalars * scalar_bytes + 16 + 15) & ~(size_t)15;
}

// The instantiation that carries `requested` columns: the least of 1, 2, 4, 8 that holds them.
inline int cols_instance(const int requested) {
  int nc = 1;
  while (nc < requested && nc < kColsMax)
    nc *= 2;
  return nc;
}

inline ColsShape cols_shape(const int n, const int m, const int T, const bool f32, const bool sym,
                            const bool mats_aligned, const int requested) {
  const size_t image = cols_image_bytes(cols_stage_scalars(n, m, sym), f32 ? 4 : 8);
  const int stages = T + 1, want = stages < kColsWantWaves ? stages : kColsWantWaves;
  for (int staged = 1; staged >= 0; --staged) {
    if (staged && !mats_aligned)
      continue;
    for (int round = 0; round < (want > 1 ? 2 : 1); ++round) { // with `want` wavefronts, then with one
      const int need = round == 0 ? want : 1;
      for (int nc = cols_instance(requested); nc >= 1; nc /= 2) {
        const size_t wave_bytes = (size_t)cols_z_doubles(n, m, nc) * 8 + (staged ? image : 0);
        const size_t red = (size_t)cols_red_bytes(nc);
        if (red + (size_t)need * wave_bytes > kColsLdsBudget)
          continue;
        int waves = (int)((kColsLdsBudget - red) / wave_bytes);
        waves = waves < kColsMaxWaves ? waves : kColsMaxWaves;
        waves = waves < stages ? waves : stages;
        return {nc, waves, staged != 0, red + (size_t)waves * wave_bytes};
      }
    }
  }
  return {0, 0, false, 0};
}

} // namespace residual
} // namespace sipamd
