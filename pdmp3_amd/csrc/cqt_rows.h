// cqt_rows.h -- device code shared by k_clip_cqt (cqt.hip) and k_clip_chroma (chroma.hip): the matrix instruction, the wave's
// own synchronisation and the rows of a tile of 16 bins times the workgroup's 16 frames.  One source, so that a bin's value of a
// frame is the same binary32 number in both kernels (DESIGN.md sections 16 and 17).  HIP only; the indexing and the arithmetic
// that the host build shares are cqt_core.h's.
#ifndef PDMP3_CQT_ROWS_H
#define PDMP3_CQT_ROWS_H
#include <hip/hip_runtime.h>

#include "cqt_core.h"

namespace pdmp3 {

typedef float f32x4 __attribute__((ext_vector_type(4)));
// v_mfma_f32_16x16x4_f32: lane l = (j = l & 15, kq = l >> 4) holds A[row j][k = kq], B[k = kq][col j] and
// D[row 4 kq + r][col j], r = 0..3; each D element is a fused multiply-add chain over k = 0..3 on top of C
__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
// what a wave's lanes wrote to its plane is there for its other lanes (LDS operations of a wave complete in order)
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Rows [r0, r1) of a tile of 16 bins (r0, r1 multiples of 4) times the 16 frames of the workgroup, Re and Im each one chain
// from +0, rows ascending, into the wave's plane `pw`.  The frames are overlapping rows of the span: the A operand is read at
// jf hop + base + n and never materialised; the B operand is the tile's rows of the table, read from memory (L2): four rows of
// 32 floats a step.  Lanes of frames from FT on (tiles of 8 and 4 frames) read frame j mod FT again: nothing of theirs is stored.
// A shorter tile's padding rows (up to three, exact zeros) may stand behind the span's last sample: the read stops at `last`,
// the span's last float, and the finite sample there times the zero adds nothing.
__device__ __forceinline__ void cqt_rows(const float* span, const float* __restrict__ tile_tab, unsigned base, int r0, int r1, unsigned hop,
                                         unsigned chunk, unsigned last, unsigned jf, int j, int kq, float* pw) {
  f32x4 re = f32x4{0.0f, 0.0f, 0.0f, 0.0f}, im = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  const unsigned q = base + (unsigned)r0 + (unsigned)kq;
  unsigned c = jf + q / hop, rem = q % hop;
  const float* bp = tile_tab + (size_t)(r0 + kq) * 32 + j;
  // one step: four rows of the table times the sixteen frames' four samples, on top of the two chains
  auto step = [&](float b_re, float b_im) {
    const float a = span[min(c * chunk + rem, last)];
    re = mfma16(a, b_re, re);
    im = mfma16(a, b_im, im);
    rem += 4;
    if (rem >= hop) {
      if (hop >= 4) { rem -= hop; c++; }
      else { c += rem / hop; rem %= hop; }
    }
  };
  // blocks of kU steps: the next block's coefficients are on their way from L2 while this block's matrix instructions run
  constexpr int kU = 8;
  const int blocks = (r1 - r0) / (4 * kU);
  float cre[kU], cim[kU], nre[kU], nim[kU];
  if (blocks > 0) {
#pragma unroll
    for (int u = 0; u < kU; u++) { cre[u] = bp[128 * u]; cim[u] = bp[128 * u + 16]; }
    bp += 128 * kU;
  }
  for (int b = 0; b < blocks; b++) {
    if (b + 1 < blocks) {
#pragma unroll
      for (int u = 0; u < kU; u++) { nre[u] = bp[128 * u]; nim[u] = bp[128 * u + 16]; }
      bp += 128 * kU;
    }
#pragma unroll
    for (int u = 0; u < kU; u++) step(cre[u], cim[u]);
#pragma unroll
    for (int u = 0; u < kU; u++) { cre[u] = nre[u]; cim[u] = nim[u]; }
  }
  for (int n = r0 + 4 * kU * blocks; n < r1; n += 4) {
    step(bp[0], bp[16]);
    bp += 128;
  }
#pragma unroll
  for (int r = 0; r < 4; r++) {
    pw[cqt_part_at(j, 4 * kq + r)] = re[r];
    pw[kCqtPlane + cqt_part_at(j, 4 * kq + r)] = im[r];
  }
}

}  // namespace pdmp3
#endif
