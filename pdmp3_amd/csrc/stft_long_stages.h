// stft_long_stages.h -- device code shared by k_clip_stft_long (stft_long.hip) and k_clip_mel_long (mel_long.hip): the two
// stages of the transform N = 64 N2 (n = N2 n1 + n2, k = k1 + 64 k2) on the matrix instruction, for a
// workgroup of eight waves and one tile kt of 16 values k1.  One source, inlined into both, so that a bin's Re and Im are the
// same binary32 numbers in both kernels; they differ in the sink that stage 2 hands them to.  HIP only; the index maps, the
// LDS layouts with their banks and the twiddle step are stft_long_core.h's.
#ifndef PDMP3_STFT_LONG_STAGES_H
#define PDMP3_STFT_LONG_STAGES_H
#include "clip_tile.h"
#include "stft_long_core.h"

namespace pdmp3 {

// Stage 1, rows (frame, n2), columns k1 = 16 kt + j: a wave keeps one tile of 16 n2 -- its sixteen window values
// wt[N2 n1 + n2], the 64-point DFT's B operands and its twiddles in registers -- and takes every (8 N2 / 16)-th frame of it:
// the A operand is wt times the plain span at fl hop + N2 n1 + n2, n1 = 4 s + kq ascending over sixteen steps; the result times
// the twiddle goes to Z in LDS.  The two kq of a 32-lane group read addresses N2 floats apart, the same banks: a two-way
// conflict on one 4-byte read per two matrix instructions, taken (a padding that removes it costs half of the span again).
template <int N2, int FT>
__device__ __forceinline__ void stftl_stage1(const float* span, const float* __restrict__ tab, unsigned hop, int kt, int wave, int j, int kq,
                                             float* z) {
  constexpr int N = 64 * N2, NT = N2 / 16;
  const int t = wave % NT;
  const float* const d64 = tab + stftl_tab_d64(N) + 16 * kt + j;
  const float* const tw = tab + stftl_tab_tw(N) + 16 * kt + j;
  float w[16], b_re[16], b_im[16], t_re[4], t_im[4];
#pragma unroll
  for (int s = 0; s < 16; s++) {
    w[s] = tab[N2 * (4 * s + kq) + 16 * t + j];
    b_re[s] = d64[(4 * s + kq) * 128];
    b_im[s] = d64[(4 * s + kq) * 128 + 64];
  }
#pragma unroll
  for (int r = 0; r < 4; r++) {
    t_re[r] = tw[(16 * t + 4 * kq + r) * 128];
    t_im[r] = tw[(16 * t + 4 * kq + r) * 128 + 64];
  }
  for (int fl = wave / NT; fl < FT; fl += 8 / NT) {
    f32x4 re = f32x4{0.0f, 0.0f, 0.0f, 0.0f}, im = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const float* const ap = span + (unsigned)fl * hop + N2 * kq + 16 * t + j;
#pragma unroll
    for (int s = 0; s < 16; s++) {
      const float a = stftl_window(w[s], ap[4 * N2 * s]);
      re = mfma16(a, b_re[s], re);
      im = mfma16(a, b_im[s], im);
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int n2 = 16 * t + 4 * kq + r;
      float zr, zi;
      stftl_twiddle(re[r], im[r], t_re[r], t_im[r], &zr, &zi);
      z[stftl_z_at(fl, n2, 0, j, N2)] = zr;
      z[stftl_z_at(fl, n2, 1, j, N2)] = zi;
    }
  }
}

// Stage 2, rows (frame, k1), columns k2 < N2 / 2: a wave keeps one tile ct = wave % (N2 / 32) of 16 columns of the half DFT in
// registers (stftl_stage2_operand) and takes every (8 / column tiles)-th frame: N2 / 2 steps over the 2 N2 terms (n2, part) of
// Z (stftl_stage2_chains), after which lane (j, kq) holds k1 = 16 kt + 4 kq + r, r = 0..3, of k2 = 16 ct + j.  The loop over
// the frames and what becomes of re, im are the caller's.  (As one function with a sink the stage cost k_clip_mel_long, which
// stands at the register limit, spills: profiles/clip_tile_ab.txt.)
template <int N2>
__device__ __forceinline__ void stftl_stage2_operand(const float* __restrict__ tab, int ct, int j, int kq, float (&b_re)[N2 / 2],
                                                     float (&b_im)[N2 / 2]) {
  constexpr int N = 64 * N2, K2 = N2 / 2;
  const float* const h2 = tab + stftl_tab_h2(N) + 16 * ct + j;
#pragma unroll
  for (int s = 0; s < N2 / 2; s++) {
    b_re[s] = h2[(4 * s + kq) * N2];
    b_im[s] = h2[(4 * s + kq) * N2 + K2];
  }
}
template <int N2>
__device__ __forceinline__ void stftl_stage2_chains(const float* z, int fl, int j, int kq, const float (&b_re)[N2 / 2],
                                                    const float (&b_im)[N2 / 2], f32x4& re, f32x4& im) {
  re = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  im = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int s = 0; s < N2 / 2; s++) {
    const float a = z[stftl_z_at(fl, 2 * s + (kq >> 1), kq & 1, j, N2)];
    re = mfma16(a, b_re[s], re);
    im = mfma16(a, b_im[s], im);
  }
}

}  // namespace pdmp3
#endif
