// stft_long_core.h -- what k_clip_stft_long (stft_long.hip) adds to mel_core.h / stft_core.h: the index
// maps of the two-stage transform N = 64 N2 (n = N2 n1 + n2, k = k1 + 64 k2), the places of its tables, the LDS layouts of
// the intermediate Z and of the workgroup's staging tile, the twiddle step and the Nyquist bin's chain.  One source for the
// kernel and for the host build the tests compile with g++ (tests/host_emul/stft_long_emul.cpp).
#ifndef PDMP3_STFT_LONG_CORE_H
#define PDMP3_STFT_LONG_CORE_H
#include "stft_core.h"

namespace pdmp3 {

constexpr int kStftLongThreads = 512;       // eight waves: one workgroup a CU at these LDS sizes, two waves a SIMD

// ---- the tables: one block of floats, wt | the 64-point DFT | the N2-point half DFT | the twiddles ----
//   wt[n], n < N: fl32(s w[n]);
//   D64[n1][128]: cos(2 pi n1 k1 / 64) at column k1 < 64, -sin at column 64 + k1;
//   H2[t][N2], t = 2 n2 + part < 2 N2, K2 = N2 / 2 columns of Re coefficients, then K2 of Im coefficients: with
//     a = 2 pi n2 k2 / N2, column k2 holds cos a (part 0: times Zr) or sin a (part 1: times Zi), column K2 + k2 holds -sin a
//     (part 0) or cos a (part 1);
//   TW[n2][128]: cos(2 pi n2 k1 / N) at column k1, -sin at column 64 + k1.
MEL_FN int stftl_n2(int n_fft) { return n_fft >> 6; }
MEL_FN int stftl_tab_d64(int n_fft) { return n_fft; }
MEL_FN int stftl_tab_h2(int n_fft) { return n_fft + 64 * 128; }
MEL_FN int stftl_tab_tw(int n_fft) { return stftl_tab_h2(n_fft) + 2 * stftl_n2(n_fft) * stftl_n2(n_fft); }
MEL_FN int stftl_tab_floats(int n_fft) { return stftl_tab_tw(n_fft) + stftl_n2(n_fft) * 128; }

// ---- LDS: region 0 (the tile's span, plain; after stage 1 the staging tile), then Z ----
// Z: (frame fl of the tile, n2, part, k1l = k1 - 16 kt): 32 floats a (fl, n2) -- Re's sixteen k1l and Im's; the two halves
// change places where bit 2 of n2 is set.
//   stage 1 writes (ds_write_b32, 32 lanes at a time = kq 0 and 1 or kq 2 and 3): lane (j, kq) holds n2 = 16 t + 4 kq + r,
//     k1l = j: the two kq of a group differ in bit 2 of n2, so they write the two halves: 32 banks once.
//   stage 2 reads (ds_read_b32): lane (j, kq) reads n2 = 2 s + (kq >> 1), part = kq & 1, k1l = j: a group's 32 lanes read the
//     32 floats of one (fl, n2): 32 banks once.
MEL_FN unsigned stftl_z_at(int fl, int n2, int part, int k1l, int N2) {
  return (unsigned)((fl * N2 + n2) * 32 + ((part ^ ((n2 >> 2) & 1)) << 4) + k1l);
}
MEL_FN unsigned stftl_z_floats(int tile, int N2) { return (unsigned)(tile * N2 * 32); }
// The staging tile: per plane (mode 0: Re's, then Im's) 16 K2 rows of tile + 1 floats, frames innermost; the row of
// (k1l, k2) is k1l K2 + k2.
//   stage 2 writes: lane (j, kq) holds k2 = 16 ct + j, k1l = 4 kq + r: rows j apart by one row, tile + 1 floats (odd): 16
//     banks once; the two kq of a group are 4 K2 rows apart, a multiple of 32 floats: a two-way conflict, taken (8 or 4
//     stores against 32 or 64 matrix instructions).
//   the store loop reads value i = (row, fl) = (i / tile, i % tile) with consecutive lanes: consecutive floats with one float
//     skipped per row -- 32 lanes cover at most 32 + 32 / tile - 1 floats, so at most 32 / tile - 1 banks are read twice (one
//     at tile 16).
MEL_FN int stftl_stage_stride(int tile) { return tile + 1; }
MEL_FN unsigned stftl_stage_plane(int tile, int N2) { return (unsigned)(16 * (N2 >> 1) * stftl_stage_stride(tile)); }
MEL_FN unsigned stftl_stage_at(int plane, int k1l, int k2, int fl, int tile, int N2) {
  return plane * stftl_stage_plane(tile, N2) + (unsigned)((k1l * (N2 >> 1) + k2) * stftl_stage_stride(tile) + fl);
}
MEL_FN unsigned stftl_stage_floats(int tile, int N2, int mode) { return (mode == 0 ? 2u : 1u) * stftl_stage_plane(tile, N2); }
// floats of the tile's span
MEL_FN unsigned stftl_span(int tile, int hop, int n_fft) { return (unsigned)(tile - 1) * (unsigned)hop + (unsigned)n_fft; }

// ---- the arithmetic (the engine compiles with -ffp-contract=off: every product and every fused step is written out) ----
// step 0: one product a sample
MEL_FN float stftl_window(float wt, float y) { return wt * y; }
// step 2: Z = Y T, three roundings a component
MEL_FN void stftl_twiddle(float yr, float yi, float tr, float ti, float* zr, float* zi) {
  *zr = __builtin_fmaf(yr, tr, -(yi * ti));
  *zi = __builtin_fmaf(yr, ti, yi * tr);
}
// step 3's chain order: the 2 N2 terms t = 2 n2 + part ascending, for Re and for Im (the matrix instruction takes four of
// them a step, k ascending).  The Nyquist bin N / 2 = (k1 0, k2 N2 / 2) is the same chain with that column's coefficients,
// which are exact: (-1)^n2 for the cosine, +0 for the sine and -0 for its negative.  z: the LDS region of Z in a workgroup
// with kt = 0.
MEL_FN void stftl_nyquist(const float* z, int fl, int N2, float* re, float* im) {
  float r = 0.0f, i = 0.0f;
  for (int n2 = 0; n2 < N2; n2++) {
    const float c = (n2 & 1) ? -1.0f : 1.0f;
    const float zr = z[stftl_z_at(fl, n2, 0, 0, N2)], zi = z[stftl_z_at(fl, n2, 1, 0, N2)];
    r = mel_fma(zr, c, r);
    r = mel_fma(zi, 0.0f, r);
    i = mel_fma(zr, -0.0f, i);
    i = mel_fma(zi, c, i);
  }
  *re = r;
  *im = i;
}

}  // namespace pdmp3
#endif
