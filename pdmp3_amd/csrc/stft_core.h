// stft_core.h -- the pointwise arithmetic and the staging layout of k_clip_stft (stft.hip).  The span's
// place in LDS, the sample of the clip's row it holds, one step of a dot product and the power are k_clip_mel's
// (mel_core.h: mel_lds_at, mel_sample, mel_fma, mel_power); here: what is stored for a bin of a frame in modes 1 .. 4, and
// where a wave's 16 bins x tile frames lie in its staging tile.  One source for the kernel and for the host build the tests
// compile with g++ (tests/host_emul/stft_emul.cpp).
#ifndef PDMP3_STFT_CORE_H
#define PDMP3_STFT_CORE_H
#include "mel_core.h"

namespace pdmp3 {

constexpr int kStftThreads = kMelThreads;   // four waves

// what is stored for (Re, Im) in modes 1 .. 4 (mode 0 stores the pair itself); sqrtf is correctly rounded
MEL_FN float stft_value(float re, float im, float floor, int mode) {
  const float p = mel_power(re, im);
  if (mode == 1) return sqrtf(p);
  if (mode == 3) return logf(fmaxf(p, floor));
  if (mode == 4) return log10f(fmaxf(p, floor));
  return p;
}

// A wave's staging tile: a plane is 16 rows (bins) of `tile` frames, tile + 4 floats apart (36 or 20: a quarter of it is odd).
//   writes: a lane (j, kq) of the matrix instruction's result holds frames 4 kq .. 4 kq + 3 of bin j: one 16-byte store at
//     j stride + 16 rt + 4 kq.  A 16-byte store is served eight lanes at a time (j = 8 h .. 8 h + 7 of one kq): bank 4 j
//     (stride 36) or 20 j mod 32 = 0, 20, 8, 28, 16, 4, 24, 12 (stride 20) and the three behind it -- the eight lanes cover
//     the 32 banks once.
//   reads: lane l of pass `it` reads value i = 64 it + l: frame i % tile of row stft_stage_row(i / tile, tile).  A 4-byte
//     read is served 32 lanes at a time: at tile 32 they are the 32 consecutive frames of one row, 32 consecutive banks; at
//     tile 16 two rows of 16 frames, rows 4 apart: 80 floats, 16 banks apart, so the two runs of 16 cover the 32 banks once.
MEL_FN int stft_stage_stride(int tile) { return tile + 4; }
MEL_FN int stft_stage_row(int q, int tile) { return tile == 32 ? q : (q & 8) | ((q & 1) << 2) | ((q >> 1) & 3); }
// floats of a wave's staging tile
MEL_FN int stft_stage_floats(int tile, int mode) { return (mode == 0 ? 2 : 1) * 16 * stft_stage_stride(tile); }

}  // namespace pdmp3
#endif
