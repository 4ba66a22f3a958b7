// fbank_core.h -- what k_clip_fbank (fbank.hip) adds to mel_core.h's indexing and arithmetic: a lane's
// share of a frame's two energy passes, the mean, the column a coefficient goes to, the energy column's value and the mean
// subtraction.  One source for the kernel and for the host build the tests compile with g++ (tests/host_emul/fbank_emul.cpp).
#ifndef PDMP3_FBANK_CORE_H
#define PDMP3_FBANK_CORE_H
#include "mel_core.h"

namespace pdmp3 {

constexpr int kFbankWave = 64;              // lanes that share a frame's energy: one wave

// The energy of the frame whose first sample lies at position p0 of the tile's span, as 64 lanes take it: lane l adds
// the samples n = l, l + 64, ... < win, ascending; the lanes' sums are added pairwise (l with l ^ 32, ^ 16, ... ^ 1), which
// gives every lane the same total; the second pass likewise over (s - mean)^2, one fused multiply-add a sample.
MEL_FN float fbank_lane_sum(const float* span, unsigned p0, int win, unsigned hop, unsigned row_pad, float scale, int lane) {
  float acc = 0.0f;
  for (int n = lane; n < win; n += kFbankWave) acc = acc + scale * span[mel_lds_at(p0 + (unsigned)n, hop, row_pad)];
  return acc;
}
MEL_FN float fbank_mean(float total, int win) { return total / (float)win; }
MEL_FN float fbank_lane_squares(const float* span, unsigned p0, int win, unsigned hop, unsigned row_pad, float scale, float mean, int lane) {
  float acc = 0.0f;
  for (int n = lane; n < win; n += kFbankWave) {
    const float a = scale * span[mel_lds_at(p0 + (unsigned)n, hop, row_pad)] - mean;
    acc = mel_fma(a, a, acc);
  }
  return acc;
}
// the mel band that column d of a frame's D = n_mels + use_energy coefficients holds, or -1: the energy
MEL_FN int fbank_column_band(int d, int n_mels, int use_energy, int htk_compat) {
  if (!use_energy) return d;
  if (htk_compat) return d < n_mels ? d : -1;
  return d ? d - 1 : -1;
}
// the energy column: E, or max(ln max(E, eps), ln energy_floor) (log_floor = -inf: no floor)
MEL_FN float fbank_energy_output(float e, float eps, float log_floor, int mode) {
  if (mode != 1) return e;
  return fmaxf(logf(fmaxf(e, eps)), log_floor);
}
// subtract_mean: a column's sum over the valid frames (tiles ascending, frames ascending inside a tile) to its mean
MEL_FN float fbank_column_mean(float sum, unsigned valid) { return sum / (float)valid; }

}  // namespace pdmp3
#endif
