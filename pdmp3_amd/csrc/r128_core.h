// r128_core.h -- the pointwise pieces of the true peak, the short-term loudness and the loudness range of clips
// (loudness.hip k_loud_blocks<true>, k_loud_gate<true>) on top of loudness_core.h: the interpolator's
// A operand, the samples in front of a wave's first block, the range's two indices and its rank by counting.  One source for
// the kernels and for the host build the tests compile with g++ (tests/host_emul/r128_emul.cpp).
#ifndef PDMP3_R128_CORE_H
#define PDMP3_R128_CORE_H
#include "loudness_core.h"

namespace pdmp3 {

constexpr int kR128Taps = PDMP3_R128_TAPS;
constexpr int kR128Steps = 7;                          // k-steps of four that a tile of 16 outputs takes: columns 16 mt - 12 .. 16 mt + 15
constexpr int kR128Window = 30;                        // sub-blocks of a short-term window
constexpr int kR128Every = 10;                         // sub-blocks between two windows of the range
constexpr int kR128MaxRange = PDMP3_R128_MAX_RANGE;
constexpr int kR128Part = 8;                           // floats of a wave's partial results: {bin 0, bin 1, bin 2, peak, interpolated peak, 0, 0, 0}

// the A operand's element Tp[i][k] = c_p[i - k] of phase p = 1 .. 3 from taps[3][12]; zero outside the band
MEL_FN float r128_tap(const float* taps, int p, int i_minus_k) {
  return i_minus_k >= 0 && i_minus_k < kR128Taps ? taps[(p - 1) * kR128Taps + i_minus_k] : 0.0f;
}
// sample t of a row of T samples: zeros in front of it (the filter starts from rest) and behind it
MEL_FN float r128_sample(const float* row, long long T, long long t) { return t >= 0 && t < T ? row[t] : 0.0f; }

// the places of the 95th and the 10th percentile among n sorted values (n >= 1): libebur128's (size_t)((n - 1) 0.95 + 0.5)
// and (size_t)((n - 1) 0.1 + 0.5) in integers
MEL_FN long long r128_hi_index(long long n) { return (19 * (n - 1) + 10) / 20; }
MEL_FN long long r128_lo_index(long long n) { return (n + 4) / 10; }

// the place of v[m] among the n values v[0 .. n - 1] sorted ascending, ties by index; +inf marks a value that is not in the set
// and counts for nothing (m's own value must be in the set)
MEL_FN long long r128_rank(const double* v, long long n, long long m) {
  const double x = v[m];
  long long r = 0;
  for (long long i = 0; i < n; i++) r += (v[i] < x || (v[i] == x && i < m)) ? 1 : 0;
  return r;
}

}  // namespace pdmp3
#endif
