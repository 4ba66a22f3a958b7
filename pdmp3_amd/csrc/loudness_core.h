// loudness_core.h -- the indexing and the pointwise arithmetic of the loudness kernels (loudness.hip):
// where a sample lies in LDS, the binary64 steps of the states' scan, the split of a state into two binary32 operands, the
// sub-block a sample's square goes to, the order in which the waves' partial sums are added, and the gate's formulas.  One
// source for the kernels and for the host build the tests compile with g++ (tests/host_emul/loudness_emul.cpp).
#ifndef PDMP3_LOUDNESS_CORE_H
#define PDMP3_LOUDNESS_CORE_H
#include <math.h>
#include <stdint.h>

#include "../../include/pdmp3_hip.h"
#include "mel_core.h"

namespace pdmp3 {

constexpr int kLoudB = PDMP3_LOUD_B, kLoudChunk = PDMP3_LOUD_CHUNK;
constexpr int kLoudSpan = kLoudB * kLoudChunk;         // samples of a chunk
constexpr int kLoudWave = kLoudSpan / 4;               // samples of a wave of k_loud_blocks: 16 blocks
constexpr int kLoudRow = 68;                           // k_loud_blocks: floats between two blocks in LDS (4 n + k: 64 banks, 16-byte rows)
constexpr int kLoudRowS = 65;                          // k_loud_states: a lane walks a block, 64 lanes 64 banks
constexpr int kLoudGateThreads = 256;

MEL_FN int loud_at(int block, int k) { return block * kLoudRow + k; }
MEL_FN int loud_at_s(int block, int k) { return block * kLoudRowS + k; }
MEL_FN double loud_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }

// sample t of a row of T samples; zeros behind it
MEL_FN float loud_sample(const float* row, long long T, long long t) { return t < T ? row[t] : 0.0f; }

// w = R u: what the block's 64 samples leave in the state, each component one chain from +0, samples ascending
MEL_FN void loud_w(const double (*R)[PDMP3_LOUD_B], const float* u, double w[4]) {
  w[0] = w[1] = w[2] = w[3] = 0.0;
  for (int j = 0; j < kLoudB; j++) {
    const double x = (double)u[j];
    for (int m = 0; m < 4; m++) w[m] = loud_fma(R[m][j], x, w[m]);
  }
}
// s[m] += (M v)[m], M [4 x 4] row-major: one chain per component on top of s, columns ascending
MEL_FN double loud_row_acc(const double* M, int m, const double v[4], double s) {
  for (int i = 0; i < 4; i++) s = loud_fma(M[m * 4 + i], v[i], s);
  return s;
}
MEL_FN void loud_mat_acc(const double* M, const double v[4], double s[4]) {
  for (int m = 0; m < 4; m++) s[m] = loud_row_acc(M, m, v, s[m]);
}
// the power of Phi that step k of a wave-level scan over blocks (level 0) or chunks (level 1) takes: Phi^(2^k), Phi^(64 2^k)
MEL_FN int loud_pow_of(int level, int k) { return level == 0 ? 1 << k : 64 + k; }
// a state as two binary32 operands: hi + lo = s to 2^-48 relative
MEL_FN void loud_split(double s, float* hi, float* lo) {
  *hi = (float)s;
  *lo = (float)(s - (double)*hi);
}
// the A operand's element Hm[i][k] from the table's column 0
MEL_FN float loud_hm(const float* Hm, int i_minus_k) { return i_minus_k >= 0 ? Hm[(size_t)i_minus_k * PDMP3_LOUD_B] : 0.0f; }

// One lane's 16 values y of one block (samples i0, i0 + 1, ... in the order given) go into the wave's three partial sums:
// sub-block t / q counted from the wave's first one.  edge: the first sample of the sub-block behind the block's first one.
MEL_FN void loud_square(float y, long long t, long long edge, int bin0, float p[3]) {
  const int bin = t >= edge ? bin0 + 1 : bin0;
  const float sq = y * y;
  p[0] = bin == 0 ? p[0] + sq : p[0];
  p[1] = bin == 1 ? p[1] + sq : p[1];
  p[2] = bin == 2 ? p[2] + sq : p[2];
}

// s_c[i] of a row from its waves' partial sums part[wave][stride] = {bin 0, bin 1, bin 2, peak, ..}: the waves that hold samples
// of [i q, (i + 1) q) in ascending order, from the first one on by plain additions
MEL_FN float loud_sub_sum(const float* part, long long i, int q, int stride = 4) {
  const long long w0 = i * q / kLoudWave, w1 = ((i + 1) * q - 1) / kLoudWave;
  float s = 0.0f;
  for (long long w = w0; w <= w1; w++) {
    const float v = part[w * stride + (i - w * kLoudWave / q)];
    s = w == w0 ? v : s + v;
  }
  return s;
}
// the mean square of the window of n sub-blocks from j on, from the sub-block sums sub[c][n_sub], binary64:
// (((s_j + s_j+1) + s_j+2) + ..) + s_j+n-1 per channel, times G_c, channels added, over n q
MEL_FN double loud_zn(const float* sub, int n_sub, int channels, int dual_mono, long long j, int q, int n) {
  double z = 0.0;
  for (int c = 0; c < channels; c++) {
    const float* s = sub + (size_t)c * (size_t)n_sub + j;
    double a = (double)s[0] + (double)s[1];
    for (int i = 2; i < n; i++) a += (double)s[i];
    z = c == 0 ? (dual_mono ? 2.0 * a : a) : z + a;
  }
  return z / ((double)n * (double)q);
}
// z_j: the window of four
MEL_FN double loud_z(const float* sub, int n_sub, int channels, int dual_mono, long long j, int q) {
  return loud_zn(sub, n_sub, channels, dual_mono, j, q, 4);
}
MEL_FN double loud_l(double z) { return z > 0.0 ? -0.691 + 10.0 * log10(z) : -INFINITY; }
// g of a clip: 1 without a target or without a loudness; else 10^((target - L) / 20), held to peak_limit / P
MEL_FN float loud_gain(double L, double P, double target, double peak_limit) {
  if (target != target || !(L > -INFINITY)) return 1.0f;
  double g = pow(10.0, (target - L) / 20.0);
  if (peak_limit > 0.0 && g * P > peak_limit) g = peak_limit / P;
  return (float)g;
}

}  // namespace pdmp3
#endif
