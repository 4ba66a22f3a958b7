// spectral_core.h -- what k_clip_spectral (spectral.hip) adds to stft_long_core.h: the LDS layout of the
// plane that holds a tile's whole spectrum with its banks, the floats of the four LDS regions, the runs of bins a lane reduces
// and the arithmetic of the six descriptors, lane by lane.  One source for the kernel and for the host build the tests compile
// with g++ (tests/host_emul/spectral_emul.cpp): what crosses lanes (the butterfly, the scan, the minimum) is written twice, in
// the orders given here.
#ifndef PDMP3_SPECTRAL_CORE_H
#define PDMP3_SPECTRAL_CORE_H
#include "stft_long_core.h"

namespace pdmp3 {

constexpr int kSpectralThreads = 512;       // eight waves: one workgroup a CU at these LDS sizes, two waves a SIMD
constexpr int kSpectralRows = 6;            // rms, zcr, centroid, bandwidth, rolloff, flatness

// frames of a workgroup: one a wave at N 2048; at N 4096 Z and the plane of eight frames alone would pass the LDS
MEL_FN int spec_tile(int n_fft) { return n_fft == 2048 ? 8 : 4; }

// ---- LDS: the span (plain, kept for all four kt), then Z (stft_long_core.h), then the plane, then the results ----
// The plane: a row of N / 2 + 1 floats a frame of the tile, rows one behind the other (no padding between them: one wave
// works on one frame at a time, so the rows' distance meets no bank rule).  Stage 2 writes the power P of a bin, the
// reduction turns it into the magnitude S = sqrtf(P) in place.  Bin k of a frame lies at column
//   spec_col(k) = k ^ g(k >> 5),   g(h) = (h & 1) << 2 | (h >> 1) & 3 | h & 24:
// the natural order with the five low bits of the column mixed with bits 5 .. 9 of the bin; a block of 32 bins stays the block
// of 32 floats it is, and bin N / 2 stays at column N / 2.  No stride does what this does: a 32-lane group of stage 2 holds
// sixteen bins 64 apart (j) twice (kq & 1: 4 apart), and in the natural order every j would meet the same bank whatever the
// rows' distance -- sixteen ways; a lane's run of consecutive bins (below) would put 32 lanes on two banks.
//   stage 2 writes (ds_write_b32, 32 lanes at a time = kq 0 and 1, or 2 and 3): lane (j, kq) holds bin 16 kt + 4 kq + r + 64 (16 ct + j):
//     k >> 5 = (kt >> 1) + 2 (16 ct + j), so g puts j's four bits into bank bits 0, 1, 3, 4, and kq & 1 is bit 2 of k: the 32
//     lanes of a group cover the 32 banks once.
//   the reduction reads and writes (ds_read_b32 / ds_write_b32): lane l at step i is at bin R l + i, R = N / 128 = 16 or 32.
//     R = 16: bit 4 of k is l & 1 and k >> 5 = l >> 1, whose bits 0 .. 3 g puts into bank bits 2, 0, 1, 3; R = 32: k >> 5 = l,
//     bank bits 2, 0, 1, 3, 4.  The 32 lanes of a group cover the 32 banks once at every step.
MEL_FN int spec_bins(int n_fft) { return n_fft / 2 + 1; }
MEL_FN unsigned spec_col(int k) {
  const unsigned h = (unsigned)k >> 5;
  return (unsigned)k ^ (((h & 1u) << 2) | ((h >> 1) & 3u) | (h & 24u));
}
MEL_FN unsigned spec_plane_floats(int tile, int n_fft) { return (unsigned)(tile * spec_bins(n_fft)); }
MEL_FN unsigned spec_span_floats(int tile, int hop, int n_fft) { return (stftl_span(tile, hop, n_fft) + 3u) & ~3u; }
// the results: [row][frame of the tile] behind the plane, so that consecutive lanes store consecutive frames of a row
MEL_FN unsigned spec_res_floats(int tile) { return (unsigned)(8 * tile); }
MEL_FN unsigned spec_lds_floats(int tile, int hop, int n_fft) {
  return (spec_span_floats(tile, hop, n_fft) + stftl_z_floats(tile, stftl_n2(n_fft)) + spec_plane_floats(tile, n_fft) + spec_res_floats(tile) + 3u) & ~3u;
}

// ---- the arithmetic (the engine compiles with -ffp-contract=off) ----
// Every sum below is a binary64 sum in one fixed order: a lane adds its own terms in ascending order, then the 64 lanes' sums
// are added -- by the butterfly (v = v + v[lane ^ off], off = 32, 16, .. 1: the same tree for every lane) or, for the
// magnitudes, by the scan (p_0 = 0, p_(l + 1) = p_l + t_l, l ascending), whose last value is THE total: the centroid, the
// bandwidth and the roll-off's threshold all use it.
//
// rows 0 and 1: lane l takes the samples n = l + 64 i of the frame, i ascending.  x^2 is exact in binary64.
MEL_FN bool spec_neg(float v, float t) { return v < -t; }
MEL_FN void spec_lane_frame(const float* x, int n_fft, int lane, float t, double* sq, int* cross) {
  double s = 0.0;
  int c = 0;
  for (int n = lane; n < n_fft; n += 64) {
    const double v = (double)x[n];
    s = s + v * v;
    if (n >= 1 && spec_neg(x[n], t) != spec_neg(x[n - 1], t)) c++;
  }
  *sq = s;
  *cross = c;
}
MEL_FN float spec_rms(double sq, int n_fft) { return (float)sqrt(sq / (double)n_fft); }
MEL_FN float spec_zcr(int cross, int n_fft) { return (float)cross / (float)n_fft; }       // (exact: an integer below 2^24 by a power of two)

// rows 2 .. 5.  Lane l's run: the bins R l .. R l + R - 1, R = N / 128, ascending; lane 63's run ends with bin N / 2.
MEL_FN int spec_run(int n_fft) { return n_fft >> 7; }
MEL_FN int spec_run_end(int n_fft, int lane) { return spec_run(n_fft) * (lane + 1) + (lane == 63 ? 1 : 0); }
MEL_FN double spec_freq(int k, double bin_hz) { return (double)k * bin_hz; }              // (exact: k < 2^12, bin_hz = sr / N has at most 31 bits)
// pass A: P -> S in place; the lane's sums of S, f S, logf(max(P, amin)) and max(P, amin)
MEL_FN void spec_lane_pass_a(float* row, int n_fft, int lane, double bin_hz, float amin, double* ts, double* tfs, double* tln, double* tp) {
  double s = 0.0, fs = 0.0, ln = 0.0, p = 0.0;
  for (int k = spec_run(n_fft) * lane; k < spec_run_end(n_fft, lane); k++) {
    const unsigned at = spec_col(k);
    const float pk = row[at], sk = sqrtf(pk), pm = fmaxf(pk, amin);
    row[at] = sk;
    s = s + (double)sk;
    fs = fs + spec_freq(k, bin_hz) * (double)sk;
    ln = ln + (double)logf(pm);
    p = p + (double)pm;
  }
  *ts = s; *tfs = fs; *tln = ln; *tp = p;
}
// pass B, the centroid c, the lane's place in the scan and the threshold known: the lane's sum of S (f - c)^2, and the first
// bin of its run at which the cumulative sum prefix + (S_first + .. + S_k) reaches the threshold (-1: none).  The running
// sum of the run is pass A's, so the last bin's cumulative sum is the next lane's prefix: the sequence never falls.
MEL_FN void spec_lane_pass_b(const float* row, int n_fft, int lane, double bin_hz, double c, double prefix, double threshold, double* tbw, int* first) {
  double bw = 0.0, run = 0.0;
  int at = -1;
  for (int k = spec_run(n_fft) * lane; k < spec_run_end(n_fft, lane); k++) {
    const double sk = (double)row[spec_col(k)], dev = spec_freq(k, bin_hz) - c;
    bw = bw + sk * (dev * dev);
    run = run + sk;
    if (at < 0 && prefix + run >= threshold) at = k;
  }
  *tbw = bw;
  *first = at;
}
// the four values of a frame from its totals, each rounded once to binary32; a frame without magnitude: rows 2 .. 4 are 0
MEL_FN double spec_centroid(double fs, double total) { return total > 0.0 ? fs / total : 0.0; }
MEL_FN double spec_threshold(double roll_percent, double total) { return roll_percent * total; }
MEL_FN float spec_bandwidth(double bw, double total) { return total > 0.0 ? (float)sqrt(bw / total) : 0.0f; }
MEL_FN float spec_rolloff(int first, double bin_hz) { return (float)spec_freq(first, bin_hz); }
MEL_FN float spec_flatness(double ln, double p, int n_fft) {
  const double bins = (double)spec_bins(n_fft);
  return (float)(exp(ln / bins) / (p / bins));
}

}  // namespace pdmp3
#endif
