// hpss_core.h -- the phases of k_clip_hpss (hpss.hip): the tile of a workgroup with its halo in LDS, the
// reflection of the bins, the selection of a median of up to 31 values in registers, the soft mask and what a mode stores.  One
// source for the kernel and for the host build the tests compile with g++ (tests/host_emul/hpss_emul.cpp).  Nothing here
// crosses lanes: a lane takes both windows of its element from LDS and everything else is its own.
#ifndef PDMP3_HPSS_CORE_H
#define PDMP3_HPSS_CORE_H
#include "stft_core.h"

namespace pdmp3 {

constexpr int kHpssThreads = 256;           // four waves
constexpr int kHpssBins = 64;               // the tile of a workgroup: bins ...
constexpr int kHpssFrames = 64;             // ... x frames: a wave's 64 lanes are the 64 frames of one bin
constexpr int kHpssMaxKernel = 31;          // the largest window; a window is padded to this many values

// ---- LDS: the tile with its halo ----
// The tile is laid out for the largest kernels whatever the call's are: 64 + 30 rows (bins) of 64 + 30 floats (frames), rows
// `pitch` = 94 floats apart, the lane's element of bin b of the tile at row 15 + b, column 15 + lane.  So every offset of
// both windows is a constant of the instruction.  Only what the call's windows reach is loaded -- row 15 - rp + r is bin
// rho(k0 - rp + r), r < 64 + 2 rp; column 15 - rh + c is stage frame f0 + c, c < 64 + 2 rh (the stage's frame 0 is the clip's
// frame -rh), zeros from the stage's last frame on -- and what a window of 31 reads beyond that is replaced (hpss_median).
// A wave is at ONE bin with its lanes at 64 consecutive frames, so
//   the harmonic window's step j reads   (15 + b) pitch + lane + j              -- 64 consecutive floats,
//   the percussive window's step i reads (b + i) pitch + 15 + lane              -- 64 consecutive floats,
//   the load writes                       (15 - rp + r) pitch + 15 - rh + lane (+ 64) -- 64 consecutive floats,
// and a 4-byte access, served 32 lanes at a time over 32 banks, meets every bank once whatever the pitch is.
constexpr int kHpssHalo = kHpssMaxKernel / 2;
constexpr int kHpssPitch = kHpssFrames + 2 * kHpssHalo;
constexpr int kHpssRows = kHpssBins + 2 * kHpssHalo;
constexpr unsigned kHpssLdsFloats = (unsigned)(kHpssRows * kHpssPitch);
// where the load puts row r, column c of what it loads, and where a lane's element lies: bin b of the tile (0 .. 63), frame `lane`
MEL_FN unsigned hpss_lds_at(int r, int c, int rh, int rp) { return (unsigned)((kHpssHalo - rp + r) * kHpssPitch + kHpssHalo - rh + c); }
MEL_FN unsigned hpss_centre(int b, int lane) { return (unsigned)((kHpssHalo + b) * kHpssPitch + kHpssHalo + lane); }

// rho: scipy.ndimage's "reflect", numpy's "symmetric" -- the edge bin is repeated.  One reflection serves: K is above 1024 and
// a tile reaches at most 64 + 15 bins past either end; the clamp keeps any index inside the spectrum all the same.
MEL_FN int hpss_reflect(int i, int bins) {
  const int r = i < 0 ? -1 - i : i >= bins ? 2 * bins - 1 - i : i;
  return r < 0 ? 0 : r >= bins ? bins - 1 : r;
}

// ---- the medians ----
// Every S is +0 or positive and finite, so binary32 values order as their bit patterns do as signed integers: the selection
// runs on the patterns with integer minimum and maximum, touches no rounding mode or denormal setting and returns one of its
// inputs.  A window of L = 2 r + 1 values is padded to 31 with (31 - L) / 2 patterns below every value in front and as many
// above every value behind, which leaves the median where it was; a 32nd value above all makes the count a power of two.
// Batcher's odd-even merge sort of 32 is a fixed network of 191 compare-exchanges; only what leads to element 15 -- the 16th
// smallest of the 31 -- survives the compiler.
MEL_FN int32_t hpss_bits(float v) { int32_t b; __builtin_memcpy(&b, &v, sizeof b); return b; }
MEL_FN float hpss_float(int32_t b) { float v; __builtin_memcpy(&v, &b, sizeof v); return v; }
MEL_FN void hpss_cex(int32_t& a, int32_t& b) {
  const int32_t lo = a < b ? a : b, hi = a < b ? b : a;
  a = lo; b = hi;
}
// merges the sorted halves of the N values LO, LO + R, LO + 2 R, ..
template <int LO, int N, int R>
MEL_FN void hpss_merge(int32_t* v) {
  constexpr int M = 2 * R;
  if constexpr (M < N) {
    hpss_merge<LO, N, M>(v);
    hpss_merge<LO + R, N, M>(v);
#pragma unroll
    for (int i = LO + R; i + R < LO + N; i += M) hpss_cex(v[i], v[i + R]);
  } else {
    hpss_cex(v[LO], v[LO + R]);
  }
}
template <int LO, int N>
MEL_FN void hpss_sort(int32_t* v) {
  if constexpr (N > 1) {
    hpss_sort<LO, N / 2>(v);
    hpss_sort<LO + N / 2, N / 2>(v);
    hpss_merge<LO, N, 1>(v);
  }
}
// the (r + 1)-th smallest of centre[-r STEP], .., centre[0], .., centre[r STEP].  All 31 places are read; what lies outside the
// window (whatever the tile holds there) is pushed below every value (in front) or above (behind) by one minimum or maximum
// with a number that is the same for all lanes: no branch, one instantiation for every size.
template <int STEP>
MEL_FN float hpss_median(const float* centre, int r) {
  int32_t v[32];
#pragma unroll
  for (int j = 0; j < kHpssMaxKernel; j++) {
    const int o = j - kHpssMaxKernel / 2;
    const int32_t x = hpss_bits(centre[o * STEP]);
    if (o < 0) { const int32_t cap = o < -r ? INT32_MIN : INT32_MAX; v[j] = x < cap ? x : cap; }
    else if (o > 0) { const int32_t cap = o > r ? INT32_MAX : INT32_MIN; v[j] = x > cap ? x : cap; }
    else v[j] = x;
  }
  v[31] = INT32_MAX;
  hpss_sort<0, 32>(v);
  return hpss_float(v[15]);
}

// ---- the masks (librosa.util.softmask; the engine compiles with -ffp-contract=off) ----
// x against margin rf; power 1 or 2, or 0 for +inf.  Binary64 throughout, rounded once to binary32: x^2 is exact, the
// product margin rf, its square, the sum and the quotient round once each.  unit: both margins are 1.
MEL_FN float hpss_mask(float x, float rf, double margin, int power, bool unit) {
  const double X = (double)x, R = margin * (double)rf;
  if (power == 0) return X > R ? 1.0f : 0.0f;
  if ((X > R ? X : R) < 0x1p-126) return unit ? 0.5f : 0.0f;
  const double a = power == 2 ? X * X : X, b = power == 2 ? R * R : R;
  return (float)(a / (a + b));
}
// component 0 (harmonic) and 1 (percussive) of an element from its two medians
MEL_FN void hpss_masks(float hm, float pm, const pdmp3_hpss_params& P, float* mh, float* mp) {
  const bool unit = P.margin_harm == 1.0 && P.margin_perc == 1.0;
  *mh = hpss_mask(hm, pm, P.margin_harm, P.power, unit);
  *mp = hpss_mask(pm, hm, P.margin_perc, P.power, unit);
}

// ---- a workgroup's place and a lane's element ----
// blockIdx.x = (frame tile x bin tiles + bin tile) x channels + channel
MEL_FN int hpss_bin_tiles(int bins) { return (bins + kHpssBins - 1) / kHpssBins; }
// the value of the tile's row r, column c (hpss.hip's load; the stage holds [bins][n_stage] magnitudes, mode 2 [..][2])
MEL_FN float hpss_load(const float* stage, const pdmp3_hpss_params& P, int k0, long long f0, int r, int c) {
  const int rp = P.kernel_perc / 2;
  const long long fs = f0 + c;
  if (fs >= P.n_stage) return 0.0f;
  const size_t at = (size_t)hpss_reflect(k0 - rp + r, P.bins) * (size_t)P.n_stage + (size_t)fs;
  return P.out_mode == 2 ? stft_value(stage[2 * at], stage[2 * at + 1], 0.0f, 1) : stage[at];
}
// element (bin k, frame f) of a channel: both medians from the tile, the masks, the stores.  `centre` points at the element in
// LDS; `stage` and `out` are the channel's.
MEL_FN void hpss_element(const float* centre, const float* stage, float* out, const pdmp3_hpss_params& P, int k, long long f) {
  const int rh = P.kernel_harm / 2, rp = P.kernel_perc / 2;
  const float hm = hpss_median<1>(centre, rh), pm = hpss_median<kHpssPitch>(centre, rp);
  if (f >= P.n_frames) return;
  const size_t plane = (size_t)P.bins * (size_t)P.n_frames, at = (size_t)k * (size_t)P.n_frames + (size_t)f;
  if (P.out_mode == 3) { out[at] = hm; out[plane + at] = pm; return; }
  float mh, mp;
  hpss_masks(hm, pm, P, &mh, &mp);
  if (P.out_mode == 0) { out[at] = mh; out[plane + at] = mp; return; }
  if (P.out_mode == 1) { const float s = *centre; out[at] = s * mh; out[plane + at] = s * mp; return; }
  const size_t sa = 2 * ((size_t)k * (size_t)P.n_stage + (size_t)(f + rh));
  const float re = stage[sa], im = stage[sa + 1];
  out[2 * at] = re * mh; out[2 * at + 1] = im * mh;
  out[2 * (plane + at)] = re * mp; out[2 * (plane + at) + 1] = im * mp;
}

}  // namespace pdmp3
#endif
