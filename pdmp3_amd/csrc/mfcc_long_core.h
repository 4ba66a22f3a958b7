// mfcc_long_core.h -- the phases of the kernels of mfcc_long.hip: the dB value of a log-mel value, the
// plane's threshold, the two LDS planes of a workgroup of k_clip_mfcc_long and the delta stencil.  One source for the kernels
// and for the host build the tests compile with g++ (tests/host_emul/mfcc_long_emul.cpp).  The product T d itself runs on the
// matrix instruction (mfcc_long.hip); the host build restates it as the chain of fused multiply-adds it is.
#ifndef PDMP3_MFCC_LONG_CORE_H
#define PDMP3_MFCC_LONG_CORE_H
#include "mel_core.h"

namespace pdmp3 {

constexpr int kMfccLongThreads = 256;       // four waves
constexpr int kMfccLongFrames = 64;         // the tile of a workgroup: a lane a frame
constexpr int kMfccLongMaxHalo = 8;         // (17 - 1) / 2: the widest stencil's reach
constexpr int kDbMaxThreads = 1024;         // k_clip_db_max: sixteen waves, one workgroup a plane
constexpr int kDbElems = 1024;              // k_clip_db: elements of a workgroup

// ---- the values (the engine compiles with -ffp-contract=off: every operation here is one binary32 rounding) ----
MEL_FN float mfcc_long_db(float l) { return 10.0f * l; }
MEL_FN float mfcc_long_threshold(float mx, float top_db) { return mx - top_db; }
// thr is -inf without top_db; d0 is finite (the log-mel's floor is positive), so the maximum is one of its arguments
MEL_FN float mfcc_long_clamp(float d0, float thr) { return fmaxf(d0, thr); }

// ---- LDS: the two planes of a workgroup ----
// Both are laid out for the widest halo whatever the call's is, so the pitches are constants:
//   D [mels16][80]: d of band m at column c, the tile's frame c - h (stage frame f0 + c); the columns a call loads are
//     cols16 = 64 + 2 h rounded up to 16 (64 or 80); bands from n_mels on and frames behind the stage hold zeros;
//   C [ceps16][84] behind it: the cepstrum q of the same column.
// A 4-byte access is served 32 lanes at a time over 32 banks.
//   the load writes D at m 80 + lane (+ 64)                    -- consecutive floats: every bank once;
//   the matrix instruction's B fragment reads D at (k + kq) 80 + col0 + j, a half wave j = 0 .. 15 and two values of kq:
//     80 = 16 mod 32, so the two runs of 16 fall on the two halves of the banks -- every bank once;
//   its result goes to C at (q0 + 4 kq + r) 84 + col0 + j: 4 x 84 = 16 mod 32, the same picture -- every bank once;
//   the stencil reads C at q 84 + lane + j                     -- consecutive floats: every bank once.
// So the C plane's pad is 4: any pitch = 4 mod 8 serves the result's writes, and the stencil does not care.
constexpr int kMfccLongDPitch = kMfccLongFrames + 2 * kMfccLongMaxHalo;
constexpr int kMfccLongCPad = 4;
constexpr int kMfccLongCPitch = kMfccLongDPitch + kMfccLongCPad;
MEL_FN unsigned mfcc_long_d_at(int m, int c) { return (unsigned)(m * kMfccLongDPitch + c); }
MEL_FN unsigned mfcc_long_c_at(int mels16, int q, int c) { return (unsigned)(mels16 * kMfccLongDPitch + q * kMfccLongCPitch + c); }
MEL_FN unsigned mfcc_long_lds_floats(int mels16, int ceps16) { return (unsigned)(mels16 * kMfccLongDPitch + ceps16 * kMfccLongCPitch); }
// the columns a call's tile loads and multiplies
MEL_FN int mfcc_long_cols16(int halo) { return (kMfccLongFrames + 2 * halo + 15) & ~15; }
// the lanes' fragment addresses of the matrix instruction (lane = (j = l & 15, kq = l >> 4)) at step k, column tile col0, and
// where element r of its result goes
MEL_FN unsigned mfcc_long_b_at(int k, int kq, int col0, int j) { return mfcc_long_d_at(k + kq, col0 + j); }
MEL_FN unsigned mfcc_long_result_at(int mels16, int q0, int kq, int r, int col0, int j) { return mfcc_long_c_at(mels16, q0 + 4 * kq + r, col0 + j); }

// the value of row m, column c of the tile at stage frame f0: d, or zero outside the bands and behind the stage
MEL_FN float mfcc_long_load(const float* stage, const pdmp3_mfcc_long_params& P, long long f0, int m, int c, float thr) {
  const long long fs = f0 + c;
  if (m >= P.n_mels || fs >= P.n_stage) return 0.0f;
  return mfcc_long_clamp(mfcc_long_db(stage[(size_t)m * (size_t)P.n_stage + (size_t)fs]), thr);
}

// ---- the deltas ----
// `at` points at cepstrum q of the frame's column - h: the 2 h + 1 values of the stencil are consecutive floats.  One chain of
// binary64 fused multiply-adds, j ascending, rounded once.
MEL_FN float mfcc_long_stencil(const float* at, const double* taps, int w) {
  double s = 0.0;
  for (int j = 0; j < w; j++) s = __builtin_fma(taps[j], (double)at[j], s);
  return (float)s;
}
// what a lane stores for cepstrum q of frame f (local column `lane`); `plane` is the C plane in LDS, `out` the channel's rows
MEL_FN void mfcc_long_store(const float* plane_q, float* out, const pdmp3_mfcc_long_params& P, int q, int lane, long long f) {
  if (f >= P.n_frames) return;
  const size_t F = (size_t)P.n_frames, at = (size_t)q * F + (size_t)f;
  const int w = 2 * P.halo + 1;
  out[at] = plane_q[lane + P.halo];
  if (P.deltas >= 1) out[(size_t)P.n_mfcc * F + at] = mfcc_long_stencil(plane_q + lane, P.taps[0], w);
  if (P.deltas >= 2) out[2 * (size_t)P.n_mfcc * F + at] = mfcc_long_stencil(plane_q + lane, P.taps[1], w);
}

}  // namespace pdmp3
#endif
