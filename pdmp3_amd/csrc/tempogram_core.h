// tempogram_core.h -- k_clip_onset, k_clip_tempogram and k_clip_tempo (tempogram.hip) phase by phase,
// written per lane over pitch_core.h's set of operations `O` (ldf / stf / ldd / std on the workgroup's LDS by index, the wave's
// fence, v_mfma_f32_16x16x4_f32, the scheduler's fence).  The kernels supply them as the device's; the host build of the tests
// (tests/host_emul/tempogram_emul.cpp) runs THE SAME code lane by lane on wave_emul.h's fibers over an LDS that is poisoned and
// bounds-checked.  The autocorrelation is pitch_frame's matrix loop with W = Wt on a span that holds one windowed frame: the
// pattern is copied, not shared, so that k_clip_pitch's code is what it is without this file.
#ifndef PDMP3_TEMPOGRAM_CORE_H
#define PDMP3_TEMPOGRAM_CORE_H
#include "pitch_core.h"

namespace pdmp3 {

constexpr int kTempogramMaxThreads = 512;   // eight waves: one frame a wave
constexpr int kOnsetThreads = 256;          // a lane a frame
constexpr int kTempoThreads = 256;          // a thread a lag, four rounds at Wt = 1024
constexpr int kTempoMaxWin = 1024;

// ---- k_clip_onset: envelope frame e of one channel.  l: [n_mels][n_mel_frames]; the frame itself is column e + lag, its
// reference column e.  The band maximum over |m' - m| <= half with m' clamped, the rectified difference and the sum over the
// bands ascending in binary64 (a difference of two binary32 values is exact there), one rounding ----
MEL_FN float onset_value(const float* l, const pdmp3_tempogram_params& P, long long e) {
  const size_t F = (size_t)P.n_mel_frames;
  const float* const cur = l + (size_t)e + (size_t)P.lag;
  const float* const old = l + (size_t)e;
  double s = 0.0;
  for (int m = 0; m < P.n_mels; m++) {
    const int lo = m - P.half < 0 ? 0 : m - P.half, hi = m + P.half > P.n_mels - 1 ? P.n_mels - 1 : m + P.half;
    float ref = old[(size_t)lo * F];
    for (int q = lo + 1; q <= hi; q++) { const float v = old[(size_t)q * F]; ref = v > ref ? v : ref; }
    const double d = (double)cur[(size_t)m * F] - (double)ref;
    s += d > 0.0 ? d : 0.0;
  }
  return (float)((10.0 / (double)P.n_mels) * s);
}

// ---- k_clip_tempogram ----
// a workgroup's LDS in floats: frames_wg spans, then frames_wg curves
struct tempogram_layout {
  unsigned curve_f, curve_stride, total_f;
};
MEL_FN tempogram_layout tempogram_lds(const pdmp3_tempogram_params& P) {
  tempogram_layout L;
  L.curve_f = (unsigned)P.frames_wg * P.span_floats;
  L.curve_stride = 256u * (unsigned)P.tiles + kPitchCurvePad;
  L.total_f = L.curve_f + (unsigned)P.frames_wg * L.curve_stride;
  return L;
}
// positions of a wave's span that the operands reach: the A operand's last row of the last tile, one k-step behind the last
// (the loop reads a k-step ahead)
MEL_FN unsigned tempogram_ext(int win, int tiles, int ksteps) {
  const unsigned reach = 4u * (unsigned)(ksteps + 1) + 240u + 256u * (unsigned)(tiles - 1);
  return kPitchFront + (reach > (unsigned)win ? reach : (unsigned)win);
}

// One frame a wave.  env: the channel's envelope, frame f's window begins at env[f]; w: the window.
template <int TILES, class O>
MEL_FN void tempogram_frame(O& o, const pdmp3_tempogram_params& P, const tempogram_layout& L, const float* env, const float* w, long long f,
                            unsigned wave, unsigned lane) {
  const unsigned j = lane & 15u, kq = lane >> 4, W = (unsigned)P.win, sb = wave * P.span_floats, cw = L.curve_f + wave * L.curve_stride;
  // x_f, one binary32 product a sample, 16 zeros in front and zeros behind
  for (unsigned x = lane; x < P.ext; x += 64u) {
    const unsigned p = x - kPitchFront;
    o.stf(sb + pitch_at(x), x >= kPitchFront && p < W ? w[p] * env[(size_t)f + p] : 0.0f);
  }
  o.sync();
  // r^(256 a + 16 m + n) = D[m][n] of A[m][k] = x[t_k + 16 m + 256 a], B[k][n] = x[t_k - n] inside the window, else 0: the
  // lane holds row m = j of A, column n = j of B at k = kq, and rows 4 kq + r of D at column j (pitch_core.h pitch_frame)
  typename O::acc4 acc[TILES];
  for (int a = 0; a < TILES; a++) acc[a] = o.zero();
  {
    unsigned xa = kPitchFront + kq + 16u * j, xb = kPitchFront + kq - j, rel = kq - j;
    // two sets of operand registers take turns: the operands of k-step ks + 1 are read before the matrix instructions of
    // k-step ks are issued; the last read reaches one k-step past the end (the span has room for it) and is left unused
    float a0[TILES], a1[TILES], b0, b1;
    const auto read = [&](float* av, float& bv) {
      const unsigned sa = sb + pitch_at(xa);
      bv = o.ldf(sb + pitch_at(xb));
      for (int a = 0; a < TILES; a++) av[a] = o.ldf(sa + kPitchTileSkew * (unsigned)a);
    };
    const auto multiply = [&](const float* av, float bv) {
      const float b = rel < W ? bv : 0.0f;             // (rel is negative as an unsigned: out of the window too)
      for (int a = 0; a < TILES; a++) o.mfma(av[a], b, acc[a]);
      xa += 4u; xb += 4u; rel += 4u;
    };
    const auto ahead = [&](float* av, float& bv) {
      xa += 4u; xb += 4u;
      read(av, bv);
      xa -= 4u; xb -= 4u;
      o.issued();
    };
    read(a0, b0);
    int ks = 0;
    for (; ks + 2 <= P.ksteps; ks += 2) {
      ahead(a1, b1);
      multiply(a0, b0);
      ahead(a0, b0);
      multiply(a1, b1);
    }
    if (ks < P.ksteps) multiply(a0, b0);
  }
  for (int a = 0; a < TILES; a++)
    for (int r = 0; r < 4; r++) o.stf(cw + 256u * (unsigned)a + 64u * kq + 16u * (unsigned)r + j, acc[a][r]);
  o.sync();
  // T = r^(tau) / r^(0) in binary64, rounded once, in the place of r^ (every lane has r^(0) before any lane overwrites it)
  const double r0 = (double)o.ldf(cw);
  o.sync();
  for (unsigned tau = lane; tau < W; tau += 64u) o.stf(cw + tau, r0 > 0.0 ? (float)((double)o.ldf(cw + tau) / r0) : 0.0f);
}

// consecutive threads store consecutive frames of one lag's row of the output [Wt][n_frames]
template <class O>
MEL_FN void tempogram_store(O& o, const pdmp3_tempogram_params& P, const tempogram_layout& L, float* out, long long f0, unsigned tid) {
  const unsigned fw = (unsigned)P.frames_wg, nt = 64u * fw;
  for (unsigned i = tid; i < (unsigned)P.win * fw; i += nt) {
    const unsigned tau = i / fw, fl = i % fw;
    const long long f = f0 + fl;
    if (f >= P.n_frames) continue;
    out[(size_t)tau * (size_t)P.n_frames + (size_t)f] = o.ldf(L.curve_f + fl * L.curve_stride + tau);
  }
}

// ---- k_clip_tempo: one workgroup a (clip, channel).  LDS in doubles: s[Wt], then per lane of wave 0 a value and a lag ----
// a thread's lags: the mean over the frames ascending, log1p, the prior
template <class O>
MEL_FN void tempo_scores(O& o, const pdmp3_tempogram_params& P, const float* T, const double* prior, unsigned tid) {
  const size_t F = (size_t)P.n_frames;
  for (unsigned tau = tid; tau < (unsigned)P.win; tau += (unsigned)kTempoThreads) {
    const float* const row = T + (size_t)tau * F;
    double sum = 0.0;
    size_t f = 0;
    for (; f + 8 <= F; f += 8) {                         // (eight loads in flight; the additions keep their order)
      float v[8];
      for (int i = 0; i < 8; i++) v[i] = row[f + i];
      for (int i = 0; i < 8; i++) sum += (double)v[i];
    }
    for (; f < F; f++) sum += (double)row[f];
    o.std(tau, log1p(1e6 * (sum / (double)F)) + prior[tau]);
  }
}
// the largest s and the smallest lag that attains it among the lags other than `skip`, in one fixed order: a lane's lags
// ascending, then the lanes ascending (wave 0; every lane returns the same)
template <class O>
MEL_FN void tempo_best(O& o, const pdmp3_tempogram_params& P, unsigned lane, int skip, double* best, int* at) {
  const unsigned W = (unsigned)P.win, pv = W, pt = W + 64u;
  double bv = -INFINITY;
  int bt = 0x7fffffff;
  for (unsigned tau = lane; tau < W; tau += 64u) {
    const double v = o.ldd(tau);
    if ((int)tau != skip && v > bv) { bv = v; bt = (int)tau; }
  }
  o.std(pv + lane, bv);
  o.std(pt + lane, (double)bt);
  o.sync();
  bv = -INFINITY; bt = 0x7fffffff;
  for (unsigned l = 0; l < 64u; l++) {
    const double v = o.ldd(pv + l);
    const int t = (int)o.ldd(pt + l);
    if (v > bv || (v == bv && t < bt)) { bv = v; bt = t; }
  }
  o.sync();
  *best = bv; *at = bt;
}
template <class O>
MEL_FN void tempo_decide(O& o, const pdmp3_tempogram_params& P, float* out, unsigned lane) {
  double s1, s2;
  int t1, t2;
  tempo_best(o, P, lane, -1, &s1, &t1);
  tempo_best(o, P, lane, t1, &s2, &t2);
  if (lane != 0) return;
  out[0] = (float)(60.0 * P.sr / ((double)P.hop * (double)t1));
  out[1] = (float)t1;
  out[2] = (float)s1;
  out[3] = (float)(s1 - s2);
}

}  // namespace pdmp3
#endif
