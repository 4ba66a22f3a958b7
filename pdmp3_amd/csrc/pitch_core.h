// pitch_core.h -- k_clip_pitch (pitch.hip) phase by phase, written per lane over a small set of
// operations `O`: LDS loads and stores by index (ldf / stf: floats, ldd / std: binary64, both counted from the start of the
// workgroup's LDS), the wave's fence (sync), v_mfma_f32_16x16x4_f32 (mfma), a vote (any), a lane exchange (shfl_xor) and a
// fence of the instruction scheduler (issued: what stands above it is issued before what stands below; nothing on the host).
// The kernel supplies them as the device's; the host build of the tests (tests/host_emul/pitch_emul.cpp) runs THE SAME code
// lane by lane on wave_emul.h's fibers over an LDS that is poisoned and bounds-checked.  A workgroup barrier lies between two
// phases.
#ifndef PDMP3_PITCH_CORE_H
#define PDMP3_PITCH_CORE_H
#include "mel_core.h"

namespace pdmp3 {

constexpr int kPitchMaxThreads = 512;       // eight waves: one frame a wave
constexpr unsigned kPitchFront = 16;        // zeros in front of the span: the B operand's lanes read up to 15 positions back
constexpr unsigned kPitchTileSkew = 288;    // pitch_at(x + 256) - pitch_at(x)
constexpr unsigned kPitchCurvePad = 8;      // floats between two waves' curves beyond 256 tiles (the store's banks)

// Position x of the span region in LDS: two floats are skipped every 16, so that the sixteen rows of the A operand -- 16
// positions apart, two k a half wave -- fall into the 32 banks of a 4-byte read once: 18 m + k mod 32 is a bijection of
// (m < 16, k < 2), and a 16-boundary between the two k moves the second by 2, which keeps it odd.  The B operand reads 17
// consecutive positions (most lanes share theirs): at most two runs, 2 apart.
MEL_FN unsigned pitch_at(unsigned x) { return x + 2u * (x >> 4); }

// the regions behind the span (pdmp3_hip.h pdmp3_pitch_params): indices in doubles (_d) and in floats (_f)
struct pitch_layout {
  unsigned q_d, t_d, u_d, curve_f, curve_stride, res_f, total_f;
};
MEL_FN pitch_layout pitch_lds(const pdmp3_pitch_params& P) {
  pitch_layout L;
  L.q_d = P.span_floats / 2;
  L.t_d = L.q_d + P.q_doubles;
  L.u_d = L.t_d + 64u * (unsigned)P.frames_wg;
  L.curve_f = 2u * (L.u_d + 64u);
  L.curve_stride = 256u * (unsigned)P.tiles + kPitchCurvePad;
  L.res_f = L.curve_f + (unsigned)P.frames_wg * L.curve_stride;
  L.total_f = L.res_f + 4u * (unsigned)P.frames_wg;
  return L;
}
// samples of the workgroup's span, and of a thread's piece of it in the scan of the squares
MEL_FN unsigned pitch_span(const pdmp3_pitch_params& P) { return P.q_doubles - 1u; }
MEL_FN unsigned pitch_piece(const pdmp3_pitch_params& P) { return (pitch_span(P) + 64u * (unsigned)P.frames_wg - 1u) / (64u * (unsigned)P.frames_wg); }

// ---- phase 1: the span, zeros outside the row, 16 zeros in front and zeros in the padding behind ----
template <class O>
MEL_FN void pitch_load(O& o, const pdmp3_pitch_params& P, const float* row, long long f0, unsigned lead, unsigned tid) {
  const unsigned nt = 64u * (unsigned)P.frames_wg, span = pitch_span(P);
  for (unsigned x = tid; x < P.ext; x += nt) {
    const unsigned p = x - kPitchFront;
    o.stf(pitch_at(x), x >= kPitchFront && p < span ? mel_sample(row, P.n_in, f0, P.hop, lead, p) : 0.0f);
  }
}

// ---- phase 2: Q[p] = z[0]^2 + .. + z[p-1]^2 in binary64 over the span (a square of a binary32 value is exact), one fixed
// order: a thread's piece left to right (2a), the pieces' sums left to right inside a lane of wave 0 and the lanes' sums left
// to right (2b), then the pieces again from their starts (2c) ----
template <class O>
MEL_FN void pitch_sq_pieces(O& o, const pdmp3_pitch_params& P, const pitch_layout& L, unsigned tid) {
  const unsigned span = pitch_span(P), piece = pitch_piece(P), lo = tid * piece, hi = lo + piece < span ? lo + piece : span;
  double s = 0.0;
  for (unsigned p = lo; p < hi; p++) { const double z = (double)o.ldf(pitch_at(p + kPitchFront)); s += z * z; }
  o.std(L.t_d + tid, s);
}
template <class O>
MEL_FN void pitch_sq_scan(O& o, const pdmp3_pitch_params& P, const pitch_layout& L, unsigned lane) {
  const unsigned fw = (unsigned)P.frames_wg, at = L.t_d + lane * fw;
  double run = 0.0;
  for (unsigned i = 0; i < fw; i++) { const double v = o.ldd(at + i); o.std(at + i, run); run += v; }
  o.std(L.u_d + lane, run);
  o.sync();
  double off = 0.0;
  for (unsigned j = 0; j < lane; j++) off += o.ldd(L.u_d + j);
  for (unsigned i = 0; i < fw; i++) o.std(at + i, off + o.ldd(at + i));
}
template <class O>
MEL_FN void pitch_sq_write(O& o, const pdmp3_pitch_params& P, const pitch_layout& L, unsigned tid) {
  const unsigned span = pitch_span(P), piece = pitch_piece(P), lo = tid * piece, hi = lo + piece < span ? lo + piece : span;
  if (lo >= span) return;
  double run = o.ldd(L.t_d + tid);
  for (unsigned p = lo; p < hi; p++) { const double z = (double)o.ldf(pitch_at(p + kPitchFront)); o.std(L.q_d + p, run); run += z * z; }
  if (hi == span) o.std(L.q_d + span, run);
}

// ---- phase 3: one frame a wave ----
template <class O>
MEL_FN int pitch_wave_min(O& o, int v) {
  for (int m = 32; m; m >>= 1) { const int w = o.shfl_xor(v, m); v = w < v ? w : v; }
  return v;
}
// d(tau) = e(0) + e(tau) - 2 r^(tau) in binary64: e from the prefix sums (qb: Q's index of the frame's first sample)
template <class O>
MEL_FN double pitch_d(O& o, unsigned qb, unsigned cw, unsigned W, double e0, unsigned tau) {
  const double e = o.ldd(qb + tau + W) - o.ldd(qb + tau);
  return (e0 + e) - 2.0 * (double)o.ldf(cw + tau);
}
template <int TILES, class O>
MEL_FN void pitch_frame(O& o, const pdmp3_pitch_params& P, const pitch_layout& L, unsigned wave, unsigned lane) {
  const unsigned j = lane & 15u, kq = lane >> 4, W = (unsigned)P.win, base = wave * (unsigned)P.hop + kPitchFront;
  const unsigned cw = L.curve_f + wave * L.curve_stride, tw = L.t_d + 64u * wave, qb = L.q_d + wave * (unsigned)P.hop;
  const int tmin = P.tmin, tmax = P.tmax;
  // r^(256 a + 16 m + n) = D[m][n] of A[m][k] = z[t_k + 16 m + 256 a], B[k][n] = z[t_k - n] inside the window, else 0: the
  // lane holds row m = j of A, column n = j of B at k = kq, and rows 4 kq + r of D at column j
  typename O::acc4 acc[TILES];
  for (int a = 0; a < TILES; a++) acc[a] = o.zero();
  {
    unsigned xa = base + kq + 16u * j, xb = base + kq - j, rel = kq - j;
    // Two sets of operand registers take turns: the operands of k-step ks + 1 are read before the matrix instructions of
    // k-step ks are issued, so a read has a k-step's matrix work to arrive in.  The last read reaches one k-step past the end
    // (the padding has room for it) and is left unused.
    float a0[TILES], a1[TILES], b0, b1;
    const auto read = [&](float* av, float& bv) {
      const unsigned sa = pitch_at(xa);
      bv = o.ldf(pitch_at(xb));
      for (int a = 0; a < TILES; a++) av[a] = o.ldf(sa + kPitchTileSkew * (unsigned)a);
    };
    const auto multiply = [&](const float* av, float bv) {
      const float b = rel < W ? bv : 0.0f;             // (rel is negative as an unsigned: out of the window too)
      for (int a = 0; a < TILES; a++) o.mfma(av[a], b, acc[a]);
      xa += 4u; xb += 4u; rel += 4u;
    };
    const auto ahead = [&](float* av, float& bv) {     // the next k-step's operands
      xa += 4u; xb += 4u;
      read(av, bv);
      xa -= 4u; xb -= 4u;
      o.issued();                                      // (the reads above are issued before the matrix instructions below)
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
  bool nz = false;
  for (unsigned p = lane; p < (unsigned)P.n; p += 64u) nz = nz || o.ldf(pitch_at(base + p)) != 0.0f;
  nz = o.any(nz);
  o.sync();
  // d, S and d' in binary64: a lane takes 4 TILES consecutive lags; S in one fixed order -- the lane's lags left to right,
  // the lanes' sums left to right; d' rounded once to binary32, in the place of r^
  {
    const unsigned c = 4u * TILES, lo = lane * c;
    const double e0 = o.ldd(qb + W) - o.ldd(qb);
    double sum = 0.0;
    for (unsigned i = 0; i < c; i++) {
      const unsigned tau = lo + i;
      if (tau >= 1u && tau <= (unsigned)tmax) sum += pitch_d(o, qb, cw, W, e0, tau);
    }
    o.std(tw + lane, sum);
    o.sync();
    double S = 0.0;
    for (unsigned l = 0; l < lane; l++) S += o.ldd(tw + l);
    for (unsigned i = 0; i < c; i++) {
      const unsigned tau = lo + i;
      if (tau > (unsigned)tmax) break;
      float dp = 1.0f;
      if (tau >= 1u) {
        const double d = pitch_d(o, qb, cw, W, e0, tau);
        S += d;
        if (S > 0.0) dp = (float)(d * (double)tau / S);
      }
      o.stf(cw + tau, dp);
    }
    o.sync();
  }
  if (P.out_mode != 0) return;
  // the decision on the binary32 curve: the smallest trough under the threshold, else the smallest lag of the minimum
  int ts = 0x7fffffff;
  for (int tau = tmin + (int)lane; tau < tmax; tau += 64) {
    const float v = o.ldf(cw + (unsigned)tau), nx = o.ldf(cw + (unsigned)tau + 1u);
    const bool trough = tau == tmin ? v < nx : (v < o.ldf(cw + (unsigned)tau - 1u) && v <= nx);
    if (trough && (double)v < P.threshold) { ts = tau; break; }
  }
  ts = pitch_wave_min(o, ts);
  if (ts == 0x7fffffff) {
    float mv = INFINITY;
    int mt = 0x7fffffff;
    for (int tau = tmin + (int)lane; tau <= tmax; tau += 64) {
      const float v = o.ldf(cw + (unsigned)tau);
      if (v < mv) { mv = v; mt = tau; }
    }
    for (int m = 32; m; m >>= 1) {
      const float wv = mel_from_bits((uint32_t)o.shfl_xor((int)mel_bits(mv), m));
      const int wt = o.shfl_xor(mt, m);
      if (wv < mv || (wv == mv && wt < mt)) { mv = wv; mt = wt; }
    }
    ts = mt;
  }
  if (lane != 0) return;
  float f0 = 0.0f, ap = 1.0f, lag = 0.0f;
  if (nz) {
    const double b = (double)o.ldf(cw + (unsigned)ts);
    double delta = 0.0;
    if (ts > tmin && ts < tmax) {
      const double a = (double)o.ldf(cw + (unsigned)ts - 1u), c = (double)o.ldf(cw + (unsigned)ts + 1u);
      const double D = (a - 2.0 * b) + c;
      if (D > 0.0) delta = (a - c) / (2.0 * D);
    }
    f0 = (float)(P.sr / ((double)ts + delta));
    ap = (float)b;
    lag = (float)ts;
  }
  o.stf(L.res_f + 4u * wave, f0);
  o.stf(L.res_f + 4u * wave + 1u, ap);
  o.stf(L.res_f + 4u * wave + 2u, lag);
}

// ---- phase 4: consecutive threads store consecutive frames of one row of the output ----
template <class O>
MEL_FN void pitch_store(O& o, const pdmp3_pitch_params& P, const pitch_layout& L, float* out, long long f0, unsigned tid) {
  const unsigned fw = (unsigned)P.frames_wg, nt = 64u * fw, rows = P.out_mode == 0 ? 3u : (unsigned)P.tmax + 1u;
  for (unsigned i = tid; i < rows * fw; i += nt) {
    const unsigned row = i / fw, fl = i % fw;
    const long long f = f0 + fl;
    if (f >= P.n_frames) continue;
    const float v = o.ldf(P.out_mode == 0 ? L.res_f + 4u * fl + row : L.curve_f + fl * L.curve_stride + row);
    out[(size_t)row * (size_t)P.n_frames + (size_t)f] = v;
  }
}

}  // namespace pdmp3
#endif
