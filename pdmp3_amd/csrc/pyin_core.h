// pyin_core.h -- k_clip_pyin_obs and k_clip_pyin_path (pyin.hip) phase by phase, written per lane over
// pitch_core.h's kind of operation set `O`: LDS loads and stores by index (ldf / stf: floats, ldu / stu: 32-bit words, both
// counted in words from the start of the workgroup's LDS; ldd / std: binary64, counted in doubles), the wave's fence (sync), a
// ballot, a lane exchange (shfl_xor) and the binary64 logarithm (log).  The kernels supply them as the device's; the host build
// of the tests (tests/host_emul/pyin_emul.cpp) runs THE SAME code lane by lane on wave_emul.h's fibers over an LDS that is
// poisoned and bounds-checked.  A workgroup barrier lies between two phases.
#ifndef PDMP3_PYIN_CORE_H
#define PDMP3_PYIN_CORE_H
#include "mel_core.h"

namespace pdmp3 {

constexpr int kPyinObsMaxThreads = 512;     // eight waves: one frame a wave
constexpr int kPyinPathMaxThreads = 1024;   // sixteen waves: one or two pitch bins a thread
constexpr unsigned kPyinNoBin = 0xffffffffu;

// the tables' block (include/pdmp3_hip.h): indices in doubles; f0: the index in floats of the bins' frequencies behind them
struct pyin_tables {
  unsigned theta, w, wsum, g, cn, t, ltri, lz, doubles, f0;
};
MEL_FN pyin_tables pyin_table_layout(const pdmp3_pyin_params& P) {
  pyin_tables T;
  const unsigned nt = (unsigned)P.n_thr, nb = (unsigned)P.n_bins, mt = (unsigned)P.max_troughs;
  T.theta = 0;
  T.w = T.theta + nt;
  T.wsum = T.w + nt;
  T.g = T.wsum + nt + 1u;
  T.cn = T.g + mt;
  T.t = T.cn + mt + 1u;
  T.ltri = T.t + nb;
  T.lz = T.ltri + 2u * (unsigned)P.hb + 1u;
  T.doubles = T.lz + nb;
  T.f0 = 2u * T.doubles;
  return T;
}
MEL_FN size_t pyin_table_bytes(const pdmp3_pyin_params& P) { return (size_t)pyin_table_layout(P).doubles * 8u + (size_t)P.n_bins * 4u; }

// ---- k_clip_pyin_obs ----
// a wave's LDS, in words: its curve (tmax + 1), its observation row with v behind it (n_bins + 1), the troughs under every
// threshold in the frame and so far (n_thr each), 64 words of the lanes' bins; every part an even number of words
struct pyin_obs_layout {
  unsigned cw, ow, nt, stride;
};
MEL_FN pyin_obs_layout pyin_obs_lds(const pdmp3_pyin_params& P) {
  pyin_obs_layout L;
  L.cw = ((unsigned)P.tmax + 2u) & ~1u;
  L.ow = ((unsigned)P.n_bins + 2u) & ~1u;
  L.nt = ((unsigned)P.n_thr + 1u) & ~1u;
  L.stride = L.cw + L.ow + 2u * L.nt + 64u;
  return L;
}
MEL_FN unsigned pyin_obs_lds_bytes(const pdmp3_pyin_params& P, int frames) { return (unsigned)frames * pyin_obs_lds(P).stride * 4u; }

MEL_FN unsigned pyin_popc(unsigned long long m) { return (unsigned)__builtin_popcountll(m); }
MEL_FN unsigned pyin_ctz(unsigned long long m) { return (unsigned)__builtin_ctzll(m); }

// phase 1: the workgroup's curves, consecutive threads reading consecutive frames of a lag's row
template <class O>
MEL_FN void pyin_obs_load(O& o, const pdmp3_pyin_params& P, const float* curve, long long f0, unsigned tid) {
  const pyin_obs_layout L = pyin_obs_lds(P);
  const unsigned fw = (unsigned)P.frames_wg, nt = 64u * fw, rows = (unsigned)P.tmax + 1u;
  for (unsigned i = tid; i < rows * fw; i += nt) {
    const unsigned row = i / fw, fl = i % fw;
    const long long f = f0 + fl;
    if (f >= P.n_frames) continue;
    o.stf(fl * L.stride + row, curve[(size_t)row * (size_t)P.n_frames + (size_t)f]);
  }
}

// rule 2 and rule 4's i_j at lag tau of the wave's curve: is it a trough, its height, the least i with h < theta_i (n_thr + 1:
// none).  The comparison is the binary32 value's against the binary64 table entry.
template <class O>
MEL_FN bool pyin_trough(O& o, const pdmp3_pyin_params& P, const double* theta, unsigned cw, int tau, float& h, int& ij) {
  h = 0.0f;
  ij = P.n_thr + 1;
  if (tau >= P.tmax) return false;
  const float v = o.ldf(cw + (unsigned)tau), nx = o.ldf(cw + (unsigned)tau + 1u);
  const bool trough = tau == P.tmin ? v < nx : (v < o.ldf(cw + (unsigned)tau - 1u) && v <= nx);
  if (!trough) return false;
  h = v;
  const double hd = (double)v;
  int lo = 1, hi = P.n_thr + 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (hd < theta[mid - 1]) hi = mid; else lo = mid + 1;
  }
  ij = lo;
  return true;
}

// phase 2: one frame a wave, rules 2 to 6.  The lags go in passes of 64, a lane a lag.  Sweep 1 counts the troughs under every
// threshold (n_i) and finds the first lowest trough; sweep 2 has n_i, so a trough's place under a threshold is the count of
// the passes before (carried in LDS) plus the prefix count of the ballot, and its probability is summed over the thresholds in
// ascending order.  A bin's entry is written by the trough of the largest lag that falls into it: inside a pass a lane stands
// back when a lane above it has the same bin, and a later pass writes over an earlier one.
template <class O>
MEL_FN void pyin_obs_frame(O& o, const pdmp3_pyin_params& P, const double* tab, unsigned wave, unsigned lane) {
  const pyin_tables T = pyin_table_layout(P);
  const pyin_obs_layout L = pyin_obs_lds(P);
  const unsigned cw = wave * L.stride, ow = cw + L.cw, tot = ow + L.ow, run = tot + L.nt, sb = run + L.nt;
  const int tmin = P.tmin, tmax = P.tmax, nt = P.n_thr, nb = P.n_bins;
  const int passes = (tmax - tmin + 63) / 64;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (unsigned i = lane; i < L.ow + 2u * L.nt; i += 64u) o.stu(ow + i, 0u);
  o.sync();
  float hmin = INFINITY;
  int tg = 0x7fffffff;
  for (int ps = 0; ps < passes; ps++) {
    const int tau = tmin + 64 * ps + (int)lane;
    float h;
    int ij;
    const bool trough = pyin_trough(o, P, tab + T.theta, cw, tau, h, ij);
    if (trough && h < hmin) { hmin = h; tg = tau; }
    if (!o.ballot(trough)) continue;
    for (int i = 1; i <= nt; i++) {
      const unsigned long long m = o.ballot(trough && ij <= i);
      if (lane == 0u && m) o.stu(tot + (unsigned)i - 1u, o.ldu(tot + (unsigned)i - 1u) + pyin_popc(m));
    }
  }
  for (int m = 32; m; m >>= 1) {
    const float wh = mel_from_bits((uint32_t)o.shfl_xor((int)mel_bits(hmin), m));
    const int wt = o.shfl_xor(tg, m);
    if (wh < hmin || (wh == hmin && wt < tg)) { hmin = wh; tg = wt; }
  }
  o.sync();
  for (int ps = 0; ps < passes; ps++) {
    const int tau = tmin + 64 * ps + (int)lane;
    float h;
    int ij;
    const bool trough = pyin_trough(o, P, tab + T.theta, cw, tau, h, ij);
    if (!o.ballot(trough)) continue;
    double pj = 0.0;
    for (int i = 1; i <= nt; i++) {
      const unsigned before = o.ldu(run + (unsigned)i - 1u);
      const bool in = trough && ij <= i;
      const unsigned long long m = o.ballot(in);
      if (in) {
        const unsigned p = before + pyin_popc(m & below), n = o.ldu(tot + (unsigned)i - 1u);
        const double prior = tab[T.g + p] * tab[T.cn + n];
        pj += tab[T.w + (unsigned)i - 1u] * prior;
      }
      if (lane == 0u && m) o.stu(run + (unsigned)i - 1u, before + pyin_popc(m));
    }
    if (trough && tau == tg) pj += P.no_trough * tab[T.wsum + (unsigned)ij - 1u];
    unsigned bin = kPyinNoBin;
    if (trough && pj != 0.0) {
      double delta = 0.0;
      if (tau > tmin) {
        const double a = (double)o.ldf(cw + (unsigned)tau - 1u), b = (double)h, c = (double)o.ldf(cw + (unsigned)tau + 1u);
        const double D = (a - 2.0 * b) + c;
        if (D > 0.0) delta = (a - c) / (2.0 * D);
      }
      const double period = (double)tau + delta;
      int lo = 0, hi = nb;                            // T_q falls with q: the count of the q with period <= T_q
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (period <= tab[T.t + (unsigned)mid]) lo = mid + 1; else hi = mid;
      }
      if (lo < nb) bin = (unsigned)lo;
    }
    o.stu(sb + lane, bin);
    o.sync();
    const unsigned long long sm = o.ballot(bin != kPyinNoBin);
    if (bin != kPyinNoBin) {
      bool stands = true;
      for (unsigned long long up = lane == 63u ? 0ull : sm >> (lane + 1u) << (lane + 1u); up && stands; up &= up - 1ull)
        stands = o.ldu(sb + pyin_ctz(up)) != bin;
      if (stands) o.stf(ow + bin, (float)pj);
    }
    o.sync();
  }
  // v: the row's sum in ascending order of the bins, in binary64 (a zero entry adds nothing: it is skipped)
  double s = 0.0;
  for (unsigned b0 = 0; b0 < (unsigned)nb; b0 += 64u) {
    const unsigned b = b0 + lane;
    const float x = b < (unsigned)nb ? o.ldf(ow + b) : 0.0f;
    for (unsigned long long m = o.ballot(x != 0.0f); m; m &= m - 1ull) s += (double)o.ldf(ow + b0 + pyin_ctz(m));
  }
  if (lane == 0u) o.stf(ow + (unsigned)nb, (float)(s < 1.0 ? s : 1.0));
}

// phase 3: mode 1: consecutive threads store consecutive frames of a bin's row of [n_bins + 1][F]; mode 0: the rows of the
// frames one behind the other, [F][n_bins + 1], as k_clip_pyin_path reads them
template <class O>
MEL_FN void pyin_obs_store(O& o, const pdmp3_pyin_params& P, float* out, long long f0, unsigned tid) {
  const pyin_obs_layout L = pyin_obs_lds(P);
  const unsigned fw = (unsigned)P.frames_wg, nt = 64u * fw, rows = (unsigned)P.n_bins + 1u;
  for (unsigned i = tid; i < rows * fw; i += nt) {
    const unsigned row = P.out_mode == 1 ? i / fw : i % rows, fl = P.out_mode == 1 ? i % fw : i / rows;
    const long long f = f0 + fl;
    if (f >= P.n_frames) continue;
    const float v = o.ldf(fl * L.stride + L.cw + row);
    if (P.out_mode == 1) out[(size_t)row * (size_t)P.n_frames + (size_t)f] = v;
    else out[(size_t)f * (size_t)rows + (size_t)row] = v;
  }
}

// ---- k_clip_pyin_path ----
// the workgroup's LDS, in doubles: the states' values V[2][2 n_bins] and V - lZ, A[2][2 n_bins], both double-buffered over the
// frames; the waves' maxima of the two halves, pv[2][2][16], and behind them their states as words, pk[2][2][16]; the window's
// logarithms ltri[2 hb + 1], which every step of every thread reads
struct pyin_path_layout {
  unsigned v_d, a_d, pv_d, pk_w, lt_d, total_d;
};
MEL_FN pyin_path_layout pyin_path_lds(const pdmp3_pyin_params& P) {
  pyin_path_layout L;
  const unsigned nb = (unsigned)P.n_bins;
  L.v_d = 0;
  L.a_d = 4u * nb;
  L.pv_d = 8u * nb;
  L.pk_w = 2u * (L.pv_d + 64u);
  L.lt_d = L.pv_d + 64u + 32u;
  L.total_d = L.lt_d + 2u * (unsigned)P.hb + 1u;
  return L;
}
MEL_FN unsigned pyin_path_threads(int n_bins) {
  const unsigned t = ((unsigned)n_bins + 63u) & ~63u;
  return t > (unsigned)kPyinPathMaxThreads ? (unsigned)kPyinPathMaxThreads : t;
}

template <class O>
MEL_FN double pyin_shfl_d(O& o, double v, int m) {
  uint64_t u;
  memcpy(&u, &v, 8);
  const uint32_t lo = (uint32_t)o.shfl_xor((int)(uint32_t)u, m), hi = (uint32_t)o.shfl_xor((int)(uint32_t)(u >> 32), m);
  u = (uint64_t)hi << 32 | lo;
  memcpy(&v, &u, 8);
  return v;
}
// the larger value, and of two equal ones the lower state: one fixed order whatever the lanes' and the waves' turn
MEL_FN void pyin_take(double x, unsigned k, double& v, unsigned& idx) {
  if (x > v || (x == v && k < idx)) { v = x; idx = k; }
}

// before the first frame: the window's logarithms into LDS
template <class O>
MEL_FN void pyin_path_window(O& o, const pdmp3_pyin_params& P, const double* tab, unsigned tid) {
  const pyin_tables T = pyin_table_layout(P);
  const pyin_path_layout L = pyin_path_lds(P);
  for (unsigned i = tid; i < 2u * (unsigned)P.hb + 1u; i += (unsigned)P.path_threads) o.std(L.lt_d + i, tab[T.ltri + i]);
}

// Frame f of the workgroup's (clip, channel): every thread's bins j = tid, tid + threads.  obs: the frame's row [n_bins + 1];
// bp: the frame's back-pointers [2 n_bins].  Reads buffer (f & 1) ^ 1 and the maxima the waves left there, writes buffer f & 1.
template <class O>
MEL_FN void pyin_path_step(O& o, const pdmp3_pyin_params& P, const double* tab, const float* obs, uint16_t* bp, long long f, unsigned tid) {
  const pyin_tables T = pyin_table_layout(P);
  const pyin_path_layout L = pyin_path_lds(P);
  const unsigned nb = (unsigned)P.n_bins, nthreads = (unsigned)P.path_threads, lane = tid & 63u, wave = tid >> 6, nw = nthreads >> 6;
  const unsigned wr = (unsigned)(f & 1), rd = wr ^ 1u;
  const unsigned Vw = L.v_d + wr * 2u * nb, Aw = L.a_d + wr * 2u * nb, Ar = L.a_d + rd * 2u * nb;
  const int hb = P.hb;
  const double NEG = -INFINITY;
  const double U = (1.0 - (double)obs[nb]) / (double)nb;
  const double lou = U > 0.0 ? o.log(U) : P.l0;
  double jump = NEG;
  unsigned jk = 0;
  if (f > 0) {
    jk = kPyinNoBin;
    for (unsigned i = 0; i < 2u; i++)
      for (unsigned w = 0; w < nw; w++) pyin_take(o.ldd(L.pv_d + rd * 32u + i * 16u + w), o.ldu(L.pk_w + rd * 32u + i * 16u + w), jump, jk);
    jump += P.l0;
  }
  double tv = NEG, tu = NEG;
  unsigned kvb = kPyinNoBin, kub = kPyinNoBin;
  for (unsigned j = tid; j < nb; j += nthreads) {
    const float ob = obs[j];
    const double lov = ob != 0.0f ? o.log((double)ob) : P.l0;
    double nv, nu;
    if (f == 0) {
      nv = P.l0 + lov;
      nu = P.lp0_u + lou;
    } else {
      double mv = NEG, mu = NEG;
      unsigned kv = 0, ku = 0;
      // (a lane whose k lies outside the bins reads its own bin instead and takes nothing: the reads do not depend on the test)
#pragma unroll 4
      for (int d = -hb; d <= hb; d++) {
        const int k = (int)j + d;
        const bool in = k >= 0 && k < (int)nb;
        const unsigned kk = in ? (unsigned)k : j;
        const double t = o.ldd(L.lt_d + (unsigned)(hb - d));            // (the target lies -d from k; -inf where the window holds 0)
        const double cv = o.ldd(Ar + kk) + t, cu = o.ldd(Ar + nb + kk) + t;
        if (in && cv > mv) { mv = cv; kv = kk; }
        if (in && cu > mu) { mu = cu; ku = kk; }
      }
      double best = mv + P.l_stay;
      unsigned from = kv;
      if (mu + P.l_sw > best) { best = mu + P.l_sw; from = nb + ku; }
      if (jump > best) { best = jump; from = jk; }
      nv = lov + best;
      bp[j] = (uint16_t)from;
      best = mv + P.l_sw;
      from = kv;
      if (mu + P.l_stay > best) { best = mu + P.l_stay; from = nb + ku; }
      if (jump > best) { best = jump; from = jk; }
      nu = lou + best;
      bp[nb + j] = (uint16_t)from;
    }
    const double lz = tab[T.lz + j];
    o.std(Vw + j, nv);
    o.std(Vw + nb + j, nu);
    o.std(Aw + j, nv - lz);
    o.std(Aw + nb + j, nu - lz);
    pyin_take(nv, j, tv, kvb);
    pyin_take(nu, nb + j, tu, kub);
  }
  for (int m = 32; m; m >>= 1) {
    const double xv = pyin_shfl_d(o, tv, m), xu = pyin_shfl_d(o, tu, m);
    const unsigned yv = (unsigned)o.shfl_xor((int)kvb, m), yu = (unsigned)o.shfl_xor((int)kub, m);
    pyin_take(xv, yv, tv, kvb);
    pyin_take(xu, yu, tu, kub);
  }
  if (lane == 0u) {
    o.std(L.pv_d + wr * 32u + wave, tv);
    o.stu(L.pk_w + wr * 32u + wave, kvb);
    o.std(L.pv_d + wr * 32u + 16u + wave, tu);
    o.stu(L.pk_w + wr * 32u + 16u + wave, kub);
  }
}

// behind the last frame, one thread: the best final state, the lowest of equal ones, and the walk back; the path's state of
// frame f goes to the first back-pointer of frame f, which nothing reads any more
template <class O>
MEL_FN void pyin_path_back(O& o, const pdmp3_pyin_params& P, uint16_t* bp) {
  const pyin_path_layout L = pyin_path_lds(P);
  const unsigned nb = (unsigned)P.n_bins, Vr = L.v_d + (unsigned)((P.n_frames - 1) & 1) * 2u * nb;
  double best = -INFINITY;
  unsigned s = 0;
  for (unsigned k = 0; k < 2u * nb; k++) {
    const double x = o.ldd(Vr + k);
    if (x > best) { best = x; s = k; }
  }
  for (long long f = (long long)P.n_frames - 1; f >= 0; f--) {
    uint16_t* const row = bp + (size_t)f * 2u * nb;
    const unsigned from = f > 0 ? row[s] : 0u;
    row[0] = (uint16_t)s;
    s = from;
  }
}

// the four planes, consecutive threads storing consecutive frames
MEL_FN void pyin_path_store(const pdmp3_pyin_params& P, const double* tab, const float* obs, const uint16_t* bp, float* out, unsigned tid) {
  const pyin_tables T = pyin_table_layout(P);
  const float* const f0 = reinterpret_cast<const float*>(tab) + T.f0;
  const unsigned nb = (unsigned)P.n_bins;
  const size_t F = (size_t)P.n_frames;
  for (size_t f = tid; f < F; f += (size_t)P.path_threads) {
    const unsigned s = bp[f * 2u * nb];
    const bool voiced = s < nb;
    const unsigned b = voiced ? s : s - nb;
    out[f] = voiced || P.use_bin ? f0[b] : P.fill;
    out[F + f] = voiced ? 1.0f : 0.0f;
    out[2u * F + f] = obs[f * (nb + 1u) + nb];
    out[3u * F + f] = (float)b;
  }
}

}  // namespace pdmp3
#endif
