// beat_core.h -- k_clip_beat_score, k_clip_beat_dp and k_clip_beat_pick (beat.hip) phase by phase,
// written per thread over pitch_core.h's set of operations `O` (ldu / stu / ldd / std on the workgroup's LDS by index, the
// wave's shuffle).  The kernels supply them as the device's and put a workgroup barrier between two phases; the host build of
// the tests (tests/host_emul/beat_emul.cpp) runs THE SAME code thread by thread, the phase that shuffles on wave_emul.h's
// fibers, over an LDS that is poisoned and bounds-checked.  Every binary64 operation here is rounded once: this file is
// compiled with floating-point contraction off on both sides.
#ifndef PDMP3_BEAT_CORE_H
#define PDMP3_BEAT_CORE_H
#include "pitch_core.h"

namespace pdmp3 {

constexpr int kBeatThreads = 256;           // of every workgroup of the three kernels
constexpr int kBeatMaxPeriod = 1023;        // P: the LDS of the ring and the tables is planned for it
constexpr int kBeatMaxFrames = 32768;       // F: the local maxima's values of a clip lie in one stage, the blocks' sums in LDS
constexpr int kBeatBlock = 64;              // frames of a block of the two sums
constexpr int kBeatTile = 256;              // frames of a tile of the local score: a thread a frame

// h = max(1, round-half-even(P / 2))
MEL_FN int beat_half(int P) {
  int h = P >> 1;
  if (P & 1) h += h & 1;
  return h < 1 ? 1 : h;
}
// doubles of the tables' block in front of P's g[0 .. P] (tx[0 .. 2 P] follows it): the periods p_min .. P - 1, 3 p + 2 each
MEL_FN size_t beat_table_at(int p_min, int P) {
  return (size_t)(3 * ((long long)P * (P - 1) - (long long)p_min * (p_min - 1)) / 2 + 2 * (long long)(P - p_min));
}
MEL_FN size_t beat_table_doubles(int p_min, int p_max) { return beat_table_at(p_min, p_max + 1); }

// a (clip, channel)'s scratch: hdr[8] doubles | cum[F] | lmv[F] doubles, then 32-bit words ls[F] | back[F] | bt[F]
// hdr: the tempo call's four floats in [0], [1]; [2] the norm; [3] 1.0 where the tracker runs, else 0.0
struct beat_work {
  unsigned cum, lmv;          // in doubles
  unsigned ls, back, bt;      // in words
  unsigned total_d;
};
MEL_FN beat_work beat_work_of(int F) {
  beat_work w;
  const unsigned f = (unsigned)F;
  w.cum = 8u; w.lmv = 8u + f;
  w.ls = 2u * (8u + 2u * f); w.back = w.ls + f; w.bt = w.back + f;
  w.total_d = 8u + 2u * f + (3u * f + 1u) / 2u;
  return w;
}

// the LDS of k_clip_beat_score in doubles: g[p_max + 1] | z[tile + 2 p_max] | bs[blocks of F]
struct beat_score_layout { unsigned g, z, bs, total_d; };
MEL_FN beat_score_layout beat_score_lds(int p_max, int F) {
  beat_score_layout L;
  L.g = 0u; L.z = (unsigned)p_max + 1u; L.bs = L.z + (unsigned)kBeatTile + 2u * (unsigned)p_max;
  L.total_d = L.bs + ((unsigned)F + (unsigned)kBeatBlock - 1u) / (unsigned)kBeatBlock + 1u;
  return L;
}
// ... of k_clip_beat_dp: ring[2 p_max + h(p_max)] | tx[2 p_max + 1] | red[threads]
struct beat_dp_layout { unsigned ring, tx, red, total_d; };
MEL_FN beat_dp_layout beat_dp_lds(int p_max) {
  beat_dp_layout L;
  L.ring = 0u; L.tx = 2u * (unsigned)p_max + (unsigned)beat_half(p_max); L.red = L.tx + 2u * (unsigned)p_max + 1u;
  L.total_d = L.red + (unsigned)kBeatThreads;
  return L;
}
// ... of k_clip_beat_pick: sc[8] doubles, then the words cnt[threads] | last[threads]
constexpr unsigned kBeatPickCnt = 16u, kBeatPickLast = 16u + (unsigned)kBeatThreads, kBeatPickWords = 16u + 2u * (unsigned)kBeatThreads;

// the period of a (clip, channel): the call's, or the tempo call's tau* where it is one the tables hold; else 0
MEL_FN int beat_period(const pdmp3_beat_params& P, const double* hdr) {
  if (P.period > 0) return P.period;
  const float tau = reinterpret_cast<const float*>(hdr)[1];
  if (!(tau >= (float)P.p_min) || !(tau <= (float)P.p_max)) return 0;
  return (int)tau;
}
MEL_FN float beat_bpm(const pdmp3_beat_params& P, const double* hdr) { return P.period > 0 ? P.bpm : reinterpret_cast<const float*>(hdr)[0]; }

// ---- k_clip_beat_score ----
// pass 0: g into LDS and the blocks' sums of o; pass 1: the blocks' sums of (o - m)^2.  A thread a block, a block ascending.
template <class O>
MEL_FN void beat_score_sums(O& o, const beat_score_layout& L, const float* env, int n, int Pd, const double* g, double m, int pass, unsigned tid) {
  if (pass == 0) for (unsigned k = tid; k <= (unsigned)Pd; k += (unsigned)kBeatThreads) o.std(L.g + k, g[k]);
  const unsigned nb = ((unsigned)n + (unsigned)kBeatBlock - 1u) / (unsigned)kBeatBlock;
  for (unsigned b = tid; b < nb; b += (unsigned)kBeatThreads) {
    const unsigned f0 = b * (unsigned)kBeatBlock, f1 = f0 + (unsigned)kBeatBlock < (unsigned)n ? f0 + (unsigned)kBeatBlock : (unsigned)n;
    double s = 0.0;
    if (pass == 0) for (unsigned f = f0; f < f1; f++) s = s + (double)env[f];
    else for (unsigned f = f0; f < f1; f++) { const double d = (double)env[f] - m; s = s + d * d; }
    o.std(L.bs + b, s);
  }
}
// the blocks' sums ascending (every thread forms the same value)
template <class O>
MEL_FN double beat_score_total(O& o, const beat_score_layout& L, int n) {
  const unsigned nb = ((unsigned)n + (unsigned)kBeatBlock - 1u) / (unsigned)kBeatBlock;
  double s = 0.0;
  for (unsigned b = 0; b < nb; b++) s = s + o.ldd(L.bs + b);
  return s;
}
MEL_FN bool beat_norm_ok(double norm) { return norm > 0.0 && norm < INFINITY; }
// z of the frames t0 - Pd .. t0 + tile - 1 + Pd into LDS, zeros outside 0 .. n - 1
template <class O>
MEL_FN void beat_score_load(O& o, const beat_score_layout& L, const float* env, int n, int Pd, double norm, int t0, unsigned tid) {
  const unsigned span = (unsigned)kBeatTile + 2u * (unsigned)Pd;
  for (unsigned q = tid; q < span; q += (unsigned)kBeatThreads) {
    const int j = t0 - Pd + (int)q;
    o.std(L.z + q, j >= 0 && j < n ? (double)env[j] / norm : 0.0);
  }
}
// frame t0 + tid: the taps ascending in j, one product and one sum each, one rounding to binary32
template <class O>
MEL_FN float beat_score_frame(O& o, const beat_score_layout& L, int Pd, unsigned tid) {
  double s = 0.0;
  for (int k = 0; k <= 2 * Pd; k++) {
    const double p = o.ldd(L.z + tid + (unsigned)k) * o.ldd(L.g + (unsigned)(k < Pd ? Pd - k : k - Pd));
    s = s + p;
  }
  return (float)s;
}

// ---- k_clip_beat_dp ----
// tx into LDS and a thread's largest ls
template <class O>
MEL_FN void beat_dp_head(O& o, const beat_dp_layout& L, const double* tx, const float* ls, int n, int Pd, unsigned tid) {
  for (unsigned d = tid; d <= 2u * (unsigned)Pd; d += (unsigned)kBeatThreads) o.std(L.tx + d, tx[d]);
  float mx = -INFINITY;
  for (unsigned i = tid; i < (unsigned)n; i += (unsigned)kBeatThreads) mx = ls[i] > mx ? ls[i] : mx;
  o.std(L.red + tid, (double)mx);
}
// the largest (smallest) of what the threads left
template <class O>
MEL_FN double beat_dp_red(O& o, const beat_dp_layout& L, bool largest) {
  double v = o.ldd(L.red);
  for (unsigned t = 1; t < (unsigned)kBeatThreads; t++) { const double w = o.ldd(L.red + t); if (largest ? w > v : w < v) v = w; }
  return v;
}
// a thread's first frame with ls >= 0.01 max ls, or n
template <class O>
MEL_FN void beat_dp_first(O& o, const beat_dp_layout& L, const float* ls, int n, double mx, unsigned tid) {
  const double thr = 0.01 * mx;
  unsigned at = (unsigned)n;
  for (unsigned i = tid; i < (unsigned)n; i += (unsigned)kBeatThreads) if ((double)ls[i] >= thr) { at = i; break; }
  o.std(L.red + tid, (double)at);
}
MEL_FN unsigned beat_dp_lanes(int h) {      // lanes of a frame: the largest power of two <= threads / h, 1 .. 64
  unsigned l = 64u;
  while (l > 1u && l * (unsigned)h > (unsigned)kBeatThreads) l >>= 1;
  return l;
}
// The frames s0 .. s0 + h - 1: lw lanes of a wave a frame, a lane's candidates d = h + q, h + q + lw, .. ascending with a strict
// comparison, then the lanes' bests in a butterfly under one total order (the larger value, of equal ones the smaller d): every
// order of the reduction gives the same.  The frames of a step read cum[s0 - 2 P .. s0 - 1] and write cum[s0 .. s0 + h - 1]:
// 2 P + h consecutive frames, distinct places of the ring.  Every lane of a wave runs every shuffle.
template <class O>
MEL_FN void beat_dp_step(O& o, const pdmp3_beat_params& P, const beat_dp_layout& L, int Pd, int n, int i0, int s0, const float* ls, double* cum,
                         int* back, float* dst, unsigned tid) {
  const int h = beat_half(Pd), R = 2 * Pd + h, pos = s0 % R;
  const unsigned lw = beat_dp_lanes(h), fp = (unsigned)kBeatThreads / lw;
  const int slot = (int)(tid / lw), q = (int)(tid % lw);
  for (int j0 = 0; j0 < h; j0 += (int)fp) {
    const int j = j0 + slot, i = s0 + j;
    const bool active = j < h && i < n;
    const float lsv = active && q == 0 ? ls[i] : 0.0f;
    double bv = -INFINITY;
    int bd = 0;
    if (active) {
      const int dmax = 2 * Pd < i ? 2 * Pd : i;
      for (int d = h + q; d <= dmax; d += (int)lw) {
        int sl = pos + j - d;
        if (sl < 0) sl += R;
        const double v = o.ldd(L.ring + (unsigned)sl) + o.ldd(L.tx + (unsigned)d);
        if (v > bv) { bv = v; bd = d; }
      }
    }
    for (unsigned m = 1; m < lw; m <<= 1) {
      uint64_t u;
      memcpy(&u, &bv, 8);
      const uint32_t lo = (uint32_t)o.shfl_xor((int)(uint32_t)u, (int)m), hi = (uint32_t)o.shfl_xor((int)(uint32_t)(u >> 32), (int)m);
      const int od = o.shfl_xor(bd, (int)m);
      u = (uint64_t)hi << 32 | lo;
      double ov;
      memcpy(&ov, &u, 8);
      if (ov > bv || (ov == bv && od != 0 && od < bd)) { bv = ov; bd = od; }
    }
    if (active && q == 0) {
      const double c = bd ? (double)lsv + bv : (double)lsv;
      int sl = pos + j;
      if (sl >= R) sl -= R;
      o.std(L.ring + (unsigned)sl, c);
      const int bk = bd && i >= i0 ? i - bd : -1;
      cum[i] = c; back[i] = bk;
      if (P.out_mode == 1) { dst[i] = (float)c; dst[(size_t)P.n_frames + (size_t)i] = (float)bk; }
    }
  }
}

// ---- k_clip_beat_pick ----
MEL_FN bool beat_is_max(const double* cum, int n, int i) { return i >= 1 && cum[i] > cum[i - 1] && (i == n - 1 || cum[i] >= cum[i + 1]); }
MEL_FN void beat_chunk(int n, unsigned tid, int* a, int* b) {
  const int c = (n + kBeatThreads - 1) / kBeatThreads;
  *a = (int)tid * c < n ? (int)tid * c : n;
  *b = *a + c < n ? *a + c : n;
}
// the local maxima of a thread's run of frames, counted
template <class O>
MEL_FN void beat_pick_count(O& o, const double* cum, int n, unsigned tid) {
  int a, b;
  beat_chunk(n, tid, &a, &b);
  unsigned c = 0;
  for (int i = a; i < b; i++) c += beat_is_max(cum, n, i) ? 1u : 0u;
  o.stu(kBeatPickCnt + tid, c);
}
template <class O>
MEL_FN unsigned beat_pick_before(O& o, unsigned upto) {
  unsigned s = 0;
  for (unsigned t = 0; t < upto; t++) s += o.ldu(kBeatPickCnt + t);
  return s;
}
// ... their values in the frames' order, one after the other
template <class O>
MEL_FN void beat_pick_gather(O& o, const double* cum, double* lmv, int n, unsigned tid) {
  int a, b;
  beat_chunk(n, tid, &a, &b);
  unsigned at = beat_pick_before(o, tid);
  for (int i = a; i < b; i++) if (beat_is_max(cum, n, i)) lmv[at++] = cum[i];
}
// the two middle ones by counting: a value is the k-th smallest where fewer than k + 1 and, with its equals, more than k lie below
template <class O>
MEL_FN void beat_pick_rank(O& o, const double* lmv, unsigned M, unsigned tid) {
  const unsigned k1 = (M - 1u) / 2u, k2 = M / 2u;
  for (unsigned c = tid; c < M; c += (unsigned)kBeatThreads) {
    const double a = lmv[c];
    unsigned lt = 0, eq = 0;
    for (unsigned j = 0; j < M; j++) { const double b = lmv[j]; lt += b < a ? 1u : 0u; eq += b == a ? 1u : 0u; }
    if (lt <= k1 && k1 < lt + eq) o.std(0u, a);
    if (lt <= k2 && k2 < lt + eq) o.std(1u, a);
  }
}
template <class O>
MEL_FN double beat_pick_median(O& o, unsigned M) {
  const double a = o.ldd(0u), b = o.ldd(1u);
  return (M & 1u) ? a : 0.5 * (a + b);
}
// a thread's last local maximum with cum >= 0.5 med, as frame + 1, or 0
template <class O>
MEL_FN void beat_pick_last(O& o, const double* cum, int n, double med, unsigned tid) {
  int a, b;
  beat_chunk(n, tid, &a, &b);
  const double half = 0.5 * med;
  unsigned last = 0;
  for (int i = a; i < b; i++) if (beat_is_max(cum, n, i) && cum[i] >= half) last = (unsigned)i + 1u;
  o.stu(kBeatPickLast + tid, last);
}
// one thread: the tail, the walk back, the trim.  sc[2 .. 6] = first, last (kept t), q, tail, thr; first > last: no beats
template <class O>
MEL_FN void beat_pick_walk(O& o, const pdmp3_beat_params& P, const float* ls, const int* back, int* bt) {
  unsigned tl = 0;
  for (unsigned t = 0; t < (unsigned)kBeatThreads; t++) { const unsigned v = o.ldu(kBeatPickLast + t); tl = v > tl ? v : tl; }
  const int tail = (int)tl - 1;
  int q = 0;
  for (int i = tail; i >= 0; i = back[i]) bt[q++] = i;            // (descending: b_t = bt[q - 1 - t]; back[i] < i)
  const auto s_of = [&](int t) {
    const double l0 = t >= 1 ? (double)ls[bt[q - t]] : 0.0, l1 = (double)ls[bt[q - 1 - t]], l2 = t + 1 < q ? (double)ls[bt[q - 2 - t]] : 0.0;
    return (0.5 * l0 + l1) + 0.5 * l2;
  };
  double ss = 0.0;
  for (int t = 0; t < q; t++) { const double s = s_of(t); ss = ss + s * s; }
  const double thr = q > 0 && P.trim ? 0.5 * sqrt(ss / (double)q) : 0.0;
  int first = q, last = -1;
  for (int t = 0; t < q; t++) if (s_of(t) > thr) { if (first == q) first = t; last = t; }
  o.std(2u, (double)first); o.std(3u, (double)last); o.std(4u, (double)q); o.std(5u, (double)tail); o.std(6u, q > 0 ? thr : -1.0);
}

}  // namespace pdmp3
#endif
