// Host build of k_clip_beat_score, k_clip_beat_dp and k_clip_beat_pick (pdmp3_amd/csrc/beat.hip) for
// tests/test_clip_beat_host.py: the kernels' own phases (pdmp3_amd/csrc/beat_core.h), thread by thread.  The phases between two
// workgroup barriers run one after the other; the programme's step, whose lanes exchange their bests, runs on wave_emul.h's 64
// fibers, a wave at a time.  The LDS is an array of the size the plan asks for in which every word knows whether it has been
// written: a load outside the array or of a word nobody wrote ends the run with -1.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../pdmp3_amd/csrc/beat_core.h"
#include "wave_emul.h"

using namespace pdmp3;

namespace {

struct Lds {
  std::vector<uint32_t> word;
  std::vector<uint8_t> written;
  int bad = 0;
  void reset(size_t bytes) {
    word.assign(bytes / 4, 0x7fc00001u);
    written.assign(bytes / 4, 0);
    bad = 0;
  }
};

struct HostOps {
  Lds* m;
  bool ok(size_t i, unsigned n) const {
    if (i + n > m->word.size()) { m->bad = 1; return false; }
    for (unsigned k = 0; k < n; k++) if (!m->written[i + k]) { m->bad = 1; return false; }
    return true;
  }
  unsigned ldu(unsigned i) const { return ok(i, 1) ? m->word[i] : 0u; }
  void stu(unsigned i, unsigned v) const {
    if ((size_t)i >= m->word.size()) { m->bad = 1; return; }
    m->word[i] = v; m->written[i] = 1;
  }
  double ldd(unsigned i) const { double v = 0.0; if (ok((size_t)2 * i, 2)) memcpy(&v, &m->word[(size_t)2 * i], 8); return v; }
  void std(unsigned i, double v) const {
    if ((size_t)2 * i + 2 > m->word.size()) { m->bad = 1; return; }
    memcpy(&m->word[(size_t)2 * i], &v, 8); m->written[(size_t)2 * i] = m->written[(size_t)2 * i + 1] = 1;
  }
  int shfl_xor(int v, int mask) const {
    emu::Wave& w = emu::g_group.wave[emu::g_group.cur];
    const int me = w.cur;
    w.ia[me] = v;
    emu::wave_sync();
    const int r = w.ia[(me ^ mask) & 63];
    emu::wave_sync();
    return r;
  }
};

bool shape_ok(int n, int F, int Pd, int p_max) { return F >= 1 && F <= kBeatMaxFrames && n >= 0 && n <= F && Pd >= 1 && Pd <= p_max && p_max <= kBeatMaxPeriod; }

}  // namespace

extern "C" int emul_beat_params_bytes() { return (int)sizeof(pdmp3_beat_params); }
extern "C" int emul_beat_half(int P) { return beat_half(P); }
extern "C" long long emul_beat_table_at(int p_min, int P) { return (long long)beat_table_at(p_min, P); }
extern "C" unsigned emul_beat_work_doubles(int F) { return beat_work_of(F).total_d; }
extern "C" unsigned emul_beat_score_lds(int p_max, int F) { return beat_score_lds(p_max, F).total_d * 8u; }
extern "C" unsigned emul_beat_dp_lds(int p_max) { return beat_dp_lds(p_max).total_d * 8u; }

// one (clip, channel): env [n] -> ls [F] (0 from n on) and the norm.  1 where the tracker runs, 0 where it does not (n < 2, a
// norm that is not finite and positive), -1 on a bad shape or where a thread read LDS it must not read
extern "C" int emul_beat_score(const float* env, int n, int F, int Pd, int p_max, const double* g, unsigned lds_bytes, float* ls, double* norm_out) {
  if (!shape_ok(n, F, Pd, p_max) || (size_t)lds_bytes < (size_t)beat_score_lds(p_max, F).total_d * 8u) return -1;
  Lds lds;
  HostOps o{&lds};
  lds.reset(lds_bytes);
  const beat_score_layout L = beat_score_lds(p_max, F);
  const unsigned nt = (unsigned)kBeatThreads;
  double norm = -1.0;
  bool run = n >= 2;
  if (run) {
    for (unsigned tid = 0; tid < nt; tid++) beat_score_sums(o, L, env, n, Pd, g, 0.0, 0, tid);
    const double m = beat_score_total(o, L, n) / (double)n;
    for (unsigned tid = 0; tid < nt; tid++) beat_score_sums(o, L, env, n, Pd, g, m, 1, tid);
    norm = sqrt(beat_score_total(o, L, n) / (double)(n - 1));
    run = beat_norm_ok(norm);
  }
  *norm_out = norm;
  for (int t0 = 0; t0 < F; t0 += kBeatTile) {
    if (run && t0 < n) for (unsigned tid = 0; tid < nt; tid++) beat_score_load(o, L, env, n, Pd, norm, t0, tid);
    for (unsigned tid = 0; tid < nt; tid++) {
      const int i = t0 + (int)tid;
      if (i < F) ls[i] = run && i < n ? beat_score_frame(o, L, Pd, tid) : 0.0f;
    }
  }
  return lds.bad ? -1 : run ? 1 : 0;
}

// one (clip, channel): ls [n] -> cum [n] and back [n].  0, or -1 as above
extern "C" int emul_beat_dp(const float* ls, int n, int F, int Pd, int p_max, const double* tx, unsigned lds_bytes, double* cum, int* back) {
  if (!shape_ok(n, F, Pd, p_max) || n < 1 || (size_t)lds_bytes < (size_t)beat_dp_lds(p_max).total_d * 8u) return -1;
  Lds lds;
  HostOps o{&lds};
  lds.reset(lds_bytes);
  const beat_dp_layout L = beat_dp_lds(p_max);
  const unsigned nt = (unsigned)kBeatThreads;
  pdmp3_beat_params P;
  memset(&P, 0, sizeof P);
  P.n_frames = F; P.out_mode = 2;
  for (unsigned tid = 0; tid < nt; tid++) beat_dp_head(o, L, tx, ls, n, Pd, tid);
  const double mx = beat_dp_red(o, L, true);
  for (unsigned tid = 0; tid < nt; tid++) beat_dp_first(o, L, ls, n, mx, tid);
  const int i0 = (int)beat_dp_red(o, L, false);
  const int h = beat_half(Pd);
  for (int s0 = 0; s0 < n; s0 += h)
    for (unsigned wave = 0; wave < nt / 64u; wave++)
      emu::run_wave([&] { beat_dp_step(o, P, L, Pd, n, i0, s0, ls, cum, back, (float*)nullptr, wave * 64u + (unsigned)emu::lane()); });
  return lds.bad ? -1 : 0;
}

// one (clip, channel): ls, cum, back [n] -> rows [2][F] (the mask; the beats, -1 behind them) and res[5] = kept, beats before
// the trim, the tail, thr, the local maxima (-1 where not reached).  0, or -1 as above.  lmv, bt: scratch of F values each
extern "C" int emul_beat_pick(const float* ls, const double* cum, const int* back, int n, int F, int trim, double* lmv, int* bt, float* rows, double* res) {
  if (n < 2 || n > F || F > kBeatMaxFrames) return -1;
  Lds lds;
  HostOps o{&lds};
  lds.reset(kBeatPickWords * 4u);
  const unsigned nt = (unsigned)kBeatThreads;
  pdmp3_beat_params P;
  memset(&P, 0, sizeof P);
  P.n_frames = F; P.trim = trim;
  for (int i = 0; i < F; i++) { rows[i] = 0.0f; rows[F + i] = -1.0f; }
  res[0] = 0.0; res[1] = res[2] = res[3] = -1.0;
  for (unsigned tid = 0; tid < nt; tid++) beat_pick_count(o, cum, n, tid);
  const unsigned M = beat_pick_before(o, nt);
  res[4] = (double)M;
  if (!M) return lds.bad ? -1 : 0;
  for (unsigned tid = 0; tid < nt; tid++) beat_pick_gather(o, cum, lmv, n, tid);
  for (unsigned tid = 0; tid < nt; tid++) beat_pick_rank(o, lmv, M, tid);
  const double med = beat_pick_median(o, M);
  for (unsigned tid = 0; tid < nt; tid++) beat_pick_last(o, cum, n, med, tid);
  beat_pick_walk(o, P, ls, back, bt);
  const int t_first = (int)o.ldd(2u), t_last = (int)o.ldd(3u), q = (int)o.ldd(4u);
  for (int t = t_first; t <= t_last; t++) {
    const int b = bt[q - 1 - t];
    rows[b] = 1.0f;
    rows[F + t - t_first] = (float)b;
  }
  res[0] = t_last >= t_first ? (double)(t_last - t_first + 1) : 0.0;
  res[1] = (double)q; res[2] = o.ldd(5u); res[3] = o.ldd(6u);
  return lds.bad ? -1 : 0;
}
