// Host build of k_clip_pyin_obs and k_clip_pyin_path (pdmp3_amd/csrc/pyin.hip) for tests/test_clip_pyin_host.py: the kernels'
// own phases (pdmp3_amd/csrc/pyin_core.h), thread by thread.  The phases between two workgroup barriers run one after the
// other; a phase whose lanes exchange values (a frame's troughs and probabilities, a step's maxima) runs on wave_emul.h's 64
// fibers, a wave at a time.  The LDS is an array of the size the plan asks for in which every word knows whether it has been
// written: a load outside the array or of a word nobody wrote ends the run with -1.  The addresses are host addresses here.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../pdmp3_amd/csrc/pyin_core.h"
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
  float ldf(unsigned i) const { return mel_from_bits(ldu(i)); }
  void stf(unsigned i, float v) const { stu(i, mel_bits(v)); }
  double ldd(unsigned i) const { double v = 0.0; if (ok((size_t)2 * i, 2)) memcpy(&v, &m->word[(size_t)2 * i], 8); return v; }
  void std(unsigned i, double v) const {
    if ((size_t)2 * i + 2 > m->word.size()) { m->bad = 1; return; }
    memcpy(&m->word[(size_t)2 * i], &v, 8); m->written[(size_t)2 * i] = m->written[(size_t)2 * i + 1] = 1;
  }
  void sync() const { emu::wave_sync(); }
  unsigned long long ballot(bool c) const { return emu::ballot(c); }
  int shfl_xor(int v, int mask) const {
    emu::Wave& w = emu::g_group.wave[emu::g_group.cur];
    const int me = w.cur;
    w.ia[me] = v;
    emu::wave_sync();
    const int r = w.ia[(me ^ mask) & 63];
    emu::wave_sync();
    return r;
  }
  double log(double x) const { return ::log(x); }
};

bool params_ok(const pdmp3_pyin_params& P) {
  return !(P.tmin < 1 || P.tmin >= P.tmax || P.tmax > 2046 || P.n_thr < 1 || P.n_thr > 256 || P.n_bins < 2 || P.n_bins > 2048 || P.hb < 0 ||
           2 * P.hb > P.n_bins || P.max_troughs != (P.tmax - 1 - P.tmin) / 2 + 1 ||
           (P.frames_wg != 1 && P.frames_wg != 2 && P.frames_wg != 4 && P.frames_wg != 8) || (P.out_mode != 0 && P.out_mode != 1) || P.n_frames < 0 ||
           (unsigned)P.path_threads != pyin_path_threads(P.n_bins) || P.obs_lds_bytes > PDMP3_MEL_LDS_SOFT || P.path_lds_bytes > PDMP3_MEL_LDS_MAX ||
           P.obs_lds_bytes < pyin_obs_lds_bytes(P, P.frames_wg) || (size_t)P.path_lds_bytes < (size_t)pyin_path_lds(P).total_d * sizeof(double));
}

}  // namespace

extern "C" int emul_pyin_params_bytes() { return (int)sizeof(pdmp3_pyin_params); }
extern "C" int emul_pyin_table_bytes(const pdmp3_pyin_params* P) { return (int)pyin_table_bytes(*P); }

// one (clip, channel): curve [tmax + 1][F] -> out, [n_bins + 1][F] (out_mode 1) or [F][n_bins + 1] (out_mode 0).  0, or -1
// where the parameters are not what pdmp3_hip_clip_pyin accepts, or where a lane read LDS it must not read
extern "C" int emul_pyin_obs(const float* curve, float* out, const double* tab, const pdmp3_pyin_params* params) {
  const pdmp3_pyin_params& P = *params;
  if (!params_ok(P)) return -1;
  Lds lds;
  HostOps o{&lds};
  const unsigned nt = 64u * (unsigned)P.frames_wg;
  for (long long f0 = 0; f0 < P.n_frames; f0 += P.frames_wg) {
    lds.reset(P.obs_lds_bytes);
    for (unsigned tid = 0; tid < nt; tid++) pyin_obs_load(o, P, curve, f0, tid);
    for (unsigned wave = 0; wave < (unsigned)P.frames_wg; wave++) {
      if (f0 + wave >= P.n_frames) continue;
      emu::run_wave([&] { pyin_obs_frame(o, P, tab, wave, (unsigned)emu::lane()); });
    }
    for (unsigned tid = 0; tid < nt; tid++) pyin_obs_store(o, P, out, f0, tid);
    if (lds.bad) return -1;
  }
  return 0;
}

// one (clip, channel): obs [F][n_bins + 1] -> the back-pointers [F][2 n_bins] and the four planes [4][F].  0, or -1 as above
extern "C" int emul_pyin_path(const float* obs, uint16_t* bp, float* out, const double* tab, const pdmp3_pyin_params* params) {
  const pdmp3_pyin_params& P = *params;
  if (!params_ok(P) || P.n_frames < 1) return -1;
  Lds lds;
  HostOps o{&lds};
  lds.reset(P.path_lds_bytes);
  const size_t nb = (size_t)P.n_bins;
  const unsigned nw = (unsigned)P.path_threads / 64u;
  for (unsigned tid = 0; tid < (unsigned)P.path_threads; tid++) pyin_path_window(o, P, tab, tid);
  for (long long f = 0; f < P.n_frames; f++)
    for (unsigned wave = 0; wave < nw; wave++)
      emu::run_wave([&] { pyin_path_step(o, P, tab, obs + (size_t)f * (nb + 1u), bp + (size_t)f * 2u * nb, f, wave * 64u + (unsigned)emu::lane()); });
  pyin_path_back(o, P, bp);
  for (unsigned tid = 0; tid < (unsigned)P.path_threads; tid++) pyin_path_store(P, tab, obs, bp, out, tid);
  return lds.bad ? -1 : 0;
}
