// Host build of k_clip_onset, k_clip_tempogram and k_clip_tempo (pdmp3_amd/csrc/tempogram.hip) for
// tests/test_clip_tempogram_host.py: the kernels' own phases (pdmp3_amd/csrc/tempogram_core.h), thread by thread.  The phases
// between two workgroup barriers run one after the other; a phase whose lanes exchange values (a frame's matrix products and
// quotients, the decision) runs on wave_emul.h's 64 fibers, the matrix instruction as the fused multiply-add chain it is.  The
// LDS is an array of the size the plan asks for in which every word knows whether it has been written: a load outside the
// array or of a word nobody wrote ends the run with -1.  The addresses in the descriptors are host addresses here.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../pdmp3_amd/csrc/tempogram_core.h"
#include "wave_emul.h"

using namespace pdmp3;

namespace {

struct Lds {
  std::vector<uint32_t> word;
  std::vector<uint8_t> written;
  int bad = 0;
  void fresh(size_t words) { word.assign(words, 0x7fc00001u); written.assign(words, 0); bad = 0; }
};

struct HostOps {
  struct acc4 {
    float v[4];
    float& operator[](int i) { return v[i]; }
  };
  Lds* m;
  bool ok(unsigned i, unsigned n) const {
    if ((size_t)i + n > m->word.size()) { m->bad = 1; return false; }
    for (unsigned k = 0; k < n; k++) if (!m->written[i + k]) { m->bad = 1; return false; }
    return true;
  }
  float ldf(unsigned i) const { float v = 0.0f; if (ok(i, 1)) memcpy(&v, &m->word[i], 4); return v; }
  double ldd(unsigned i) const { double v = 0.0; if (ok(2 * i, 2)) memcpy(&v, &m->word[2 * i], 8); return v; }
  void stf(unsigned i, float v) const {
    if ((size_t)i >= m->word.size()) { m->bad = 1; return; }
    memcpy(&m->word[i], &v, 4); m->written[i] = 1;
  }
  void std(unsigned i, double v) const {
    if ((size_t)2 * i + 2 > m->word.size()) { m->bad = 1; return; }
    memcpy(&m->word[2 * i], &v, 8); m->written[2 * i] = m->written[2 * i + 1] = 1;
  }
  acc4 zero() const { return acc4{{0.0f, 0.0f, 0.0f, 0.0f}}; }
  void mfma(float a, float b, acc4& c) const { emu::mfma16(a, b, c.v); }
  void sync() const { emu::wave_sync(); }
  void issued() const {}
};

template <class T>
T* at(uint64_t address) { return reinterpret_cast<T*>(static_cast<uintptr_t>(address)); }
float* env_of(const pdmp3_tempogram_desc& d, const pdmp3_tempogram_params& P, int ch) {
  return at<float>(d.env) + (size_t)ch * (P.out_mode == 0 ? (size_t)d.dst_chan_stride : (size_t)P.env_stride);
}
float* tg_of(const pdmp3_tempogram_desc& d, const pdmp3_tempogram_params& P, int ch) {
  return at<float>(d.tg) + (size_t)ch * (P.out_mode == 1 ? (size_t)d.dst_chan_stride : (size_t)P.win * (size_t)P.n_frames);
}

template <int TILES>
void frame_wave(HostOps& o, const pdmp3_tempogram_params& P, const tempogram_layout& L, const float* env, const float* w, long long f, unsigned wave) {
  emu::run_wave([&] { tempogram_frame<TILES>(o, P, L, env, w, f, wave, (unsigned)emu::lane()); });
}

int tempogram_workgroup(const pdmp3_tempogram_desc& d, const pdmp3_tempogram_params& P, const float* w, int ch, long long f0, Lds& lds) {
  const unsigned nt = 64u * (unsigned)P.frames_wg;
  lds.fresh(P.lds_bytes / 4);
  HostOps o{&lds};
  const tempogram_layout L = tempogram_lds(P);
  for (unsigned wave = 0; wave < (unsigned)P.frames_wg; wave++) {
    if (f0 + wave >= P.n_frames) continue;
    switch (P.tiles) {
      case 1: frame_wave<1>(o, P, L, env_of(d, P, ch), w, f0 + wave, wave); break;
      case 2: frame_wave<2>(o, P, L, env_of(d, P, ch), w, f0 + wave, wave); break;
      case 3: frame_wave<3>(o, P, L, env_of(d, P, ch), w, f0 + wave, wave); break;
      default: frame_wave<4>(o, P, L, env_of(d, P, ch), w, f0 + wave, wave); break;
    }
  }
  for (unsigned tid = 0; tid < nt; tid++) tempogram_store(o, P, L, tg_of(d, P, ch), f0, tid);
  return lds.bad ? -1 : 0;
}

int tempo_workgroup(const pdmp3_tempogram_desc& d, const pdmp3_tempogram_params& P, const double* prior, int ch, Lds& lds) {
  lds.fresh(2 * (kTempoMaxWin + 128));
  HostOps o{&lds};
  for (unsigned tid = 0; tid < (unsigned)kTempoThreads; tid++) tempo_scores(o, P, tg_of(d, P, ch), prior, tid);
  float* const out = at<float>(d.dst) + (size_t)ch * (size_t)d.dst_chan_stride;
  emu::run_wave([&] { tempo_decide(o, P, out, (unsigned)emu::lane()); });
  return lds.bad ? -1 : 0;
}

}  // namespace

extern "C" int emul_tempogram_desc_bytes() { return (int)sizeof(pdmp3_tempogram_desc); }
extern "C" int emul_tempogram_params_bytes() { return (int)sizeof(pdmp3_tempogram_params); }
// 0, or -1 where the parameters are not what pdmp3_hip_clip_tempogram accepts, or where a lane read LDS it must not read
extern "C" int emul_clip_tempogram(const pdmp3_tempogram_desc* descs, int n_clips, const float* window, const double* prior,
                                   const pdmp3_tempogram_params* params) {
  const pdmp3_tempogram_params& P = *params;
  if (P.n_mels < 1 || P.n_mels > 256 || P.lag < 1 || P.lag > 16 || P.half < 0 || P.half > 4 || P.hop < 1 || P.win < 16 || P.win > kTempoMaxWin ||
      (P.win & 1) || P.tiles != (P.win + 255) / 256 || P.ksteps != (P.win + 18) / 4 ||
      (P.frames_wg != 1 && P.frames_wg != 2 && P.frames_wg != 4 && P.frames_wg != 8) || (P.channels != 1 && P.channels != 2) || P.out_mode < 0 ||
      P.out_mode > 2 || P.n_frames < 0 || P.n_env != (P.out_mode == 0 ? (long long)P.n_frames : (long long)P.n_frames + P.win - 1) ||
      P.n_mel_frames != (long long)P.n_env + P.lag || (P.out_mode != 0 && P.env_stride < (unsigned)P.n_env) || !(P.sr > 0.0) || (P.span_floats & 3u) ||
      P.lds_bytes > PDMP3_MEL_LDS_MAX)
    return -1;
  if (P.ext < tempogram_ext(P.win, P.tiles, P.ksteps) || P.span_floats < pitch_at(P.ext) || (size_t)P.lds_bytes < (size_t)tempogram_lds(P).total_f * sizeof(float))
    return -1;
  Lds lds;
  for (int k = 0; k < n_clips; k++) {
    const pdmp3_tempogram_desc& d = descs[k];
    for (int ch = 0; ch < P.channels; ch++) {
      const float* const l = at<const float>(d.mel) + (size_t)ch * (size_t)P.n_mels * (size_t)P.n_mel_frames;
      for (long long e = 0; e < P.n_env; e++) env_of(d, P, ch)[e] = onset_value(l, P, e);
    }
    if (P.out_mode == 0) continue;
    for (long long f0 = 0; f0 < P.n_frames; f0 += P.frames_wg)
      for (int ch = 0; ch < P.channels; ch++)
        if (tempogram_workgroup(d, P, window, ch, f0, lds) != 0) return -1;
    if (P.out_mode == 1) continue;
    for (int ch = 0; ch < P.channels; ch++)
      if (tempo_workgroup(d, P, prior, ch, lds) != 0) return -1;
  }
  return 0;
}
