// Host build of k_clip_pitch (pdmp3_amd/csrc/pitch.hip) for tests/test_clip_pitch_host.py: the kernel's own phases
// (pdmp3_amd/csrc/pitch_core.h), thread by thread.  The phases between two workgroup barriers run one after the other; a phase
// whose lanes exchange values (the scan of the squares, a frame's matrix products, sums and decision) runs on wave_emul.h's 64
// fibers, the matrix instruction as the fused multiply-add chain it is.  The LDS is an array of the size the plan asks for in
// which every word knows whether it has been written: a load outside the array or of a word nobody wrote ends the run with -1.
// The addresses in the descriptors are host addresses here.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../pdmp3_amd/csrc/pitch_core.h"
#include "wave_emul.h"

using namespace pdmp3;

namespace {

struct Lds {
  std::vector<uint32_t> word;
  std::vector<uint8_t> written;
  int bad = 0;
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
  bool any(bool c) const { return emu::any(c); }
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

template <int TILES>
void frame_wave(HostOps& o, const pdmp3_pitch_params& P, const pitch_layout& L, unsigned wave) {
  emu::run_wave([&] { pitch_frame<TILES>(o, P, L, wave, (unsigned)emu::lane()); });
}

int workgroup(const pdmp3_mel_desc& d, const pdmp3_pitch_params& P, int ch, long long f0, Lds& lds) {
  const unsigned nt = 64u * (unsigned)P.frames_wg;
  lds.word.assign(P.lds_bytes / 4, 0x7fc00001u);
  lds.written.assign(P.lds_bytes / 4, 0);
  lds.bad = 0;
  HostOps o{&lds};
  const pitch_layout L = pitch_lds(P);
  const float* const row = reinterpret_cast<const float*>(static_cast<uintptr_t>(d.src)) + (size_t)ch * d.src_chan_stride;
  float* const out = reinterpret_cast<float*>(static_cast<uintptr_t>(d.dst)) + (size_t)ch * d.dst_chan_stride;
  for (unsigned tid = 0; tid < nt; tid++) pitch_load(o, P, row, f0, d.lead, tid);
  for (unsigned tid = 0; tid < nt; tid++) pitch_sq_pieces(o, P, L, tid);
  emu::run_wave([&] { pitch_sq_scan(o, P, L, (unsigned)emu::lane()); });
  for (unsigned tid = 0; tid < nt; tid++) pitch_sq_write(o, P, L, tid);
  // (the scratch of the scan is the frames' from here on: what a wave reads of it, it has to have written itself)
  for (unsigned i = 2 * L.t_d; i < L.curve_f; i++) lds.written[i] = 0;
  for (unsigned wave = 0; wave < (unsigned)P.frames_wg; wave++) {
    if (f0 + wave >= P.n_frames) continue;
    switch (P.tiles) {
      case 1: frame_wave<1>(o, P, L, wave); break;
      case 2: frame_wave<2>(o, P, L, wave); break;
      case 3: frame_wave<3>(o, P, L, wave); break;
      case 4: frame_wave<4>(o, P, L, wave); break;
      case 5: frame_wave<5>(o, P, L, wave); break;
      case 6: frame_wave<6>(o, P, L, wave); break;
      case 7: frame_wave<7>(o, P, L, wave); break;
      default: frame_wave<8>(o, P, L, wave); break;
    }
  }
  for (unsigned tid = 0; tid < nt; tid++) pitch_store(o, P, L, out, f0, tid);
  return lds.bad ? -1 : 0;
}

}  // namespace

extern "C" int emul_pitch_desc_bytes() { return (int)sizeof(pdmp3_mel_desc); }
extern "C" int emul_pitch_params_bytes() { return (int)sizeof(pdmp3_pitch_params); }
extern "C" unsigned emul_pitch_at(unsigned x) { return pitch_at(x); }
// 0, or -1 where the parameters are not what pdmp3_hip_clip_pitch accepts, or where a lane read LDS it must not read
extern "C" int emul_clip_pitch(const pdmp3_mel_desc* descs, int n_clips, const pdmp3_pitch_params* params) {
  const pdmp3_pitch_params& P = *params;
  if (P.n < 64 || P.n > 2048 || (P.n & 1) || P.win < 4 || P.win > P.n - 2 || P.hop < 1 || P.hop > P.n || P.tmin < 1 || P.tmin >= P.tmax ||
      P.tmax > P.n - P.win - 1 || P.tiles != (P.tmax + 256) / 256 || P.tiles > 8 || P.ksteps != (P.win + 18) / 4 ||
      (P.frames_wg != 1 && P.frames_wg != 2 && P.frames_wg != 4 && P.frames_wg != 8) || (P.channels != 1 && P.channels != 2) ||
      (P.out_mode != 0 && P.out_mode != 1) || P.n_frames < 0 || P.n_in < 0 || !(P.sr > 0.0) || !(P.threshold > 0.0) || (P.span_floats & 3u) ||
      P.lds_bytes > PDMP3_MEL_LDS_MAX)
    return -1;
  const size_t reach = (size_t)4 * (P.ksteps + 1) + 240 + (size_t)256 * (P.tiles - 1), first = (size_t)(P.frames_wg - 1) * P.hop;
  const size_t ext = kPitchFront + first + (reach > (size_t)P.n ? reach : (size_t)P.n);
  if (P.q_doubles != first + P.n + 1 || P.ext < ext || P.span_floats < pitch_at(P.ext) || (size_t)P.lds_bytes < (size_t)pitch_lds(P).total_f * sizeof(float))
    return -1;
  Lds lds;
  for (int k = 0; k < n_clips; k++)
    for (long long f0 = 0; f0 < P.n_frames; f0 += P.frames_wg)
      for (int ch = 0; ch < P.channels; ch++)
        if (workgroup(descs[k], P, ch, f0, lds) != 0) return -1;
  return 0;
}
