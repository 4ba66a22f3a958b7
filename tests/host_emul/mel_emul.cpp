// Host build of k_clip_mel (pdmp3_amd/csrc/mel.hip) for tests/test_clip_mel_host.py: the kernel's own indexing and pointwise
// arithmetic (pdmp3_amd/csrc/mel_core.h) driven by the kernel's structure -- a workgroup per (tile of frames, channel, clip),
// LDS as a plain array with the kernel's three regions, each matrix instruction's result as the fused multiply-add chain it
// is (k ascending).  The addresses in the descriptors are host addresses here.
#include <stdint.h>

#include <vector>

#include "../../pdmp3_amd/csrc/mel_core.h"

using namespace pdmp3;

static const float kPoison = -1e30f;

static void workgroup(const pdmp3_mel_desc& d, const float* dft, const float* fbt, const pdmp3_mel_params& P, int ch, long long f0,
                      uint32_t* row_max, std::vector<float>& lds) {
  const unsigned hop = (unsigned)P.hop, pad = (unsigned)P.row_pad;
  const int Kp = P.bins16, Mp = P.mels16, PS = Kp + 2, FT = P.tile, FTS = FT + 1, ld = 2 * Kp;
  lds.assign(P.lds_bytes / sizeof(float), kPoison);
  float* const span = lds.data();
  float* const pw = lds.data() + P.span_floats;
  const float* const row = reinterpret_cast<const float*>(static_cast<uintptr_t>(d.src)) + (size_t)ch * d.src_chan_stride;
  const unsigned n_span = (unsigned)(FT - 1) * hop + (unsigned)P.rows;
  for (unsigned p = 0; p < n_span; p++) span[mel_lds_at(p, hop, pad)] = mel_sample(row, P.n_in, f0, P.hop, d.lead, p);
  for (int fl = 0; fl < FT; fl++)
    for (int k = 0; k < Kp; k++) {
      float re = 0.0f, im = 0.0f;
      for (int n = 0; n < P.rows; n++) {
        const float a = span[mel_lds_at((unsigned)fl * hop + (unsigned)n, hop, pad)];
        re = mel_fma(a, dft[(size_t)n * ld + k], re);
        im = mel_fma(a, dft[(size_t)n * ld + Kp + k], im);
      }
      pw[fl * PS + k] = mel_power(re, im);
    }
  std::vector<float> tile((size_t)Mp * FT);
  for (int fl = 0; fl < FT; fl++)
    for (int m = 0; m < Mp; m++) {
      float acc = 0.0f;
      for (int k = 0; k < Kp; k++) acc = mel_fma(pw[fl * PS + k], fbt[(size_t)k * Mp + m], acc);
      tile[(size_t)m * FT + fl] = acc;
    }
  float* const mt = lds.data();                        // (over the span, as in the kernel: it must fit in front of the powers)
  for (int m = 0; m < Mp; m++)
    for (int fl = 0; fl < FT; fl++) mt[m * FTS + fl] = tile[(size_t)m * FT + fl];
  float* const out = reinterpret_cast<float*>(static_cast<uintptr_t>(d.dst)) + (size_t)ch * d.dst_chan_stride;
  for (int i = 0; i < P.n_mels * FT; i++) {
    const int m = i / FT, fl = i % FT;
    const long long f = f0 + fl;
    if (f >= P.n_frames) continue;
    const float v = mt[m * FTS + fl];
    if (P.out_mode == 3) { const uint32_t u = mel_bits(v); if (u > *row_max) *row_max = u; }
    out[(size_t)m * (size_t)P.n_frames + (size_t)f] = mel_output(v, P.floor, P.out_mode);
  }
}

extern "C" int emul_mel_desc_bytes() { return (int)sizeof(pdmp3_mel_desc); }
extern "C" int emul_mel_params_bytes() { return (int)sizeof(pdmp3_mel_params); }
// 0, or -1 where the parameters would let the kernel leave its LDS
extern "C" int emul_clip_mel(const pdmp3_mel_desc* descs, int n_clips, const float* dft, const float* fbt, const pdmp3_mel_params* params) {
  const pdmp3_mel_params& P = *params;
  const size_t span = (size_t)(P.tile - 1) * P.hop + P.rows, chunks = (span + P.hop - 1) / P.hop;
  if (P.span_floats < chunks * (size_t)(P.hop + P.row_pad) || P.span_floats < (size_t)P.mels16 * (P.tile + 1) ||
      (size_t)P.lds_bytes < ((size_t)P.span_floats + (size_t)P.tile * (P.bins16 + 2)) * sizeof(float) || P.lds_bytes > PDMP3_MEL_LDS_MAX)
    return -1;
  std::vector<float> lds;
  for (int k = 0; k < n_clips; k++) {
    uint32_t row_max = 0;
    for (long long f0 = 0; f0 < P.n_frames; f0 += P.tile)
      for (int ch = 0; ch < P.channels; ch++) workgroup(descs[k], dft, fbt, P, ch, f0, &row_max, lds);
    if (P.out_mode != 3) continue;
    const float top = mel_from_bits(row_max);
    for (int ch = 0; ch < P.channels; ch++) {
      float* const out = reinterpret_cast<float*>(static_cast<uintptr_t>(descs[k].dst)) + (size_t)ch * descs[k].dst_chan_stride;
      for (long long i = 0; i < (long long)P.n_mels * P.n_frames; i++) out[i] = mel_whisper(out[i], top, P.floor);
    }
  }
  return 0;
}
