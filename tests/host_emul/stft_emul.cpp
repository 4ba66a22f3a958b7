// Host build of k_clip_stft (pdmp3_amd/csrc/stft.hip) for tests/test_clip_stft_host.py: the kernel's own indexing, pointwise
// arithmetic and staging layout (pdmp3_amd/csrc/mel_core.h, stft_core.h) driven by the kernel's structure -- a workgroup per
// (tile of frames, channel, clip), LDS as a plain array with the kernel's regions (the span, then a staging tile a wave), each
// matrix instruction's result as the fused multiply-add chain it is (k ascending), each wave's 16 bins x tile frames written
// to its staging tile as the lanes write them and read back as the lanes read them.  The addresses in the descriptors are
// host addresses here.
#include <stdint.h>

#include <vector>

#include "../../pdmp3_amd/csrc/stft_core.h"

using namespace pdmp3;

static const float kPoison = -1e30f;

// -1: a staging slot was read that its wave had not written for this tile of bins
static int workgroup(const pdmp3_mel_desc& d, const float* tab, const pdmp3_stft_params& P, int ch, long long f0, std::vector<float>& lds) {
  const unsigned hop = (unsigned)P.hop, pad = (unsigned)P.row_pad;
  const int Kp = P.bins16, FT = P.tile, RT = FT / 16, S = stft_stage_stride(FT), ld = 2 * Kp, mode = P.out_mode;
  lds.assign(P.lds_bytes / sizeof(float), kPoison);
  float* const span = lds.data();
  const float* const row = reinterpret_cast<const float*>(static_cast<uintptr_t>(d.src)) + (size_t)ch * d.src_chan_stride;
  const unsigned n_span = (unsigned)(FT - 1) * hop + (unsigned)P.rows;
  for (unsigned p = 0; p < n_span; p++) span[mel_lds_at(p, hop, pad)] = mel_sample(row, P.n_in, f0, P.hop, d.lead, p);
  float* const out = reinterpret_cast<float*>(static_cast<uintptr_t>(d.dst)) + (size_t)ch * d.dst_chan_stride;
  for (int wave = 0; wave < 4; wave++) {
    float* const st = lds.data() + P.span_floats + wave * stft_stage_floats(FT, mode);
    for (int bt = wave; bt < (Kp >> 4); bt += 4) {
      for (int i = 0; i < stft_stage_floats(FT, mode); i++) st[i] = kPoison;
      for (int lane = 0; lane < 64; lane++) {
        const int j = lane & 15, kq = lane >> 4;
        for (int rt = 0; rt < RT; rt++)
          for (int r = 0; r < 4; r++) {
            const int fl = 16 * rt + 4 * kq + r, k = (bt << 4) + j;
            float re = 0.0f, im = 0.0f;
            for (int n = 0; n < P.rows; n++) {
              const float a = span[mel_lds_at((unsigned)fl * hop + (unsigned)n, hop, pad)];
              re = mel_fma(a, tab[(size_t)n * ld + k], re);
              im = mel_fma(a, tab[(size_t)n * ld + Kp + k], im);
            }
            float* const sp = st + j * S + 4 * kq + 16 * rt + r;
            if (mode == 0) { sp[0] = re; sp[16 * S] = im; }
            else sp[0] = stft_value(re, im, P.floor, mode);
          }
      }
      for (int it = 0; it < 16 * FT / 64; it++)
        for (int lane = 0; lane < 64; lane++) {
          const int i = 64 * it + lane, b = stft_stage_row(i / FT, FT), fl = i % FT, k = (bt << 4) + b;
          const long long f = f0 + fl;
          const float v0 = st[b * S + fl];
          const float v1 = mode == 0 ? st[16 * S + b * S + fl] : 0.0f;
          if (v0 == kPoison || v1 == kPoison) return -1;
          if (k >= P.bins || f >= P.n_frames) continue;
          const size_t at = (size_t)k * (size_t)P.n_frames + (size_t)f;
          if (mode != 0) out[at] = v0;
          else { out[2 * at] = v0; out[2 * at + 1] = v1; }
        }
    }
  }
  return 0;
}

extern "C" int emul_stft_desc_bytes() { return (int)sizeof(pdmp3_mel_desc); }
extern "C" int emul_stft_params_bytes() { return (int)sizeof(pdmp3_stft_params); }
// 0, or -1 where the parameters would let the kernel leave its LDS
extern "C" int emul_clip_stft(const pdmp3_mel_desc* descs, int n_clips, const float* tab, const pdmp3_stft_params* params) {
  const pdmp3_stft_params& P = *params;
  if (P.tile != 16 && P.tile != 32) return -1;
  const size_t span = (size_t)(P.tile - 1) * P.hop + P.rows, chunks = (span + P.hop - 1) / P.hop;
  if (P.span_floats < chunks * (size_t)(P.hop + P.row_pad) || (P.span_floats & 3u) ||
      (size_t)P.lds_bytes < ((size_t)P.span_floats + 4 * (size_t)stft_stage_floats(P.tile, P.out_mode)) * sizeof(float) || P.lds_bytes > PDMP3_MEL_LDS_MAX)
    return -1;
  std::vector<float> lds;
  for (int k = 0; k < n_clips; k++)
    for (long long f0 = 0; f0 < P.n_frames; f0 += P.tile)
      for (int ch = 0; ch < P.channels; ch++)
        if (workgroup(descs[k], tab, P, ch, f0, lds) != 0) return -1;
  return 0;
}
