// Host build of k_clip_mfcc (pdmp3_amd/csrc/mfcc.hip) for tests/test_clip_mfcc_host.py: the kernel's own indexing and
// pointwise arithmetic (pdmp3_amd/csrc/mel_core.h, fbank_core.h, mfcc_core.h) driven by the kernel's structure -- a workgroup
// per (tile of frames, channel, clip), LDS as a plain array with the kernel's regions.  Stages 1 .. 4 as
// tests/host_emul/fbank_emul.cpp has them; then stages 5 .. 8: the logarithm in place over the padded mel tile, the energy out of
// the powers' rows into the spare float behind a frame's cepstra, the DCT as the fused multiply-add chain the matrix
// instruction is (k ascending over the mels16, the padded bands' ln eps against the table's zero rows included), the cepstra
// where the powers were, the stores, the tile's column sums and the finishing pass.  The addresses in the descriptors are
// host addresses here.
#include <stdint.h>

#include <vector>

#include "../../pdmp3_amd/csrc/mfcc_core.h"

using namespace pdmp3;

static const float kPoison = -1e30f;

// what wave_sum gives every lane: l with l ^ 32, ^ 16, ... ^ 1
static float wave_sum(float* v) {
  for (int off = kFbankWave / 2; off; off >>= 1)
    for (int l = 0; l < off; l++) v[l] = v[l] + v[l + off];
  return v[0];
}

static void workgroup(const pdmp3_fbank_desc& d, const float* dft, const float* fbt, const float* dct, const pdmp3_mfcc_params& Q, int ch,
                      long long f0, float* tile_sums, std::vector<float>& lds) {
  const pdmp3_fbank_params& P = Q.fb;
  const unsigned hop = (unsigned)P.hop, pad = (unsigned)P.row_pad;
  const int Kp = P.bins16, Mp = P.mels16, PS = Kp + 2, FT = P.tile, FTS = FT + 1, ld = 2 * Kp;
  lds.assign(P.lds_bytes / sizeof(float), kPoison);
  float* const span = lds.data();
  float* const pw = lds.data() + P.span_floats;
  const float* const row = reinterpret_cast<const float*>(static_cast<uintptr_t>(d.src)) + (size_t)ch * d.src_chan_stride;
  const unsigned n_span = (unsigned)(FT - 1) * hop + (unsigned)P.rows;
  for (unsigned p = 0; p < n_span; p++) span[mel_lds_at(p, hop, pad)] = mel_sample(row, P.n_in, f0, P.hop, 0u, p);
  if (P.use_energy)
    for (int fl = 0; fl < FT; fl++) {
      const unsigned p0 = (unsigned)fl * hop;
      float lanes[kFbankWave], mean = 0.0f;
      if (P.remove_dc) {
        for (int l = 0; l < kFbankWave; l++) lanes[l] = fbank_lane_sum(span, p0, P.win, hop, pad, P.scale, l);
        mean = fbank_mean(wave_sum(lanes), P.win);
      }
      for (int l = 0; l < kFbankWave; l++) lanes[l] = fbank_lane_squares(span, p0, P.win, hop, pad, P.scale, mean, l);
      pw[fl * PS + Kp] = wave_sum(lanes);
    }
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
  // stage 5: the energies leave the powers' rows, the logarithm in place
  const int Cp = Q.ceps16, CS = mfcc_ceps_stride(Cp);
  std::vector<float> energy(FT, 0.0f);
  if (P.use_energy) for (int fl = 0; fl < FT; fl++) energy[fl] = pw[fl * PS + Kp];
  for (int i = 0; i < Mp * FT; i++) {
    const int m = i / FT, fl = i - m * FT;
    mt[m * FTS + fl] = mel_output(mt[m * FTS + fl], P.eps, 1);
  }
  // stage 6: the powers' region becomes the cepstra's (poisoned first: nothing of the powers may be read any more)
  for (size_t i = P.span_floats; i < lds.size(); i++) lds[i] = kPoison;
  float* const ct = pw;
  if (P.use_energy) for (int fl = 0; fl < FT; fl++) ct[fl * CS + Cp] = energy[fl];
  for (int fl = 0; fl < FT; fl++)
    for (int c = 0; c < Cp; c++) {
      float acc = 0.0f;
      for (int k = 0; k < Mp; k++) acc = mel_fma(mt[k * FTS + fl], dct[(size_t)k * Cp + c], acc);
      ct[fl * CS + c] = acc;
    }
  // stages 7 and 8
  float* const out = reinterpret_cast<float*>(static_cast<uintptr_t>(d.dst)) + (size_t)ch * d.dst_chan_stride;
  const int D = Q.n_ceps, ecol = mfcc_energy_column(D, P.use_energy, P.htk_compat);
  for (int i = 0; i < D * FT; i++) {
    const int fl = i / D, dc = i - fl * D;
    const long long f = f0 + fl;
    if (f >= P.n_frames) break;
    float* const cf = ct + fl * CS;
    const float v = mfcc_output(cf, Cp, dc, ecol, P.eps, P.energy_log_floor);
    if (P.subtract_mean && dc == ecol) cf[dc] = v;
    out[(size_t)f * (size_t)D + (size_t)dc] = v;
  }
  if (!P.subtract_mean) return;
  long long cnt = (long long)d.valid - f0;
  cnt = cnt < 0 ? 0 : cnt > FT ? FT : cnt;
  for (int dc = 0; dc < D; dc++) {
    float s = 0.0f;
    for (int fl = 0; fl < (int)cnt; fl++) s = s + ct[fl * CS + dc];
    tile_sums[dc] = s;
  }
}

extern "C" int emul_mfcc_desc_bytes() { return (int)sizeof(pdmp3_fbank_desc); }
extern "C" int emul_mfcc_params_bytes() { return (int)sizeof(pdmp3_mfcc_params); }
// 0, or -1 where the parameters would let the kernel leave its LDS
extern "C" int emul_clip_mfcc(const pdmp3_fbank_desc* descs, int n_clips, const float* dft, const float* fbt, const float* dct,
                              const pdmp3_mfcc_params* params) {
  const pdmp3_mfcc_params& Q = *params;
  const pdmp3_fbank_params& P = Q.fb;
  const size_t span = (size_t)(P.tile - 1) * P.hop + P.rows, chunks = (span + P.hop - 1) / P.hop;
  if (Q.n_ceps < 1 || Q.n_ceps > P.n_mels || Q.ceps16 != ((Q.n_ceps + 15) & ~15) || P.out_mode != 1) return -1;
  if (P.span_floats < chunks * (size_t)(P.hop + P.row_pad) || P.span_floats < (size_t)P.mels16 * (P.tile + 1) ||
      (size_t)P.lds_bytes < ((size_t)P.span_floats + mfcc_second_region(P.tile, P.bins16, Q.ceps16)) * sizeof(float) || P.lds_bytes > PDMP3_MEL_LDS_MAX)
    return -1;
  const int D = Q.n_ceps;
  const size_t tiles = ((size_t)P.n_frames + P.tile - 1) / P.tile;
  std::vector<float> lds, sums(tiles * D + 1, kPoison);
  for (int k = 0; k < n_clips; k++) {
    const pdmp3_fbank_desc& d = descs[k];
    if ((long long)d.valid > (long long)P.n_frames) return -1;
    for (int ch = 0; ch < P.channels; ch++) {
      for (size_t t = 0; t < tiles; t++) workgroup(d, dft, fbt, dct, Q, ch, (long long)t * P.tile, sums.data() + t * D, lds);
      if (!P.subtract_mean || !d.valid) continue;
      float* const out = reinterpret_cast<float*>(static_cast<uintptr_t>(d.dst)) + (size_t)ch * d.dst_chan_stride;
      std::vector<float> mean(D);
      for (int dc = 0; dc < D; dc++) {
        float s = 0.0f;
        for (size_t t = 0; t < tiles; t++) s = s + sums[t * D + dc];
        mean[dc] = fbank_column_mean(s, d.valid);
      }
      for (long long i = 0; i < (long long)D * P.n_frames; i++) out[i] = out[i] - mean[(size_t)(i % D)];
    }
  }
  return 0;
}
