// Host build of k_clip_stft_long (pdmp3_amd/csrc/stft_long.hip) for tests/test_clip_stft_long_host.py: the kernel's own index
// maps, LDS layouts, twiddle step and Nyquist chain (pdmp3_amd/csrc/stft_long_core.h, with mel_core.h / stft_core.h) driven
// by the kernel's structure -- a workgroup of eight waves per (tile of frames, sixteen k1, channel, clip), LDS as a plain
// array with the kernel's regions, each matrix instruction's result as the fused multiply-add chain it is (k ascending),
// every LDS value written by the lane that writes it and read by the lane that reads it.  What a stage no longer needs is
// poisoned before the next one: the span once Z is complete (the staging tile takes its place), Z once the staging tile is.
// The addresses in the descriptors are host addresses here.
#include <stdint.h>

#include <vector>

#include "../../pdmp3_amd/csrc/stft_long_core.h"

using namespace pdmp3;

static const float kPoison = -1e30f;

// -1: an LDS slot was read that this workgroup had not written in the stage before
static int workgroup(const pdmp3_mel_desc& d, const float* tab, const pdmp3_stft_long_params& P, int ch, int kt, long long f0,
                     std::vector<float>& lds) {
  const int N = P.n_fft, N2 = P.n2, K2 = N2 / 2, NT = N2 / 16, NCT = K2 / 16, FT = P.tile, mode = P.out_mode;
  lds.assign(P.lds_bytes / sizeof(float), kPoison);
  float* const span = lds.data();
  float* const stage = lds.data();
  float* const z = lds.data() + P.span_floats;
  const float* const row = reinterpret_cast<const float*>(static_cast<uintptr_t>(d.src)) + (size_t)ch * d.src_chan_stride;
  float* const out = reinterpret_cast<float*>(static_cast<uintptr_t>(d.dst)) + (size_t)ch * d.dst_chan_stride;
  const unsigned n_span = stftl_span(FT, P.hop, N);
  for (unsigned p = 0; p < n_span; p++) span[p] = mel_sample(row, P.n_in, f0, P.hop, d.lead, p);

  // stage 1 and the twiddles
  const float* const d64 = tab + stftl_tab_d64(N);
  const float* const tw = tab + stftl_tab_tw(N);
  for (int wave = 0; wave < 8; wave++) {
    const int t = wave % NT;
    for (int fl = wave / NT; fl < FT; fl += 8 / NT)
      for (int lane = 0; lane < 64; lane++) {
        const int j = lane & 15, kq = lane >> 4;
        for (int r = 0; r < 4; r++) {
          const int n2 = 16 * t + 4 * kq + r, k1 = 16 * kt + j;
          float re = 0.0f, im = 0.0f;
          for (int n1 = 0; n1 < 64; n1++) {
            const float y = span[(unsigned)fl * (unsigned)P.hop + (unsigned)(N2 * n1 + n2)];
            if (y == kPoison) return -1;
            const float a = stftl_window(tab[N2 * n1 + n2], y);
            re = mel_fma(a, d64[n1 * 128 + k1], re);
            im = mel_fma(a, d64[n1 * 128 + 64 + k1], im);
          }
          float zr, zi;
          stftl_twiddle(re, im, tw[n2 * 128 + k1], tw[n2 * 128 + 64 + k1], &zr, &zi);
          z[stftl_z_at(fl, n2, 0, j, N2)] = zr;
          z[stftl_z_at(fl, n2, 1, j, N2)] = zi;
        }
      }
  }
  for (unsigned p = 0; p < P.span_floats; p++) span[p] = kPoison;
  for (unsigned p = 0; p < stftl_z_floats(FT, N2); p++) if (z[p] == kPoison) return -1;

  // the Nyquist bin
  if (kt == 0)
    for (int tid = 0; tid < FT && f0 + tid < P.n_frames; tid++) {
      float re, im;
      stftl_nyquist(z, tid, N2, &re, &im);
      const size_t at = (size_t)(N / 2) * (size_t)P.n_frames + (size_t)(f0 + tid);
      if (mode != 0) out[at] = stft_value(re, im, P.floor, mode);
      else { out[2 * at] = re; out[2 * at + 1] = im; }
    }

  // stage 2
  const float* const h2 = tab + stftl_tab_h2(N);
  for (int wave = 0; wave < 8; wave++) {
    const int ct = wave % NCT;
    for (int fl = wave / NCT; fl < FT; fl += 8 / NCT)
      for (int lane = 0; lane < 64; lane++) {
        const int j = lane & 15, kq = lane >> 4;
        for (int r = 0; r < 4; r++) {
          const int k1l = 4 * kq + r, k2 = 16 * ct + j;
          float re = 0.0f, im = 0.0f;
          for (int t = 0; t < 2 * N2; t++) {
            const float a = z[stftl_z_at(fl, t >> 1, t & 1, k1l, N2)];
            re = mel_fma(a, h2[t * N2 + k2], re);
            im = mel_fma(a, h2[t * N2 + K2 + k2], im);
          }
          if (mode == 0) {
            stage[stftl_stage_at(0, k1l, k2, fl, FT, N2)] = re;
            stage[stftl_stage_at(1, k1l, k2, fl, FT, N2)] = im;
          } else {
            stage[stftl_stage_at(0, k1l, k2, fl, FT, N2)] = stft_value(re, im, P.floor, mode);
          }
        }
      }
  }
  for (unsigned p = 0; p < stftl_z_floats(FT, N2); p++) z[p] = kPoison;

  // the store loop
  for (int i0 = 0; i0 < 16 * K2 * FT; i0 += kStftLongThreads)
    for (int tid = 0; tid < kStftLongThreads; tid++) {
      const int i = i0 + tid;
      if (i >= 16 * K2 * FT) break;
      const int rw = i / FT, fl = i % FT, k1l = rw / K2, k2 = rw % K2, k = 16 * kt + k1l + 64 * k2;
      const long long f = f0 + fl;
      const float v0 = stage[stftl_stage_at(0, k1l, k2, fl, FT, N2)];
      const float v1 = mode == 0 ? stage[stftl_stage_at(1, k1l, k2, fl, FT, N2)] : 0.0f;
      if (v0 == kPoison || v1 == kPoison) return -1;
      if (f >= P.n_frames) continue;
      const size_t at = (size_t)k * (size_t)P.n_frames + (size_t)f;
      if (mode != 0) out[at] = v0;
      else { out[2 * at] = v0; out[2 * at + 1] = v1; }
    }
  return 0;
}

extern "C" int emul_stft_long_desc_bytes() { return (int)sizeof(pdmp3_mel_desc); }
extern "C" int emul_stft_long_params_bytes() { return (int)sizeof(pdmp3_stft_long_params); }
// 0, or -1 where the parameters would let the kernel leave its LDS (or a stage read what the one before had not written)
extern "C" int emul_clip_stft_long(const pdmp3_mel_desc* descs, int n_clips, const float* tab, const pdmp3_stft_long_params* params) {
  const pdmp3_stft_long_params& P = *params;
  const bool path = P.n2 == 32 ? (P.tile == 16 || P.tile == 8) : P.n2 == 64 ? (P.tile == 8 || P.tile == 4) : false;
  if (!path || P.n_fft != 64 * P.n2 || (P.span_floats & 3u) || P.span_floats < stftl_span(P.tile, P.hop, P.n_fft) ||
      P.span_floats < stftl_stage_floats(P.tile, P.n2, P.out_mode) ||
      (size_t)P.lds_bytes < ((size_t)P.span_floats + stftl_z_floats(P.tile, P.n2)) * sizeof(float) || P.lds_bytes > PDMP3_MEL_LDS_MAX)
    return -1;
  std::vector<float> lds;
  for (int k = 0; k < n_clips; k++)
    for (long long f0 = 0; f0 < P.n_frames; f0 += P.tile)
      for (int ch = 0; ch < P.channels; ch++)
        for (int kt = 0; kt < 4; kt++)
          if (workgroup(descs[k], tab, P, ch, kt, f0, lds) != 0) return -1;
  return 0;
}
