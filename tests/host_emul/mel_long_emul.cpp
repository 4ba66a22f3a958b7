// Host build of k_clip_mel_long (pdmp3_amd/csrc/mel_long.hip) for tests/test_clip_mel_long_host.py: the kernel's own index
// maps and LDS layouts (pdmp3_amd/csrc/mel_long_core.h on stft_long_core.h / mel_core.h) driven by the kernel's structure -- a
// workgroup of eight waves per (tile of frames, channel, clip) that takes the four tiles of k1 one after the other, LDS as a
// plain array with the kernel's three regions, each matrix instruction's result as the fused multiply-add chain it is (k
// ascending), every LDS value written by the lane that writes it and read by the lane that reads it, the accumulators of the
// filterbank per (wave, band tile, lane, r) as the kernel's registers.  What a stage no longer needs is poisoned: Z once the
// power tile is complete, the power tile once its kt's GEMM is through; the span stays.  The addresses in the descriptors are
// host addresses here.
#include <stdint.h>

#include <vector>

#include "../../pdmp3_amd/csrc/mel_long_core.h"

using namespace pdmp3;

static const float kPoison = -1e30f;

// -1: an LDS slot was read that this workgroup had not written in the stage before
static int workgroup(const pdmp3_mel_desc& d, const float* tab, const float* op, const pdmp3_mel_long_params& P, int ch, long long f0,
                     std::vector<float>& lds) {
  const int N = P.n_fft, N2 = P.n2, K2 = N2 / 2, NT = N2 / 16, NCT = K2 / 16, FT = P.tile, SLOTS = mell_slots(N2);
  const int mp = P.mels16, nbt = mp >> 4;
  lds.assign(P.lds_bytes / sizeof(float), kPoison);
  float* const span = lds.data();
  float* const z = lds.data() + P.span_floats;
  float* const pw = z + stftl_z_floats(FT, N2);
  const float* const row = reinterpret_cast<const float*>(static_cast<uintptr_t>(d.src)) + (size_t)ch * d.src_chan_stride;
  float* const out = reinterpret_cast<float*>(static_cast<uintptr_t>(d.dst)) + (size_t)ch * d.dst_chan_stride;
  const unsigned n_span = stftl_span(FT, P.hop, N);
  for (unsigned p = 0; p < n_span; p++) span[p] = mel_sample(row, P.n_in, f0, P.hop, d.lead, p);

  // acc[wave][q][lane][r]: band 16 (wave + 8 q) + 4 kq + r of frame j
  std::vector<float> acc(8 * 2 * 64 * 4, 0.0f);
  const float* const d64 = tab + stftl_tab_d64(N);
  const float* const tw = tab + stftl_tab_tw(N);
  const float* const h2 = tab + stftl_tab_h2(N);
  for (int kt = 0; kt < 4; kt++) {
    // stage 1 and the twiddles
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
    for (unsigned p = 0; p < stftl_z_floats(FT, N2); p++) if (z[p] == kPoison) return -1;

    // stage 2 and the powers
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
            const unsigned at = mell_p_at(fl, mell_slot(k1l, k2, N2), N2);
            if (pw[at] != kPoison) return -1;                                  // (two bins in one slot)
            pw[at] = mel_power(re, im);
          }
        }
    }
    for (unsigned p = 0; p < stftl_z_floats(FT, N2); p++) z[p] = kPoison;

    // the filterbank: rows the bands, columns the frames, k the slots ascending
    for (int wave = 0; wave < 8; wave++)
      for (int q = 0; q < 2; q++) {
        const int bt = wave + 8 * q;
        if (bt >= nbt) continue;
        for (int lane = 0; lane < 64; lane++) {
          const int j = lane & 15, kq = lane >> 4;
          for (int r = 0; r < 4; r++) {
            const int band = 16 * bt + 4 * kq + r;
            float a = acc[((wave * 2 + q) * 64 + lane) * 4 + r];
            for (int s = 0; s < SLOTS; s++) {
              const float p = j < FT ? pw[mell_p_at(j, s, N2)] : 0.0f;
              if (p == kPoison) return -1;
              a = mel_fma(op[(size_t)(SLOTS * kt + s) * (size_t)mp + (size_t)band], p, a);
            }
            acc[((wave * 2 + q) * 64 + lane) * 4 + r] = a;
          }
        }
      }
    for (unsigned p = 0; p < mell_p_floats(FT, N2); p++) pw[p] = kPoison;
  }

  // the stores, from the registers
  for (int wave = 0; wave < 8; wave++)
    for (int lane = 0; lane < 64; lane++) {
      const int j = lane & 15, kq = lane >> 4;
      const long long f = f0 + j;
      if (j >= FT || f >= P.n_frames) continue;
      for (int r = 0; r < 4; r++)
        for (int q = 0; q < 2; q++) {
          const int m = 16 * (wave + 8 * q) + 4 * kq + r;
          if (m < P.n_mels) out[(size_t)m * (size_t)P.n_frames + (size_t)f] = mel_output(acc[((wave * 2 + q) * 64 + lane) * 4 + r], P.floor, P.out_mode);
        }
    }
  return 0;
}

extern "C" int emul_mel_long_desc_bytes() { return (int)sizeof(pdmp3_mel_desc); }
extern "C" int emul_mel_long_params_bytes() { return (int)sizeof(pdmp3_mel_long_params); }
// the core header's maps for the tests: the operand's row of bin k < N / 2, and the LDS floats of a plan
extern "C" int emul_mel_long_operand_row(int k, int n2) { return mell_operand_row((k & 63) >> 4, k & 15, k >> 6, n2); }
extern "C" unsigned emul_mel_long_lds_floats(int tile, int hop, int n_fft) { return mell_lds_floats(tile, hop, n_fft); }
// 0, or -1 where the parameters would let the kernel leave its LDS (or a stage read what the one before had not written)
extern "C" int emul_clip_mel_long(const pdmp3_mel_desc* descs, int n_clips, const float* tab, const float* op, const pdmp3_mel_long_params* params) {
  const pdmp3_mel_long_params& P = *params;
  const bool path = P.n2 == 32 ? (P.tile == 16 || P.tile == 8) : P.n2 == 64 ? (P.tile == 8 || P.tile == 4) : false;
  if (!path || P.n_fft != 64 * P.n2 || P.hop < 1 || P.hop > P.n_fft || P.n_mels < 1 || P.n_mels > 256 || P.mels16 != ((P.n_mels + 15) & ~15) ||
      (P.span_floats & 3u) || P.span_floats < stftl_span(P.tile, P.hop, P.n_fft) ||
      (size_t)P.lds_bytes < ((size_t)P.span_floats + stftl_z_floats(P.tile, P.n2) + mell_p_floats(P.tile, P.n2)) * sizeof(float) ||
      P.lds_bytes > PDMP3_MEL_LDS_MAX)
    return -1;
  std::vector<float> lds;
  for (int k = 0; k < n_clips; k++)
    for (long long f0 = 0; f0 < P.n_frames; f0 += P.tile)
      for (int ch = 0; ch < P.channels; ch++)
        if (workgroup(descs[k], tab, op, P, ch, f0, lds) != 0) return -1;
  return 0;
}
