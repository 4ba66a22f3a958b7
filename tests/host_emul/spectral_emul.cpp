// Host build of k_clip_spectral (pdmp3_amd/csrc/spectral.hip) for tests/test_clip_spectral_host.py: the kernel's own index maps,
// LDS layouts and lane arithmetic (pdmp3_amd/csrc/spectral_core.h on stft_long_core.h / mel_core.h) driven by the kernel's
// structure -- a workgroup of eight waves per (tile of frames, channel, clip) that takes the four tiles of k1 one after the
// other, LDS as a plain array with the kernel's four regions, each matrix instruction's result as the fused multiply-add chain
// it is (k ascending), every LDS value written by the lane that writes it and read by the lane that reads it, and what crosses
// lanes (the butterfly, the scan, the minimum) in spectral_core.h's orders.  What a stage no longer needs is poisoned: Z once a
// kt's powers are in the plane.  The addresses in the descriptors are host addresses here.
#include <stdint.h>

#include <vector>

#include "../../pdmp3_amd/csrc/spectral_core.h"

using namespace pdmp3;

static const float kPoison = -1e30f;

// v = v + v[lane ^ off], off = 32 .. 1: every lane ends with the same value
static double butterfly(double* v) {
  double t[64];
  for (int off = 32; off; off >>= 1) {
    for (int l = 0; l < 64; l++) t[l] = v[l] + v[l ^ off];
    for (int l = 0; l < 64; l++) v[l] = t[l];
  }
  return v[0];
}

// -1: an LDS slot was read that this workgroup had not written in the stage before
static int workgroup(const pdmp3_mel_desc& d, const float* tab, const pdmp3_spectral_params& P, int ch, long long f0, std::vector<float>& lds) {
  const int N = P.n_fft, N2 = P.n2, K2 = N2 / 2, NT = N2 / 16, NCT = K2 / 16, FT = P.tile, K = spec_bins(N);
  lds.assign(P.lds_bytes / sizeof(float), kPoison);
  float* const span = lds.data();
  float* const z = lds.data() + P.span_floats;
  float* const plane = z + stftl_z_floats(FT, N2);
  float* const res = plane + spec_plane_floats(FT, N);
  const float* const row = reinterpret_cast<const float*>(static_cast<uintptr_t>(d.src)) + (size_t)ch * d.src_chan_stride;
  float* const out = reinterpret_cast<float*>(static_cast<uintptr_t>(d.dst)) + (size_t)ch * d.dst_chan_stride;
  const unsigned n_span = stftl_span(FT, P.hop, N);
  for (unsigned p = 0; p < n_span; p++) span[p] = mel_sample(row, P.n_in, f0, P.hop, d.lead, p);

  // rows 0 and 1: wave `wave` the frames wave, wave + 8, ..
  for (int wave = 0; wave < 8; wave++)
    for (int fl = wave; fl < FT; fl += 8) {
      double sq[64];
      int cross = 0;
      for (int lane = 0; lane < 64; lane++) {
        int c;
        spec_lane_frame(span + (unsigned)fl * (unsigned)P.hop, N, lane, P.zcr_threshold, &sq[lane], &c);
        cross += c;
      }
      res[0 * FT + fl] = spec_rms(butterfly(sq), N);
      res[1 * FT + fl] = spec_zcr(cross, N);
    }

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

    // the Nyquist bin
    if (kt == 0)
      for (int tid = 0; tid < FT; tid++) {
        float re, im;
        stftl_nyquist(z, tid, N2, &re, &im);
        const unsigned at = (unsigned)(tid * K) + spec_col(N / 2);
        if (plane[at] != kPoison) return -1;
        plane[at] = mel_power(re, im);
      }

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
            const unsigned at = (unsigned)(fl * K) + spec_col(16 * kt + k1l + 64 * k2);
            if (plane[at] != kPoison) return -1;                               // (two bins in one column)
            plane[at] = mel_power(re, im);
          }
        }
    }
    for (unsigned p = 0; p < stftl_z_floats(FT, N2); p++) z[p] = kPoison;
  }
  for (unsigned p = 0; p < spec_plane_floats(FT, N); p++) if (plane[p] == kPoison) return -1;

  // the reductions
  for (int wave = 0; wave < 8; wave++)
    for (int fl = wave; fl < FT; fl += 8) {
      float* const pr = plane + fl * K;
      double ts[64], tfs[64], tln[64], tp[64], prefix[64], tbw[64];
      for (int lane = 0; lane < 64; lane++) spec_lane_pass_a(pr, N, lane, P.bin_hz, P.amin, &ts[lane], &tfs[lane], &tln[lane], &tp[lane]);
      double total = 0.0;
      for (int l = 0; l < 64; l++) { prefix[l] = total; total = total + ts[l]; }
      const double fs = butterfly(tfs), ln = butterfly(tln), p = butterfly(tp);
      const double c = spec_centroid(fs, total);
      int first = N;
      for (int lane = 0; lane < 64; lane++) {
        int at;
        spec_lane_pass_b(pr, N, lane, P.bin_hz, c, prefix[lane], spec_threshold(P.roll_percent, total), &tbw[lane], &at);
        if (at >= 0 && at < first) first = at;
      }
      res[2 * FT + fl] = (float)c;
      res[3 * FT + fl] = spec_bandwidth(butterfly(tbw), total);
      res[4 * FT + fl] = spec_rolloff(first, P.bin_hz);
      res[5 * FT + fl] = spec_flatness(ln, p, N);
    }

  // the stores
  for (int tid = 0; tid < kSpectralRows * FT; tid++) {
    const int rw = tid / FT, fl = tid % FT;
    const long long f = f0 + fl;
    if (res[rw * FT + fl] == kPoison) return -1;
    if (f < P.n_frames) out[(size_t)rw * (size_t)P.n_frames + (size_t)f] = res[rw * FT + fl];
  }
  return 0;
}

extern "C" int emul_spectral_desc_bytes() { return (int)sizeof(pdmp3_mel_desc); }
extern "C" int emul_spectral_params_bytes() { return (int)sizeof(pdmp3_spectral_params); }
// the core header's maps for the tests: the column of bin k in a frame's row of the plane, and the LDS floats of a plan
extern "C" unsigned emul_spectral_col(int k) { return spec_col(k); }
extern "C" unsigned emul_spectral_lds_floats(int tile, int hop, int n_fft) { return spec_lds_floats(tile, hop, n_fft); }
// 0, or -1 where the parameters would let the kernel leave its LDS (or a stage read what the one before had not written)
extern "C" int emul_clip_spectral(const pdmp3_mel_desc* descs, int n_clips, const float* tab, const pdmp3_spectral_params* params) {
  const pdmp3_spectral_params& P = *params;
  const bool path = (P.n2 == 32 && P.tile == 8) || (P.n2 == 64 && P.tile == 4);
  if (!path || P.n_fft != 64 * P.n2 || P.hop < 1 || P.hop > P.n_fft || (P.span_floats & 3u) || P.span_floats < stftl_span(P.tile, P.hop, P.n_fft) ||
      (size_t)P.lds_bytes < ((size_t)P.span_floats + stftl_z_floats(P.tile, P.n2) + spec_plane_floats(P.tile, P.n_fft) + spec_res_floats(P.tile)) * sizeof(float) ||
      P.lds_bytes > PDMP3_MEL_LDS_MAX || !(P.roll_percent > 0.0 && P.roll_percent < 1.0) || !(P.amin > 0.0f) || !(P.zcr_threshold >= 0.0f))
    return -1;
  std::vector<float> lds;
  for (int k = 0; k < n_clips; k++)
    for (long long f0 = 0; f0 < P.n_frames; f0 += P.tile)
      for (int ch = 0; ch < P.channels; ch++)
        if (workgroup(descs[k], tab, P, ch, f0, lds) != 0) return -1;
  return 0;
}
