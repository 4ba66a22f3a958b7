// Host build of the kernels of pdmp3_amd/csrc/mfcc_long.hip for tests/test_clip_mfcc_long_host.py: the kernels' own values, LDS
// planes and stencil (pdmp3_amd/csrc/mfcc_long_core.h) driven by the kernels' structure -- k_clip_db_max's plane maximum, then a
// workgroup of four waves per (tile of 64 frames, channel, clip), LDS as a plain array filled with a NaN's pattern before every
// workgroup, every LDS value written by the lane that writes it and read by the lane that reads it, or k_clip_db's elements.
// The matrix instruction is restated as what it is: per element of the result a chain of fused multiply-adds over the bands
// in ascending order, its fragments read and its result written at the addresses the lanes use.  A slot that is read must
// have been written by this workgroup.  The addresses in the descriptors are host addresses here.
#include <math.h>
#include <stdint.h>

#include <vector>

#include "../../pdmp3_amd/csrc/mfcc_long_core.h"

using namespace pdmp3;

static const float* stage_of(const pdmp3_mel_desc& d, int ch) {
  return reinterpret_cast<const float*>(static_cast<uintptr_t>(d.src)) + (size_t)ch * d.src_chan_stride;
}
static float* thr_of(const pdmp3_mel_desc& d, int channels, int ch) {
  return reinterpret_cast<float*>(static_cast<uintptr_t>(d.src)) + (size_t)channels * d.src_chan_stride + ch;
}

static void db_max(const pdmp3_mel_desc& d, const pdmp3_mfcc_long_params& P, int ch) {
  const float* const stage = stage_of(d, ch) + P.halo;
  float mx = -INFINITY;
  for (int m = 0; m < P.n_mels; m++)
    for (int t = 0; t < P.n_frames; t++) mx = fmaxf(mx, mfcc_long_db(stage[(size_t)m * (size_t)P.n_stage + (size_t)t]));
  *thr_of(d, P.channels, ch) = mfcc_long_threshold(mx, P.top_db);
}

// -1: an LDS slot would be read that this workgroup had not written, or an address leaves the LDS
static int workgroup(const pdmp3_mel_desc& d, const float* dct, const pdmp3_mfcc_long_params& P, int ch, long long f0, std::vector<float>& lds,
                     std::vector<char>& written) {
  lds.assign(P.lds_bytes / sizeof(float), NAN);
  written.assign(lds.size(), 0);
  const float* const stage = stage_of(d, ch);
  float* const out = reinterpret_cast<float*>(static_cast<uintptr_t>(d.dst)) + (size_t)ch * d.dst_chan_stride;
  const float thr = P.use_top ? *thr_of(d, P.channels, ch) : -INFINITY;
  const int Mp = P.mels16, cols = mfcc_long_cols16(P.halo), waves = kMfccLongThreads / 64;

  for (int wave = 0; wave < waves; wave++)
    for (int m = wave; m < Mp; m += waves)
      for (int lane = 0; lane < 64; lane++)
        for (int c = lane; c < cols; c += 64) {
          const unsigned at = mfcc_long_d_at(m, c);
          if (at >= lds.size() || written[at]) return -1;
          lds[at] = mfcc_long_load(stage, P, f0, m, c, thr);
          written[at] = 1;
        }

  const int nct = cols >> 4;
  for (int wave = 0; wave < waves; wave++)
    for (int t = wave; t < nct * (P.ceps16 >> 4); t += waves) {
      const int col0 = (t % nct) << 4, q0 = (t / nct) << 4;
      float acc[64][4] = {};
      for (int k = 0; k < Mp; k += 4) {
        // lane (j, kq) holds A[row j][k + kq] and B[k + kq][col j]; D[row 4 kq + r][col j] adds the four products, k ascending
        float a[64], b[64];
        for (int lane = 0; lane < 64; lane++) {
          const int j = lane & 15, kq = lane >> 4;
          const unsigned at = mfcc_long_b_at(k, kq, col0, j);
          if (at >= lds.size() || !written[at]) return -1;
          a[lane] = dct[(size_t)(q0 + j) * (size_t)Mp + (size_t)(k + kq)];
          b[lane] = lds[at];
        }
        for (int lane = 0; lane < 64; lane++)
          for (int r = 0; r < 4; r++)
            for (int kk = 0; kk < 4; kk++) acc[lane][r] = fmaf(a[16 * kk + 4 * (lane >> 4) + r], b[16 * kk + (lane & 15)], acc[lane][r]);
      }
      for (int lane = 0; lane < 64; lane++)
        for (int r = 0; r < 4; r++) {
          const unsigned at = mfcc_long_result_at(Mp, q0, lane >> 4, r, col0, lane & 15);
          if (at >= lds.size() || written[at]) return -1;
          lds[at] = acc[lane][r];
          written[at] = 1;
        }
    }

  for (int wave = 0; wave < waves; wave++)
    for (int q = wave; q < P.n_mfcc; q += waves)
      for (int lane = 0; lane < 64; lane++) {
        const unsigned at = mfcc_long_c_at(Mp, q, 0);
        for (int j = 0; j <= 2 * P.halo; j++)
          if (at + lane + j >= lds.size() || !written[at + lane + j]) return -1;
        mfcc_long_store(lds.data() + at, out, P, q, lane, f0 + lane);
      }
  return 0;
}

extern "C" int emul_mfcc_long_desc_bytes() { return (int)sizeof(pdmp3_mel_desc); }
extern "C" int emul_mfcc_long_params_bytes() { return (int)sizeof(pdmp3_mfcc_long_params); }
// the core header's numbers and maps for the tests
extern "C" int emul_mfcc_long_d_pitch() { return kMfccLongDPitch; }
extern "C" int emul_mfcc_long_c_pitch() { return kMfccLongCPitch; }
extern "C" int emul_mfcc_long_cols16(int halo) { return mfcc_long_cols16(halo); }
extern "C" unsigned emul_mfcc_long_lds_floats(int mels16, int ceps16) { return mfcc_long_lds_floats(mels16, ceps16); }
extern "C" unsigned emul_mfcc_long_d_at(int m, int c) { return mfcc_long_d_at(m, c); }
extern "C" unsigned emul_mfcc_long_c_at(int mels16, int q, int c) { return mfcc_long_c_at(mels16, q, c); }
extern "C" unsigned emul_mfcc_long_b_at(int k, int kq, int col0, int j) { return mfcc_long_b_at(k, kq, col0, j); }
extern "C" unsigned emul_mfcc_long_result_at(int mels16, int q0, int kq, int r, int col0, int j) { return mfcc_long_result_at(mels16, q0, kq, r, col0, j); }
// 0, or -1 where the parameters would let a kernel leave its LDS or read what it had not written
extern "C" int emul_clip_mfcc_long(const pdmp3_mel_desc* descs, int n_clips, const float* dct, const pdmp3_mfcc_long_params* params) {
  const pdmp3_mfcc_long_params& P = *params;
  if (P.n_mels < 1 || P.n_mels > 256 || P.mels16 != ((P.n_mels + 15) & ~15) || P.n_frames < 0 || P.halo < 0 || P.halo > kMfccLongMaxHalo ||
      P.n_stage != P.n_frames + 2 * P.halo || (P.out_mode != 0 && P.out_mode != 1))
    return -1;
  if (P.out_mode == 0 &&
      (P.n_mfcc < 1 || P.n_mfcc > P.n_mels || P.n_mfcc > 128 || P.ceps16 != ((P.n_mfcc + 15) & ~15) || P.tile != kMfccLongFrames ||
       P.d_pitch != kMfccLongDPitch || P.c_pitch != kMfccLongCPitch || P.lds_bytes != mfcc_long_lds_floats(P.mels16, P.ceps16) * sizeof(float) ||
       P.lds_bytes > PDMP3_MEL_LDS_MAX || P.deltas < 0 || P.deltas > 2 || (P.deltas == 0) != (P.halo == 0) || !dct))
    return -1;
  if (P.out_mode == 1 && P.halo != 0) return -1;
  std::vector<float> lds;
  std::vector<char> written;
  for (int k = 0; k < n_clips; k++)
    for (int ch = 0; ch < P.channels; ch++) {
      if (P.use_top) db_max(descs[k], P, ch);
      if (P.out_mode == 1) {
        const float* const stage = stage_of(descs[k], ch);
        float* const out = reinterpret_cast<float*>(static_cast<uintptr_t>(descs[k].dst)) + (size_t)ch * descs[k].dst_chan_stride;
        const float thr = P.use_top ? *thr_of(descs[k], P.channels, ch) : -INFINITY;
        for (size_t i = 0; i < (size_t)P.n_mels * (size_t)P.n_frames; i++) out[i] = mfcc_long_clamp(mfcc_long_db(stage[i]), thr);
        continue;
      }
      for (long long f0 = 0; f0 < P.n_frames; f0 += kMfccLongFrames)
        if (workgroup(descs[k], dct, P, ch, f0, lds, written) != 0) return -1;
    }
  return 0;
}
