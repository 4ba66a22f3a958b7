// Host build of k_clip_hpss (pdmp3_amd/csrc/hpss.hip) for tests/test_clip_hpss_host.py: the kernel's own layout, reflection,
// selection network, masks and stores (pdmp3_amd/csrc/hpss_core.h) driven by the kernel's structure -- a workgroup of four waves
// per (tile of 64 bins x 64 frames, channel, clip), LDS as a plain array filled with changing bit patterns (a NaN's, -1, a
// large float's) before every workgroup, every LDS value written by the lane that writes it and read by the lane that reads it.
// The slots a window of the call's sizes reads must have been written by this workgroup; what a window of 31 reads beyond them
// is whatever the fill left there, as on the device.  The addresses in the descriptors are host addresses here.
#include <stdint.h>

#include <vector>

#include "../../pdmp3_amd/csrc/hpss_core.h"

using namespace pdmp3;

static const uint32_t kFill[4] = {0x7fc00000u, 0xffffffffu, 0x7f7fffffu, 0x80000001u};

// -1: a window of the call's sizes would read an LDS slot that this workgroup had not written
static int workgroup(const pdmp3_mel_desc& d, const pdmp3_hpss_params& P, int ch, int k0, long long f0, std::vector<float>& lds,
                     std::vector<char>& written) {
  const int rh = P.kernel_harm / 2, rp = P.kernel_perc / 2;
  lds.resize(P.lds_bytes / sizeof(float));
  for (size_t i = 0; i < lds.size(); i++) lds[i] = hpss_float((int32_t)kFill[(i + (size_t)k0 + (size_t)f0) & 3]);
  written.assign(lds.size(), 0);
  const float* const stage = reinterpret_cast<const float*>(static_cast<uintptr_t>(d.src)) + (size_t)ch * d.src_chan_stride;
  float* const out = reinterpret_cast<float*>(static_cast<uintptr_t>(d.dst)) + (size_t)ch * d.dst_chan_stride;

  const int rows = kHpssBins + 2 * rp, cols = kHpssFrames + 2 * rh;
  for (int wave = 0; wave < kHpssThreads / 64; wave++)
    for (int r = wave; r < rows; r += kHpssThreads / 64)
      for (int lane = 0; lane < 64; lane++)
        for (int c = lane; c < cols; c += 64) {
          const unsigned at = hpss_lds_at(r, c, rh, rp);
          if (at >= lds.size() || written[at]) return -1;
          lds[at] = hpss_load(stage, P, k0, f0, r, c);
          written[at] = 1;
        }

  for (int wave = 0; wave < kHpssThreads / 64; wave++)
    for (int b = 16 * wave; b < 16 * wave + 16; b++) {
      const int k = k0 + b;
      if (k >= P.bins) break;
      for (int lane = 0; lane < 64; lane++) {
        const unsigned at = hpss_centre(b, lane);
        if (at < (unsigned)(kHpssHalo * kHpssPitch) || (size_t)at + kHpssHalo * kHpssPitch >= lds.size()) return -1;    // (a window of 31 inside the LDS)
        for (int o = -rh; o <= rh; o++) if (!written[at + o]) return -1;
        for (int o = -rp; o <= rp; o++) if (!written[at + o * kHpssPitch]) return -1;
        hpss_element(lds.data() + at, stage, out, P, k, f0 + lane);
      }
    }
  return 0;
}

extern "C" int emul_hpss_desc_bytes() { return (int)sizeof(pdmp3_mel_desc); }
extern "C" int emul_hpss_params_bytes() { return (int)sizeof(pdmp3_hpss_params); }
// the core header's numbers and maps for the tests
extern "C" int emul_hpss_pitch() { return kHpssPitch; }
extern "C" unsigned emul_hpss_lds_floats() { return kHpssLdsFloats; }
extern "C" unsigned emul_hpss_lds_at(int r, int c, int rh, int rp) { return hpss_lds_at(r, c, rh, rp); }
extern "C" unsigned emul_hpss_centre(int b, int lane) { return hpss_centre(b, lane); }
extern "C" int emul_hpss_reflect(int i, int bins) { return hpss_reflect(i, bins); }
// the (r + 1)-th smallest of the 2 r + 1 floats around v[15 step]; v holds 31 values `step` apart
extern "C" float emul_hpss_median(const float* v, int step, int r) {
  return step == 1 ? hpss_median<1>(v + 15, r) : hpss_median<kHpssPitch>(v + 15 * kHpssPitch, r);
}
extern "C" float emul_hpss_mask(float x, float rf, double margin, int power, int unit) { return hpss_mask(x, rf, margin, power, unit != 0); }
// 0, or -1 where the parameters would let the kernel leave its LDS (or a window would read what the load had not written)
extern "C" int emul_clip_hpss(const pdmp3_mel_desc* descs, int n_clips, const pdmp3_hpss_params* params) {
  const pdmp3_hpss_params& P = *params;
  const auto kernel_ok = [](int l) { return l >= 3 && l <= kHpssMaxKernel && (l & 1); };
  if (!kernel_ok(P.kernel_harm) || !kernel_ok(P.kernel_perc) || P.tile_bins != kHpssBins || P.tile_frames != kHpssFrames || P.pitch != kHpssPitch ||
      P.lds_bytes != kHpssLdsFloats * sizeof(float) || P.lds_bytes > PDMP3_MEL_LDS_MAX || P.bins != P.n_fft / 2 + 1 || P.n_frames < 0 ||
      P.n_stage != P.n_frames + P.kernel_harm - 1 || P.out_mode < 0 || P.out_mode > 3 || (P.power != 0 && P.power != 1 && P.power != 2))
    return -1;
  std::vector<float> lds;
  std::vector<char> written;
  for (int k = 0; k < n_clips; k++)
    for (long long f0 = 0; f0 < P.n_frames; f0 += kHpssFrames)
      for (int bt = 0; bt < hpss_bin_tiles(P.bins); bt++)
        for (int ch = 0; ch < P.channels; ch++)
          if (workgroup(descs[k], P, ch, bt * kHpssBins, f0, lds, written) != 0) return -1;
  return 0;
}
