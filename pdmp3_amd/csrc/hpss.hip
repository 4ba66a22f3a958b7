// hpss.hip -- k_clip_hpss: median-filter harmonic-percussive separation of clips (include/pdmp3_bulk.h
// pdmp3_amd_bulk_decode_clips_hpss).  It reads the spectrum k_clip_stft_long wrote into a stage of the
// stream object and writes the caller's rows: the two medians, the soft masks, or the masked spectrum.  The tile's layout, the
// reflection, the selection network, the masks and the stores are hpss_core.h's, one source with the host build of the
// tests.  Launched by stream.hip pdmp3_hip_clip_hpss.  A translation unit of its own.
#include <hip/hip_runtime.h>

#include "../../include/pdmp3_hip.h"
#include "hpss_core.h"

namespace {

using namespace pdmp3;

// One workgroup of four waves per (tile of 64 bins x 64 frames, channel, clip).
//   1. the tile with its halo -- rp bins on both sides, reflected, rh frames on both sides -- goes to LDS once, into a layout
//      made for 15 and 15: wave w takes the rows w, w + 4, .., its lanes consecutive frames (mode 2: the magnitude of the
//      stage's pair, formed on the way);
//   2. wave w takes the bins 16 w .. 16 w + 15 of the tile one after the other, lane l frame f0 + l: both windows from LDS, both
//      medians in registers, the masks, the stores -- consecutive lanes store consecutive frames.
// One barrier, between the two steps.  Bins from K on and frames from F on are not stored; columns behind the stage's last
// frame hold zeros, which only such frames' windows reach.
__global__ __launch_bounds__(kHpssThreads) void k_clip_hpss(const pdmp3_mel_desc* __restrict__ descs, pdmp3_hpss_params P) {
  extern __shared__ __align__(16) float lds[];
  const pdmp3_mel_desc d = descs[blockIdx.y];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int rh = P.kernel_harm / 2, rp = P.kernel_perc / 2;
  const unsigned nbt = (unsigned)hpss_bin_tiles(P.bins);
  const int ch = (int)(blockIdx.x % (unsigned)P.channels);
  const unsigned t = blockIdx.x / (unsigned)P.channels;
  const int k0 = (int)(t % nbt) * kHpssBins;
  const long long f0 = (long long)(t / nbt) * kHpssFrames;
  if (f0 >= P.n_frames) return;
  const float* const stage = reinterpret_cast<const float*>(static_cast<uintptr_t>(d.src)) + (size_t)ch * d.src_chan_stride;
  float* const out = reinterpret_cast<float*>(static_cast<uintptr_t>(d.dst)) + (size_t)ch * d.dst_chan_stride;

  const int rows = kHpssBins + 2 * rp, cols = kHpssFrames + 2 * rh;
  for (int r = wave; r < rows; r += kHpssThreads / 64)
    for (int c = lane; c < cols; c += 64) lds[hpss_lds_at(r, c, rh, rp)] = hpss_load(stage, P, k0, f0, r, c);
  __syncthreads();

  for (int b = 16 * wave; b < 16 * wave + 16; b++) {
    const int k = k0 + b;
    if (k >= P.bins) break;
    hpss_element(lds + hpss_centre(b, lane), stage, out, P, k, f0 + lane);
  }
}

}  // namespace

hipError_t pdmp3_launch_clip_hpss(hipStream_t s, const pdmp3_mel_desc* descs, int n_clips, const pdmp3_hpss_params* params) {
  const pdmp3_hpss_params P = *params;
  if (n_clips <= 0 || P.n_frames <= 0) return hipSuccess;
  if (P.tile_bins != pdmp3::kHpssBins || P.tile_frames != pdmp3::kHpssFrames || P.pitch != pdmp3::kHpssPitch ||
      P.lds_bytes != pdmp3::kHpssLdsFloats * sizeof(float))
    return hipErrorInvalidValue;
  const unsigned tiles = (unsigned)((P.n_frames + pdmp3::kHpssFrames - 1) / pdmp3::kHpssFrames) * (unsigned)pdmp3::hpss_bin_tiles(P.bins);
  const dim3 grid(tiles * (unsigned)P.channels, (unsigned)n_clips);
  hipLaunchKernelGGL(k_clip_hpss, grid, dim3(pdmp3::kHpssThreads), P.lds_bytes, s, descs, P);
  return hipGetLastError();
}
