// resample.hip -- k_clip_audio: the staged int16 PCM of a batch of clips to rows of a planar float32 batch at one sampling
// frequency and channel count (include/pdmp3_bulk.h pdmp3_amd_bulk_decode_clips_audio).  Launched by
// stream.hip pdmp3_hip_clip_audio.  A translation unit of its own, so that the decode, unpack, merge and pack kernels' code
// is what it is without it (as engine_lsf.hip and clip.hip); its arithmetic is resample_core.h's.
#include <hip/hip_runtime.h>

#include "../../include/pdmp3_hip.h"
#include "resample_core.h"

namespace {

using namespace pdmp3;

// One workgroup per (tile of kAudioTile output samples, clip); lane = output sample, four a lane.  Every branch on the
// clip's descriptor is uniform over the workgroup.
//   the stream's own rate: each lane fetches its sample (one 4-byte load of L | R, or 2 bytes of a mono frame), converts,
//     stores -- no filter, no LDS;
//   another rate: the tile's outputs j0 .. j1 read input samples [n_lo, n_hi] = [q(j0) + d0, q(j1) + d0 + taps - 1].  With
//     PDMP3_AUDIO_LDS_X the span is fetched once, converted / downmixed, and kept in LDS as one plane per channel; with
//     PDMP3_AUDIO_LDS_TABLE the clip's whole table lies behind it (16-byte loads), else the lanes read their rows from
//     global memory (L2: every workgroup of the clip reads the same table).  A clip whose span does not fit LDS (a very
//     low output rate with a wide filter) takes resample_core.h audio_output per sample, straight from memory.
//   outputs at or behind the stream's end J are stored as 0.0; nothing at or behind n_samples is stored.
// Stores: lanes of a wave write 64 consecutive floats of one channel's row.
__global__ __launch_bounds__(kAudioThreads) void k_clip_audio(const pdmp3_audio_desc* __restrict__ descs, const uint32_t* __restrict__ frames,
                                                               const float* __restrict__ tables, long long n_samples, int channels) {
  extern __shared__ __align__(16) float lds[];
  const pdmp3_audio_desc d = descs[blockIdx.y];
  const long long t0 = (long long)blockIdx.x * kAudioTile;
  if (t0 >= n_samples) return;
  const int nt = n_samples - t0 < kAudioTile ? (int)(n_samples - t0) : kAudioTile;
  const long long j0 = d.start + t0;
  float* const out0 = reinterpret_cast<float*>(static_cast<uintptr_t>(d.dst)) + t0;
  float* const out1 = out0 + d.chan_stride;
  const int lane = threadIdx.x;

  if (d.M == d.L || j0 >= d.n_out || !(d.flags & PDMP3_AUDIO_LDS_X)) {
    for (int t = lane; t < nt; t += kAudioThreads) {
      out0[t] = audio_output(d, frames, tables, channels, j0 + t, 0);
      if (channels == 2) out1[t] = audio_output(d, frames, tables, channels, j0 + t, 1);
    }
    return;
  }

  // the valid outputs of the tile and the input span they read
  const int nv = d.n_out - j0 < nt ? (int)(d.n_out - j0) : nt;
  const long long q0 = (long long)(((unsigned long long)j0 * d.M) / d.L);
  const uint32_t r0 = (uint32_t)(((unsigned long long)j0 * d.M) % d.L);
  long long q1;
  uint32_t r1;
  audio_phase(d, q0, r0, nv - 1, &q1, &r1);
  const long long n_lo = q0 + d.d0;
  int span = (int)(q1 - q0) + d.taps;
  if (span > (int)d.span_cap) span = (int)d.span_cap;          // (the host sized the LDS by span_cap: never more)
  float* const x0 = lds;
  float* const x1 = lds + d.span_cap;
  for (int i = lane; i < span; i += kAudioThreads) {
    int l, r;
    float a, b;
    audio_fetch(d, frames, n_lo + i, &l, &r);
    audio_convert(l, r, channels, &a, &b);
    x0[i] = a;
    if (channels == 2) x1[i] = b;
  }
  const float* tab = tables + d.table;
  if (d.flags & PDMP3_AUDIO_LDS_TABLE) {
    float* const lt = lds + (size_t)d.span_cap * channels;     // (span_cap is a multiple of 4, d.table too: 16-byte rows)
    const unsigned n4 = (d.L * (unsigned)d.taps + 3u) >> 2;
    const float4* s4 = reinterpret_cast<const float4*>(tab);
    float4* d4 = reinterpret_cast<float4*>(lt);
    for (unsigned i = lane; i < n4; i += kAudioThreads) d4[i] = s4[i];
    tab = lt;
  }
  __syncthreads();
  for (int t = lane; t < nt; t += kAudioThreads) {
    float y0 = 0.0f, y1 = 0.0f;
    if (t < nv) {
      long long q;
      uint32_t r;
      audio_phase(d, q0, r0, t, &q, &r);
      const int at = (int)(q - q0);
      if (at + d.taps <= span) {                                // (always: the span ends with the last valid output's taps)
        const float* h = tab + (size_t)r * (unsigned)d.taps;
        y0 = audio_dot(h, x0 + at, d.taps);
        if (channels == 2) y1 = audio_dot(h, x1 + at, d.taps);
      }
    }
    out0[t] = y0;
    if (channels == 2) out1[t] = y1;
  }
}

}  // namespace

hipError_t pdmp3_launch_clip_audio(hipStream_t s, const pdmp3_audio_desc* descs, int n_clips, const uint32_t* frames, const float* tables,
                                   long long n_samples, int channels, unsigned lds_bytes) {
  if (n_clips <= 0 || n_samples <= 0) return hipSuccess;
  const unsigned tiles = (unsigned)((n_samples + pdmp3::kAudioTile - 1) / pdmp3::kAudioTile);
  hipLaunchKernelGGL(k_clip_audio, dim3(tiles, (unsigned)n_clips), dim3(pdmp3::kAudioThreads), lds_bytes, s, descs, frames, tables, n_samples,
                     channels);
  return hipGetLastError();
}
