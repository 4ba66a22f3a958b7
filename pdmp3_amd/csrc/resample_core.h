// resample_core.h -- the arithmetic of k_clip_audio (resample.hip): where a per-channel sample of a
// clip's staged int16 PCM lies, its conversion / downmix to float, the phase of an output sample and the dot product with
// its row of the filter table.  One source for the kernel and for the host build the tests compile with g++
// (tests/host_emul/resample_emul.cpp), like decode_core.h and unpack_core.h.
#ifndef PDMP3_RESAMPLE_CORE_H
#define PDMP3_RESAMPLE_CORE_H
#include <stdint.h>

#include "../../include/pdmp3_hip.h"

#if defined(__HIPCC__)
#define RS_FN __host__ __device__ __forceinline__
#else
#define RS_FN inline
#endif

namespace pdmp3 {

constexpr int kAudioThreads = 256;          // lanes of a workgroup of k_clip_audio
constexpr int kAudioTile = PDMP3_AUDIO_TILE; // output samples (per channel) of a workgroup: four a lane
constexpr unsigned kAudioLdsMax = PDMP3_AUDIO_LDS_BYTES;

// Per-channel sample n of the clip's stream as the two int16 values of its channels (a mono frame gives its sample to
// both); 0, 0 outside the stream's [0, N) and outside the staged frames (which only taps with a zero coefficient reach).
// frames[]: per staged frame (its PCM's offset in the clip's stage in units of 1152 bytes) << 1 | mono.
RS_FN void audio_fetch(const pdmp3_audio_desc& d, const uint32_t* frames, long long n, int* l, int* r) {
  *l = *r = 0;
  if (n < 0 || n >= d.n_in) return;
  const long long f = n / d.spf - d.frame0;
  if (f < 0 || f >= (long long)d.n_frames) return;
  const unsigned i = (unsigned)(n % d.spf);
  const uint32_t e = frames[d.frame_tab + f];
  const uint8_t* p = reinterpret_cast<const uint8_t*>(static_cast<uintptr_t>(d.src)) + (size_t)(e >> 1) * 1152u;
  if (e & 1u) {
    *l = *r = reinterpret_cast<const int16_t*>(p)[i];
  } else {
    const uint32_t v = reinterpret_cast<const uint32_t*>(p)[i];      // L | R << 16: one load
    *l = (int16_t)(v & 0xffffu);
    *r = (int16_t)(v >> 16);
  }
}
// ... as the floats of the call's C channels: C == 1: (l + r) / 65536 (exact in binary32; a mono frame's own sample / 32768),
// C == 2: l / 32768, r / 32768
RS_FN void audio_convert(int l, int r, int channels, float* x0, float* x1) {
  if (channels == 1) { *x0 = (float)(l + r) * (1.0f / 65536.0f); *x1 = 0.0f; }
  else { *x0 = (float)l * (1.0f / 32768.0f); *x1 = (float)r * (1.0f / 32768.0f); }
}
// the taps of a row against `taps` consecutive samples, in binary32
RS_FN float audio_dot(const float* h, const float* x, int taps) {
  float acc = 0.0f;
  for (int k = 0; k < taps; k++) acc += h[k] * x[k];
  return acc;
}
// Output sample j = j0 + t of a tile that starts at j0 = q0 L + r0 (j0 M = q0 L + r0, 0 <= r0 < L): j M = q L + r.  The
// row of the table is r, its first tap multiplies input sample q + d0.  t < kAudioTile and M <= 48000: 32 bits hold r0 + t M.
RS_FN void audio_phase(const pdmp3_audio_desc& d, long long q0, uint32_t r0, int t, long long* q, uint32_t* r) {
  const uint32_t x = r0 + (uint32_t)t * d.M;
  *q = q0 + x / d.L;
  *r = x % d.L;
}
// One output sample of channel c straight from the staged PCM and the table in memory: what the kernel does for a clip
// whose input span does not fit LDS, and the definition its LDS form must agree with.
RS_FN float audio_output(const pdmp3_audio_desc& d, const uint32_t* frames, const float* table, int channels, long long j, int c) {
  if (j >= d.n_out) return 0.0f;                     // padding behind the stream's end
  int l, r;
  float x0, x1;
  if (d.M == d.L) {                                  // the stream's own rate: no filter
    audio_fetch(d, frames, j, &l, &r);
    audio_convert(l, r, channels, &x0, &x1);
    return c ? x1 : x0;
  }
  const long long q = (long long)(((unsigned long long)j * d.M) / d.L);
  const uint32_t ph = (uint32_t)(((unsigned long long)j * d.M) % d.L);
  const float* h = table + d.table + (size_t)ph * (unsigned)d.taps;
  float acc = 0.0f;
  for (int k = 0; k < d.taps; k++) {
    audio_fetch(d, frames, q + d.d0 + k, &l, &r);
    audio_convert(l, r, channels, &x0, &x1);
    acc += h[k] * (c ? x1 : x0);
  }
  return acc;
}

}  // namespace pdmp3
#endif
