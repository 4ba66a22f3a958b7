// Host build of k_clip_audio (pdmp3_amd/csrc/resample.hip) for tests/test_clip_audio_host.py: the kernel's own arithmetic
// (pdmp3_amd/csrc/resample_core.h) driven by the kernel's loop structure -- a workgroup per (tile, clip), its lanes one after
// the other, LDS as a plain array.  The addresses in the descriptors are host addresses here.
#include <stdint.h>

#include <vector>

#include "../../pdmp3_amd/csrc/resample_core.h"

using namespace pdmp3;

static void workgroup(const pdmp3_audio_desc& d, const uint32_t* frames, const float* tables, long long n_samples, int channels, long long tile,
                      std::vector<float>& lds) {
  const long long t0 = tile * kAudioTile;
  const int nt = n_samples - t0 < kAudioTile ? (int)(n_samples - t0) : kAudioTile;
  const long long j0 = d.start + t0;
  float* const out0 = reinterpret_cast<float*>(static_cast<uintptr_t>(d.dst)) + t0;
  float* const out1 = out0 + d.chan_stride;
  if (d.M == d.L || j0 >= d.n_out || !(d.flags & PDMP3_AUDIO_LDS_X)) {
    for (int t = 0; t < nt; t++) {
      out0[t] = audio_output(d, frames, tables, channels, j0 + t, 0);
      if (channels == 2) out1[t] = audio_output(d, frames, tables, channels, j0 + t, 1);
    }
    return;
  }
  const int nv = d.n_out - j0 < nt ? (int)(d.n_out - j0) : nt;
  const long long q0 = (long long)(((unsigned long long)j0 * d.M) / d.L);
  const uint32_t r0 = (uint32_t)(((unsigned long long)j0 * d.M) % d.L);
  long long q1;
  uint32_t r1;
  audio_phase(d, q0, r0, nv - 1, &q1, &r1);
  const long long n_lo = q0 + d.d0;
  int span = (int)(q1 - q0) + d.taps;
  if (span > (int)d.span_cap) span = (int)d.span_cap;
  const size_t tab_floats = ((size_t)d.L * (size_t)d.taps + 3) & ~(size_t)3;
  lds.assign((size_t)d.span_cap * channels + ((d.flags & PDMP3_AUDIO_LDS_TABLE) ? tab_floats : 0), -1e30f);
  if (lds.size() * sizeof(float) > kAudioLdsMax) { for (int t = 0; t < nt; t++) out0[t] = -1e30f; return; }   // (the host's sizing is wrong)
  float* const x0 = lds.data();
  float* const x1 = x0 + d.span_cap;
  for (int i = 0; i < span; i++) {
    int l, r;
    float a, b;
    audio_fetch(d, frames, n_lo + i, &l, &r);
    audio_convert(l, r, channels, &a, &b);
    x0[i] = a;
    if (channels == 2) x1[i] = b;
  }
  const float* tab = tables + d.table;
  if (d.flags & PDMP3_AUDIO_LDS_TABLE) {
    float* const lt = x0 + (size_t)d.span_cap * channels;
    for (size_t i = 0; i < (size_t)d.L * (size_t)d.taps; i++) lt[i] = tab[i];
    tab = lt;
  }
  for (int t = 0; t < nt; t++) {
    float y0 = 0.0f, y1 = 0.0f;
    if (t < nv) {
      long long q;
      uint32_t r;
      audio_phase(d, q0, r0, t, &q, &r);
      const int at = (int)(q - q0);
      if (at + d.taps <= span) {
        const float* h = tab + (size_t)r * (unsigned)d.taps;
        y0 = audio_dot(h, x0 + at, d.taps);
        if (channels == 2) y1 = audio_dot(h, x1 + at, d.taps);
      } else {
        y0 = y1 = -1e30f;                      // (cannot happen: the test would see it)
      }
    }
    out0[t] = y0;
    if (channels == 2) out1[t] = y1;
  }
}

extern "C" int emul_audio_desc_bytes() { return (int)sizeof(pdmp3_audio_desc); }
extern "C" void emul_clip_audio(const pdmp3_audio_desc* descs, int n_clips, const uint32_t* frames, const float* tables, long long n_samples,
                                int channels) {
  std::vector<float> lds;
  for (int k = 0; k < n_clips; k++)
    for (long long tile = 0; tile * kAudioTile < n_samples; tile++) workgroup(descs[k], frames, tables, n_samples, channels, tile, lds);
}
