// mel_core.h -- the indexing and the pointwise arithmetic of k_clip_mel (mel.hip): where a sample of
// a tile's span lies in LDS, which sample of the clip's row it is, one step of the two dot products (the matrix instruction
// is this fused multiply-add chain, k ascending), the power, the floor and the logarithms, mode 3's finish and the integer
// form of its maximum.  One source for the kernel and for the host build the tests compile with g++
// (tests/host_emul/mel_emul.cpp), like resample_core.h.
#ifndef PDMP3_MEL_CORE_H
#define PDMP3_MEL_CORE_H
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/pdmp3_hip.h"

#if defined(__HIPCC__)
#define MEL_FN __host__ __device__ __forceinline__
#else
#define MEL_FN inline
#endif

namespace pdmp3 {

constexpr int kMelThreads = 256;            // lanes of a workgroup of k_clip_mel: four waves

// Position p of a tile's span (p = 0: the first sample of the tile's first frame) in LDS: chunks of `hop` samples lie
// hop + row_pad floats apart, so that the sixteen frames a matrix instruction reads at once fall into different banks.
MEL_FN unsigned mel_lds_at(unsigned p, unsigned hop, unsigned row_pad) { return p + (p / hop) * row_pad; }
// ... and the sample of the clip's row it holds: frame f0's sample n = p is row sample f0 hop - lead + p; zeros outside
// the row (in front of the stream, and behind the samples the call decoded)
MEL_FN float mel_sample(const float* row, long long n_in, long long f0, int hop, unsigned lead, unsigned p) {
  const long long t = f0 * hop - (long long)lead + (long long)p;
  return t >= 0 && t < n_in ? row[t] : 0.0f;
}
// one step of a dot product as the matrix instruction takes it
MEL_FN float mel_fma(float a, float b, float acc) { return __builtin_fmaf(a, b, acc); }
MEL_FN float mel_power(float re, float im) { return mel_fma(im, im, re * re); }
// what is stored for M in modes 0 .. 2; mode 3 stores M, and mel_whisper finishes it once the row's maximum is known
MEL_FN float mel_output(float m, float floor, int mode) {
  if (mode == 1) return logf(fmaxf(m, floor));
  if (mode == 2) return log10f(fmaxf(m, floor));
  return m;
}
// M >= 0: the order of the floats is the order of their bits
MEL_FN uint32_t mel_bits(float m) { uint32_t u; memcpy(&u, &m, 4); return u; }
MEL_FN float mel_from_bits(uint32_t u) { float m; memcpy(&m, &u, 4); return m; }
MEL_FN float mel_whisper(float m, float row_max, float floor) {
  const float g = log10f(fmaxf(row_max, floor));
  return (fmaxf(log10f(fmaxf(m, floor)), g - 8.0f) + 4.0f) * 0.25f;
}

}  // namespace pdmp3
#endif
