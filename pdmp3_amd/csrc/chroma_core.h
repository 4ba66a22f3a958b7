// chroma_core.h -- the indexing and the pointwise arithmetic of k_clip_chroma (chroma.hip).  The transform
// in front of it is k_clip_cqt's (cqt_core.h: the segments, the planes of partial sums and their one order; stft_core.h:
// stft_value); here: where a bin's value of a frame lies in the q plane, the class of a bin, the fold of a class's bins in
// ascending order, the three norms over the classes and the quotient.  One source for the kernel and for the host build the
// tests compile with g++ (tests/host_emul/chroma_emul.cpp).
#ifndef PDMP3_CHROMA_CORE_H
#define PDMP3_CHROMA_CORE_H
#include "cqt_core.h"

namespace pdmp3 {

// where bin k (of all the bins) or class p of frame fl (of the workgroup's 16) lies in its plane: cqt_core.h's stride, so the
// sixteen lanes that hold sixteen bins of a frame write sixteen banks, and sixteen lanes of one bin sixteen consecutive ones
MEL_FN int chroma_at(int k, int fl) { return k * 17 + fl; }
// group g = (k + r / 2) / r holds the r bins about bin g r (r = 3: g r - 1, g r, g r + 1); its class is g + base mod n_chroma
MEL_FN int chroma_class(int k, int r, int base, int n_chroma) { return ((k + r / 2) / r + base) % n_chroma; }

// c_p of frame fl: the bins of class p in ascending k -- groups g = g0, g0 + n_chroma, ... with g0 = p - base mod n_chroma, each
// its bins [g r - r / 2, g r - r / 2 + r) inside [0, n_bins) -- from the first term on by plain additions; +0 without a bin
MEL_FN float chroma_fold(const float* q, int fl, int p, int n_bins, int r, int base, int n_chroma) {
  float c = 0.0f;
  bool first = true;
  for (int g = (p - base + n_chroma) % n_chroma; g * r - r / 2 < n_bins; g += n_chroma) {
    const int a = g * r - r / 2, b = a + r < n_bins ? a + r : n_bins;
    for (int k = a < 0 ? 0 : a; k < b; k++) {
      const float v = q[chroma_at(k, fl)];
      c = first ? v : c + v;
      first = false;
    }
  }
  return c;
}

// d of frame fl over the classes p = 0 .. n_chroma - 1 ascending: 1 L1 ((c_0 + c_1) + c_2) + ... (every c_p >= 0), 2 L2 the
// correctly rounded sqrtf of s = c_0 c_0, s = fma(c_p, c_p, s), 3 the maximum
MEL_FN float chroma_norm_of(const float* cls, int fl, int n_chroma, int norm) {
  const float c0 = cls[chroma_at(0, fl)];
  float d = norm == 2 ? c0 * c0 : c0;
  for (int p = 1; p < n_chroma; p++) {
    const float c = cls[chroma_at(p, fl)];
    d = norm == 1 ? d + c : norm == 2 ? mel_fma(c, c, d) : fmaxf(d, c);
  }
  return norm == 2 ? sqrtf(d) : d;
}

// what is stored: c / max(d, floor), one correctly rounded division; no branch on d other than the max
MEL_FN float chroma_quotient(float c, float d, float floor) { return c / fmaxf(d, floor); }

}  // namespace pdmp3
#endif
