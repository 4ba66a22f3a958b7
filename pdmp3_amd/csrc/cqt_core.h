// cqt_core.h -- the indexing and the pointwise arithmetic of k_clip_cqt (cqt.hip).  The span's place in
// LDS, the sample of the clip's row it holds and one step of a dot product are k_clip_mel's (mel_core.h: mel_lds_at,
// mel_sample, mel_fma), what is stored for (Re, Im) is k_clip_stft's (stft_core.h: stft_value); here: the rows of a wave's
// segment of a split tile, where a wave's 16 bins x 16 frames of partial sums lie in LDS, and the one order in which they are
// added.  One source for the kernel and for the host build the tests compile with g++ (tests/host_emul/cqt_emul.cpp).
#ifndef PDMP3_CQT_CORE_H
#define PDMP3_CQT_CORE_H
#include "stft_core.h"

namespace pdmp3 {

constexpr int kCqtWaves = 8;
constexpr int kCqtThreads = 64 * kCqtWaves;
constexpr int kCqtPlane = 16 * 17;                 // 16 bins, 17 floats apart: a wave's Re plane; its Im plane follows
constexpr int kCqtPart = 2 * kCqtPlane;            // floats of a wave's partial sums

// rows of a segment of a split tile of R rows (R a multiple of 4): ceil(R / 8) rounded up to 4; segment s is rows
// [min(s q, R), min((s + 1) q, R))
MEL_FN int cqt_seg_rows(int R) { return (((R + kCqtWaves - 1) / kCqtWaves) + 3) & ~3; }
MEL_FN int cqt_seg_begin(int R, int s) { const int a = s * cqt_seg_rows(R); return a < R ? a : R; }
// where bin b (of the tile's 16) of frame fl (of the workgroup's 16) lies in a wave's plane
MEL_FN int cqt_part_at(int b, int fl) { return b * 17 + fl; }
// the value of `parts` waves' partial sums at `at`: ((p0 + p1) + p2) + ..., binary32 additions in this order and no other
MEL_FN float cqt_reduce(const float* part, int at, int parts) {
  float v = part[at];
  for (int s = 1; s < parts; s++) v = v + part[s * kCqtPart + at];
  return v;
}

}  // namespace pdmp3
#endif
