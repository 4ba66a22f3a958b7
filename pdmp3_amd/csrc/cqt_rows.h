// cqt_rows.h -- device code shared by k_clip_cqt (cqt.hip) and k_clip_chroma (chroma.hip): the rows of a tile of 16 bins times
// the workgroup's 16 frames, and the loop over a plan's tiles with its barriers.  One source, so that a bin's value of a frame
// is the same binary32 number in both kernels (DESIGN.md sections 16 and 17).  HIP only; the matrix instruction and the wave's
// own synchronisation are clip_tile.h's, the indexing and the arithmetic that the host build shares cqt_core.h's.
#ifndef PDMP3_CQT_ROWS_H
#define PDMP3_CQT_ROWS_H
#include "clip_tile.h"
#include "cqt_core.h"

namespace pdmp3 {

// Rows [r0, r1) of a tile of 16 bins (r0, r1 multiples of 4) times the 16 frames of the workgroup, Re and Im each one chain
// from +0, rows ascending, into the wave's plane `pw`.  The frames are overlapping rows of the span: the A operand is read at
// jf hop + base + n and never materialised; the B operand is the tile's rows of the table, read from memory (L2): four rows of
// 32 floats a step.  Lanes of frames from FT on (tiles of 8 and 4 frames) read frame j mod FT again: nothing of theirs is stored.
// A shorter tile's padding rows (up to three, exact zeros) may stand behind the span's last sample: the read stops at `last`,
// the span's last float, and the finite sample there times the zero adds nothing.
__device__ __forceinline__ void cqt_rows(const float* span, const float* __restrict__ tile_tab, unsigned base, int r0, int r1, unsigned hop,
                                         unsigned chunk, unsigned last, unsigned jf, int j, int kq, float* pw) {
  f32x4 re = f32x4{0.0f, 0.0f, 0.0f, 0.0f}, im = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  const unsigned q = base + (unsigned)r0 + (unsigned)kq;
  unsigned c = jf + q / hop, rem = q % hop;
  const float* bp = tile_tab + (size_t)(r0 + kq) * 32 + j;
  // one step: four rows of the table times the sixteen frames' four samples, on top of the two chains
  auto step = [&](float b_re, float b_im) {
    const float a = span[min(c * chunk + rem, last)];
    re = mfma16(a, b_re, re);
    im = mfma16(a, b_im, im);
    rem += 4;
    if (rem >= hop) {
      if (hop >= 4) { rem -= hop; c++; }
      else { c += rem / hop; rem %= hop; }
    }
  };
  // blocks of kU steps: the next block's coefficients are on their way from L2 while this block's matrix instructions run
  constexpr int kU = 8;
  const int blocks = (r1 - r0) / (4 * kU);
  float cre[kU], cim[kU], nre[kU], nim[kU];
  if (blocks > 0) {
#pragma unroll
    for (int u = 0; u < kU; u++) { cre[u] = bp[128 * u]; cim[u] = bp[128 * u + 16]; }
    bp += 128 * kU;
  }
  for (int b = 0; b < blocks; b++) {
    if (b + 1 < blocks) {
#pragma unroll
      for (int u = 0; u < kU; u++) { nre[u] = bp[128 * u]; nim[u] = bp[128 * u + 16]; }
      bp += 128 * kU;
    }
#pragma unroll
    for (int u = 0; u < kU; u++) step(cre[u], cim[u]);
#pragma unroll
    for (int u = 0; u < kU; u++) { cre[u] = nre[u]; cim[u] = nim[u]; }
  }
  for (int n = r0 + 4 * kU * blocks; n < r1; n += 4) {
    step(bp[0], bp[16]);
    bp += 128;
  }
#pragma unroll
  for (int r = 0; r < 4; r++) {
    pw[cqt_part_at(j, 4 * kq + r)] = re[r];
    pw[kCqtPlane + cqt_part_at(j, 4 * kq + r)] = im[r];
  }
}

// The tiles of a plan, the span being in LDS.
//   - the first n_split tiles of 16 bins, the long ones: each wave takes one of eight runs of the tile's rows (cqt_seg_begin)
//     and writes its 16 x 16 partial sums of Re and of Im to its plane `pw` of `part`; after a barrier the first four waves
//     hand the eight planes' 256 values to the sink; a second barrier frees the planes;
//   - the other tiles go whole to one wave each, round robin, through the wave's own plane: no workgroup barrier.
// sink(planes, parts, t, i): value i of tile t's 16 bins x 16 frames, to be added over `parts` planes in cqt_reduce's order.
template <class Sink>
__device__ __forceinline__ void cqt_tiles(const float* span, const float* __restrict__ tab, const pdmp3_cqt_params& P, unsigned hop, unsigned chunk,
                                          unsigned last, unsigned jf, int tid, int wave, int lane, int j, int kq, float* part, float* pw,
                                          Sink sink) {
  for (int t = 0; t < P.n_split; t++) {
    const int R = P.tile_rows[t];
    cqt_rows(span, tab + (size_t)P.tile_at[t] * 32, (unsigned)P.tile_base[t], cqt_seg_begin(R, wave), cqt_seg_begin(R, wave + 1), hop, chunk, last,
             jf, j, kq, pw);
    __syncthreads();
    if (tid < 256) sink(part, kCqtWaves, t, tid);
    __syncthreads();                                   // (the next tile's partial sums go to the same planes)
  }
  for (int t = P.n_split + wave; t < P.n_tiles; t += kCqtWaves) {
    cqt_rows(span, tab + (size_t)P.tile_at[t] * 32, (unsigned)P.tile_base[t], 0, P.tile_rows[t], hop, chunk, last, jf, j, kq, pw);
    wave_sync();
#pragma unroll
    for (int it = 0; it < 4; it++) sink(pw, 1, t, 64 * it + lane);
    wave_sync();
  }
}

}  // namespace pdmp3
#endif
