// Host build of k_clip_chroma (pdmp3_amd/csrc/chroma.hip) for tests/test_clip_chroma_host.py: the kernel's own indexing and
// pointwise arithmetic (pdmp3_amd/csrc/mel_core.h, stft_core.h, cqt_core.h, chroma_core.h) driven by the kernel's structure --
// a workgroup per (tile of frames, channel, clip), LDS as a plain array with the kernel's regions (the span, a plane of partial
// sums a wave with the class plane over them, the q plane), each matrix instruction's result as the fused multiply-add chain
// it is (rows ascending), a split tile's rows cut into the eight waves' segments, the planes written as the lanes write them,
// and the fold, the norm and the quotient thread by thread as the 512 lanes take them.  The addresses in the descriptors are
// host addresses here.  The LDS is poisoned between the kernel's barriers where a region changes hands: a float read that
// nobody had written since ends the run with -1.
#include <stdint.h>

#include <vector>

#include "../../pdmp3_amd/csrc/chroma_core.h"

using namespace pdmp3;

static const float kPoison = -1e30f;

// rows [r0, r1) of tile t for the 16 lanes' frames into the wave's plane (tests/host_emul/cqt_emul.cpp's rows_of)
static int rows_of(const float* span, const float* tab, const pdmp3_cqt_params& P, int t, int r0, int r1, unsigned last, float* pw) {
  const unsigned hop = (unsigned)P.hop, pad = (unsigned)P.row_pad;
  const float* const tt = tab + (size_t)P.tile_at[t] * 32;
  for (int lane = 0; lane < 64; lane++) {
    const int j = lane & 15, kq = lane >> 4;
    for (int r = 0; r < 4; r++) {
      const int fl = 4 * kq + r;
      const unsigned jf = (unsigned)(fl & (P.tile - 1));
      float re = 0.0f, im = 0.0f;
      for (int n = r0; n < r1; n++) {
        unsigned at = mel_lds_at(jf * hop + (unsigned)P.tile_base[t] + (unsigned)n, hop, pad);
        if (at > last) at = last;
        const float a = span[at];
        if (a == kPoison) return -1;
        re = mel_fma(a, tt[(size_t)n * 32 + j], re);
        im = mel_fma(a, tt[(size_t)n * 32 + 16 + j], im);
      }
      pw[cqt_part_at(j, fl)] = re;
      pw[kCqtPlane + cqt_part_at(j, fl)] = im;
    }
  }
  return 0;
}

static int keep(const pdmp3_cqt_params& P, float* q, const float* part, int parts, int t, int i) {
  const int b = i >> 4, fl = i & 15;
  for (int s = 0; s < parts; s++)
    if (part[s * kCqtPart + cqt_part_at(b, fl)] == kPoison || part[s * kCqtPart + kCqtPlane + cqt_part_at(b, fl)] == kPoison) return -1;
  const float re = cqt_reduce(part, cqt_part_at(b, fl), parts);
  const float im = cqt_reduce(part + kCqtPlane, cqt_part_at(b, fl), parts);
  q[chroma_at((t << 4) + b, fl)] = stft_value(re, im, P.floor, P.out_mode);
  return 0;
}

static int workgroup(const pdmp3_mel_desc& d, const float* tab, const pdmp3_chroma_params& S, int ch, long long f0, std::vector<float>& lds) {
  const pdmp3_cqt_params& P = S.cqt;
  const unsigned hop = (unsigned)P.hop, pad = (unsigned)P.row_pad;
  lds.assign(P.lds_bytes / sizeof(float), kPoison);
  float* const span = lds.data();
  float* const part = lds.data() + P.span_floats;
  float* const q = lds.data() + S.q_at;
  float* const cls = lds.data() + S.class_at;
  const float* const row = reinterpret_cast<const float*>(static_cast<uintptr_t>(d.src)) + (size_t)ch * d.src_chan_stride;
  const unsigned n_span = (unsigned)(P.tile - 1) * hop + (unsigned)P.rows0;
  const unsigned last = mel_lds_at(n_span - 1, hop, pad);
  if ((size_t)last >= P.span_floats) return -1;
  for (unsigned p = 0; p < n_span; p++) span[mel_lds_at(p, hop, pad)] = mel_sample(row, P.n_in, f0, P.hop, d.lead, p);
  for (int t = 0; t < P.n_split; t++) {
    const int R = P.tile_rows[t];
    for (int i = 0; i < kCqtWaves * kCqtPart; i++) part[i] = kPoison;
    for (int wave = 0; wave < kCqtWaves; wave++)
      if (rows_of(span, tab, P, t, cqt_seg_begin(R, wave), cqt_seg_begin(R, wave + 1), last, part + wave * kCqtPart) != 0) return -1;
    for (int tid = 0; tid < 256; tid++)
      if (keep(P, q, part, kCqtWaves, t, tid) != 0) return -1;
  }
  for (int wave = 0; wave < kCqtWaves; wave++) {
    float* const pw = part + wave * kCqtPart;
    for (int t = P.n_split + wave; t < P.n_tiles; t += kCqtWaves) {
      for (int i = 0; i < kCqtPart; i++) pw[i] = kPoison;
      if (rows_of(span, tab, P, t, 0, P.tile_rows[t], last, pw) != 0) return -1;
      for (int i = 0; i < 256; i++)
        if (keep(P, q, pw, 1, t, i) != 0) return -1;
    }
  }
  // the barrier: the partial sums are free, the class plane takes their place
  for (int i = 0; i < kCqtWaves * kCqtPart; i++) part[i] = kPoison;
  for (int k = 0; k < P.n_bins; k++)
    for (int fl = 0; fl < 16; fl++)
      if (q[chroma_at(k, fl)] == kPoison) return -1;
  const int n_val = S.n_chroma << 4;
  for (int tid = 0; tid < kCqtThreads; tid++) {
    const int fl = tid & 15;
    for (int i = tid; i < n_val; i += kCqtThreads) cls[chroma_at(i >> 4, fl)] = chroma_fold(q, fl, i >> 4, P.n_bins, S.r, S.base_class, S.n_chroma);
  }
  // the second barrier
  float* const out = reinterpret_cast<float*>(static_cast<uintptr_t>(d.dst)) + (size_t)ch * d.dst_chan_stride;
  for (int tid = 0; tid < kCqtThreads; tid++) {
    const int fl = tid & 15;
    const long long f = f0 + fl;
    if (tid >= n_val || fl >= P.tile || f >= P.n_frames) continue;
    for (int p = 0; p < S.n_chroma; p++)
      if (cls[chroma_at(p, fl)] == kPoison) return -1;
    const float dn = S.chroma_norm ? chroma_norm_of(cls, fl, S.n_chroma, S.chroma_norm) : 0.0f;
    for (int i = tid; i < n_val; i += kCqtThreads) {
      const float c = cls[chroma_at(i >> 4, fl)];
      out[(size_t)(i >> 4) * (size_t)P.n_frames + (size_t)f] = S.chroma_norm ? chroma_quotient(c, dn, S.norm_floor) : c;
    }
  }
  return 0;
}

extern "C" int emul_chroma_desc_bytes() { return (int)sizeof(pdmp3_mel_desc); }
extern "C" int emul_chroma_params_bytes() { return (int)sizeof(pdmp3_chroma_params); }
// the class of bin k as the kernel's fold sees it: the p whose chroma_fold takes bin k (chroma_core.h's own map beside it)
extern "C" int emul_chroma_class(int k, int r, int base, int n_chroma) { return chroma_class(k, r, base, n_chroma); }
// 0, or -1 where the parameters would let the kernel leave its LDS or its table of table_rows rows
extern "C" int emul_clip_chroma(const pdmp3_mel_desc* descs, int n_clips, const float* tab, long long table_rows, const pdmp3_chroma_params* params) {
  const pdmp3_chroma_params& S = *params;
  const pdmp3_cqt_params& P = S.cqt;
  if (P.tile != 16 && P.tile != 8 && P.tile != 4) return -1;
  if (P.n_tiles < 1 || P.n_tiles > PDMP3_CQT_MAX_TILES || P.n_split < 0 || P.n_split > P.n_tiles || P.rows0 != P.tile_rows[0]) return -1;
  for (int t = 0; t < P.n_tiles; t++)
    if ((P.tile_rows[t] & 3) || P.tile_at[t] + (long long)P.tile_rows[t] > table_rows || P.tile_base[t] < 0 ||
        P.tile_base[t] + P.tile_rows[t] > P.rows0 + 3)
      return -1;
  const size_t span = (size_t)(P.tile - 1) * P.hop + P.rows0, chunks = (span + P.hop - 1) / P.hop;
  if (P.span_floats < chunks * (size_t)(P.hop + P.row_pad) || (P.span_floats & 3u) || P.lds_bytes > PDMP3_MEL_LDS_MAX) return -1;
  if (S.class_at != P.span_floats || S.q_at != P.span_floats + PDMP3_CQT_PART_FLOATS || (size_t)S.n_chroma * 17 > PDMP3_CQT_PART_FLOATS ||
      (size_t)P.lds_bytes < ((size_t)S.q_at + (size_t)P.n_tiles * 16 * 17) * sizeof(float))
    return -1;
  if ((P.out_mode != 1 && P.out_mode != 2) || S.n_chroma < 1 || S.r < 1 || S.base_class < 0 || S.base_class >= S.n_chroma) return -1;
  std::vector<float> lds;
  for (int k = 0; k < n_clips; k++)
    for (long long f0 = 0; f0 < P.n_frames; f0 += P.tile)
      for (int ch = 0; ch < P.channels; ch++)
        if (workgroup(descs[k], tab, S, ch, f0, lds) != 0) return -1;
  return 0;
}
