// chroma.hip -- k_clip_chroma: rows of the resampled signal of a batch of clips (k_clip_audio's output in the stream object's
// third audio stage) to pitch-class profiles, planar float32 [n_chroma][n_frames] per clip and channel
// (include/pdmp3_bulk.h pdmp3_amd_bulk_decode_clips_chroma).  Launched by stream.hip
// pdmp3_hip_clip_chroma.  A translation unit of its own.  The span's load is clip_tile.h's and the tile loop cqt_rows.h's
// cqt_tiles, one source for this kernel and k_clip_cqt: the same rows, segments and order of the partial sums (cqt_core.h) and
// the same stft_value (stft_core.h), so a bin's value of a frame is the binary32 number k_clip_cqt stores; it goes to LDS,
// and the fold, the norms and the quotient behind it are chroma_core.h's.
#include <hip/hip_runtime.h>

#include "../../include/pdmp3_hip.h"
#include "chroma_core.h"
#include "cqt_rows.h"

namespace {

using namespace pdmp3;

// value i of a tile's 16 bins x 16 frames, where cqt.hip's cqt_store stores it: the partial sums of `parts` waves added in
// cqt_reduce's order and turned into the magnitude or the power by stft_value -- into the q plane.  All 16 x 16 values of
// every tile are written (padding bins: +0 from the table's zero columns; frames from the tile's on: a frame again), so the
// fold reads nothing that was not written; what it reads are bins below n_bins alone.
__device__ __forceinline__ void chroma_keep(const pdmp3_cqt_params& P, float* q, const float* part, int parts, int t, int i) {
  const int b = i >> 4, fl = i & 15;
  const float re = cqt_reduce(part, cqt_part_at(b, fl), parts);
  const float im = cqt_reduce(part + kCqtPlane, cqt_part_at(b, fl), parts);
  q[chroma_at((t << 4) + b, fl)] = stft_value(re, im, P.floor, P.out_mode);
}

// One workgroup of eight waves per (tile of P.tile frames, channel, clip).
//   1. - 3. as cqt.hip's cqt_tile (cqt_tiles with chroma_keep for the sink): the span to LDS once, the split tiles over the
//      eight waves' segments of rows and their planes added in one fixed order, the other tiles whole to one wave each,
//      round robin -- every value to the q plane;
//   4. a barrier; value i = 16 p + fl of the n_chroma x 16: the bins of class p of frame fl added in ascending k
//      (chroma_fold), into the class plane, which lies over the partial sums: nobody reads those behind the barrier;
//   5. a barrier; each lane forms its frame's d over the classes in ascending order (chroma_norm_of) and stores
//      c_p / max(d, floor) for its classes; consecutive lanes store consecutive frames of one class.
// The order of operations of a value depends on the spec alone.
__device__ __forceinline__ void chroma_tile(const pdmp3_mel_desc& d, const float* __restrict__ tab, const pdmp3_chroma_params& S, int ch,
                                            long long f0, float* lds) {
  const pdmp3_cqt_params& P = S.cqt;
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, j = lane & 15, kq = lane >> 4;
  const unsigned hop = (unsigned)P.hop, pad = (unsigned)P.row_pad, chunk = hop + pad;
  const int FT = P.tile;
  const unsigned jf = (unsigned)(j & (FT - 1));
  float* const span = lds;
  float* const part = lds + P.span_floats;
  float* const pw = part + wave * kCqtPart;
  float* const q = lds + S.q_at;
  float* const cls = lds + S.class_at;
  const float* const row = reinterpret_cast<const float*>(static_cast<uintptr_t>(d.src)) + (size_t)ch * d.src_chan_stride;

  const unsigned n_span = (unsigned)(FT - 1) * hop + (unsigned)P.rows0;
  const unsigned last = mel_lds_at(n_span - 1, hop, pad);
  span_load<kCqtThreads>(span, row, P.n_in, f0, P.hop, pad, d.lead, n_span, tid);
  __syncthreads();

  cqt_tiles(span, tab, P, hop, chunk, last, jf, tid, wave, lane, j, kq, part, pw,
            [&](const float* planes, int parts, int t, int i) { chroma_keep(P, q, planes, parts, t, i); });
  __syncthreads();                                     // the q plane is whole, the partial sums are free

  const int n_val = S.n_chroma << 4, fl = tid & 15;    // (512 is a multiple of 16: a lane's values are all of frame fl)
  for (int i = tid; i < n_val; i += kCqtThreads) cls[chroma_at(i >> 4, fl)] = chroma_fold(q, fl, i >> 4, P.n_bins, S.r, S.base_class, S.n_chroma);
  __syncthreads();

  const long long f = f0 + fl;
  if (tid >= n_val || fl >= FT || f >= P.n_frames) return;
  float* const out = reinterpret_cast<float*>(static_cast<uintptr_t>(d.dst)) + (size_t)ch * d.dst_chan_stride;
  const float dn = S.chroma_norm ? chroma_norm_of(cls, fl, S.n_chroma, S.chroma_norm) : 0.0f;
  for (int i = tid; i < n_val; i += kCqtThreads) {
    const float c = cls[chroma_at(i >> 4, fl)];
    out[(size_t)(i >> 4) * (size_t)P.n_frames + (size_t)f] = S.chroma_norm ? chroma_quotient(c, dn, S.norm_floor) : c;
  }
}

// a workgroup's (tile, channel, clip)
__device__ __forceinline__ void chroma_entry(const pdmp3_mel_desc* __restrict__ descs, const float* __restrict__ tab, const pdmp3_chroma_params& S,
                                             float* lds) {
  const pdmp3_mel_desc d = descs[blockIdx.y];
  const int ch = blockIdx.x % S.cqt.channels;
  const long long f0 = (long long)(blockIdx.x / S.cqt.channels) * S.cqt.tile;
  if (f0 >= S.cqt.n_frames) return;
  chroma_tile(d, tab, S, ch, f0, lds);
}

__global__ __launch_bounds__(kCqtThreads) void k_clip_chroma(const pdmp3_mel_desc* __restrict__ descs, const float* __restrict__ tab,
                                                             pdmp3_chroma_params S) {
  extern __shared__ __align__(16) float lds[];
  chroma_entry(descs, tab, S, lds);
}

// A plan of more than the 64 KB a launch can ask for dynamically: the same code on a static array of all the LDS a workgroup
// may have, one workgroup a CU.
__global__ __launch_bounds__(kCqtThreads) void k_clip_chroma_big(const pdmp3_mel_desc* __restrict__ descs, const float* __restrict__ tab,
                                                                 pdmp3_chroma_params S) {
  __shared__ __align__(16) float lds[PDMP3_MEL_LDS_MAX / sizeof(float)];
  chroma_entry(descs, tab, S, lds);
}

}  // namespace

hipError_t pdmp3_launch_clip_chroma(hipStream_t s, const pdmp3_mel_desc* descs, int n_clips, const float* table, const pdmp3_chroma_params* params) {
  const pdmp3_chroma_params S = *params;
  const pdmp3_cqt_params& P = S.cqt;
  if (n_clips <= 0 || P.n_frames <= 0) return hipSuccess;
  // a plan this file has no kernel for
  if ((P.tile != 16 && P.tile != 8 && P.tile != 4) || P.lds_bytes > PDMP3_MEL_LDS_MAX || P.n_tiles < 1 || P.n_tiles > PDMP3_CQT_MAX_TILES ||
      P.n_split < 0 || P.n_split > P.n_tiles || (P.out_mode != 1 && P.out_mode != 2) || S.n_chroma < 1 || S.r < 1)
    return hipErrorInvalidValue;
  return pdmp3::launch_clip_pair(k_clip_chroma, k_clip_chroma_big, s, pdmp3::kCqtThreads, P.n_frames, P.tile, P.channels, n_clips, P.lds_bytes,
                                 descs, table, S);
}
