// cqt.hip -- k_clip_cqt: rows of the resampled signal of a batch of clips (k_clip_audio's output in the stream object's third
// audio stage) to their constant-Q transform, planar float32 [n_bins][n_frames] per clip and channel -- complex
// ([n_bins][n_frames][2]), magnitude, power or its logarithm (include/pdmp3_bulk.h pdmp3_amd_bulk_decode_clips_cqt; DESIGN.md
// section 16).  Launched by stream.hip pdmp3_hip_clip_cqt.  A translation unit of its own; the span's load is clip_tile.h's,
// the rows of a tile and the loop over the tiles cqt_rows.h's (one source for this kernel and k_clip_chroma, which keeps the
// values this one stores); the span's indexing is mel_core.h's, what is stored stft_core.h's, the segments and the order of
// the partial sums cqt_core.h's.
#include <hip/hip_runtime.h>

#include "../../include/pdmp3_hip.h"
#include "cqt_rows.h"

namespace {

using namespace pdmp3;

// value i of a tile's 16 bins x 16 frames: the partial sums of `parts` waves added in cqt_reduce's order, turned into what is
// stored (stft_value; mode 0: the pair); consecutive lanes store consecutive frames of one bin.  Bins from n_bins on and
// frames from the tile's and from F on are not stored.
__device__ __forceinline__ void cqt_store(const pdmp3_cqt_params& P, float* out, const float* part, int parts, int t, long long f0, int i) {
  const int b = i >> 4, fl = i & 15, k = (t << 4) + b;
  const long long f = f0 + fl;
  const float re = cqt_reduce(part, cqt_part_at(b, fl), parts);
  const float im = cqt_reduce(part + kCqtPlane, cqt_part_at(b, fl), parts);
  if (k >= P.n_bins || fl >= P.tile || f >= P.n_frames) return;
  const size_t at = (size_t)k * (size_t)P.n_frames + (size_t)f;
  if (P.out_mode != 0) out[at] = stft_value(re, im, P.floor, P.out_mode);
  else *reinterpret_cast<f32x2*>(out + 2 * at) = f32x2{re, im};
}

// One workgroup of eight waves per (tile of P.tile frames, channel, clip).
//   1. the tile's span -- (tile - 1) hop + rows0 samples, zeros outside the clip's row -- goes to LDS once (mel_lds_at);
//   2. the first n_split tiles of 16 bins, the long ones: each wave takes one of eight runs of the tile's rows
//      (cqt_seg_begin) and writes its 16 x 16 partial sums of Re and of Im to its plane; after a barrier the first four waves
//      add the eight planes in one fixed order and store; a second barrier frees the planes;
//   3. the other tiles go whole to one wave each, round robin, through the wave's own plane: no workgroup barrier.
// (2 and 3 are cqt_rows.h's cqt_tiles with cqt_store for the sink.)
// The order of operations of a value depends on the plan alone: every frame's values come from the same chains whatever its
// place in a tile, clip or batch.
__device__ __forceinline__ void cqt_tile(const pdmp3_mel_desc& d, const float* __restrict__ tab, const pdmp3_cqt_params& P, int ch, long long f0,
                                         float* lds) {
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, j = lane & 15, kq = lane >> 4;
  const unsigned hop = (unsigned)P.hop, pad = (unsigned)P.row_pad, chunk = hop + pad;
  const int FT = P.tile;
  const unsigned jf = (unsigned)(j & (FT - 1));
  float* const span = lds;
  float* const part = lds + P.span_floats;
  float* const pw = part + wave * kCqtPart;
  const float* const row = reinterpret_cast<const float*>(static_cast<uintptr_t>(d.src)) + (size_t)ch * d.src_chan_stride;

  const unsigned n_span = (unsigned)(FT - 1) * hop + (unsigned)P.rows0;
  const unsigned last = mel_lds_at(n_span - 1, hop, pad);
  span_load<kCqtThreads>(span, row, P.n_in, f0, P.hop, pad, d.lead, n_span, tid);
  __syncthreads();

  float* const out = reinterpret_cast<float*>(static_cast<uintptr_t>(d.dst)) + (size_t)ch * d.dst_chan_stride;
  cqt_tiles(span, tab, P, hop, chunk, last, jf, tid, wave, lane, j, kq, part, pw,
            [&](const float* planes, int parts, int t, int i) { cqt_store(P, out, planes, parts, t, f0, i); });
}

// a workgroup's (tile, channel, clip)
__device__ __forceinline__ void cqt_entry(const pdmp3_mel_desc* __restrict__ descs, const float* __restrict__ tab, const pdmp3_cqt_params& P,
                                          float* lds) {
  const pdmp3_mel_desc d = descs[blockIdx.y];
  const int ch = blockIdx.x % P.channels;
  const long long f0 = (long long)(blockIdx.x / P.channels) * P.tile;
  if (f0 >= P.n_frames) return;
  cqt_tile(d, tab, P, ch, f0, lds);
}

__global__ __launch_bounds__(kCqtThreads) void k_clip_cqt(const pdmp3_mel_desc* __restrict__ descs, const float* __restrict__ tab,
                                                          pdmp3_cqt_params P) {
  extern __shared__ __align__(16) float lds[];
  cqt_entry(descs, tab, P, lds);
}

// A plan of more than the 64 KB a launch can ask for dynamically (the low octaves: C1 at 22 050 Hz is 95.5 KB): the same code
// on a static array of all the LDS a workgroup may have, one workgroup a CU.
__global__ __launch_bounds__(kCqtThreads) void k_clip_cqt_big(const pdmp3_mel_desc* __restrict__ descs, const float* __restrict__ tab,
                                                              pdmp3_cqt_params P) {
  __shared__ __align__(16) float lds[PDMP3_MEL_LDS_MAX / sizeof(float)];
  cqt_entry(descs, tab, P, lds);
}

}  // namespace

hipError_t pdmp3_launch_clip_cqt(hipStream_t s, const pdmp3_mel_desc* descs, int n_clips, const float* table, const pdmp3_cqt_params* params) {
  const pdmp3_cqt_params P = *params;
  if (n_clips <= 0 || P.n_frames <= 0) return hipSuccess;
  // a plan this file has no kernel for
  if ((P.tile != 16 && P.tile != 8 && P.tile != 4) || P.lds_bytes > PDMP3_MEL_LDS_MAX || P.n_tiles < 1 || P.n_tiles > PDMP3_CQT_MAX_TILES ||
      P.n_split < 0 || P.n_split > P.n_tiles)
    return hipErrorInvalidValue;
  return pdmp3::launch_clip_pair(k_clip_cqt, k_clip_cqt_big, s, pdmp3::kCqtThreads, P.n_frames, P.tile, P.channels, n_clips, P.lds_bytes, descs,
                                 table, P);
}
