// stft.hip -- k_clip_stft: rows of the resampled signal of a batch of clips (k_clip_audio's output in the stream object's
// third audio stage) to their short-time Fourier transform, planar float32 [bins][n_frames] per clip and channel -- complex
// ([bins][n_frames][2]), magnitude, power or its logarithm (include/pdmp3_bulk.h pdmp3_amd_bulk_decode_clips_stft; DESIGN.md
// section 13).  Launched by stream.hip pdmp3_hip_clip_stft.  A translation unit of its own; the span's load and the DFT are
// k_clip_mel's: clip_tile.h's, one source inlined here, which leaves a tile of bins' Re and Im in registers; the span's indexing
// is mel_core.h's, the pointwise arithmetic and the staging layout stft_core.h's.
#include <hip/hip_runtime.h>

#include "../../include/pdmp3_hip.h"
#include "clip_tile.h"
#include "stft_core.h"

namespace {

using namespace pdmp3;

// One workgroup of four waves per (tile of 16 RT frames, channel, clip).
//   1. the tile's span -- (tile - 1) hop + rows samples, zeros outside the clip's row -- goes to LDS once (mel_lds_at);
//   2. DFT, as k_clip_mel's (tile_dft, a tile of 16 bins a call): the frames are overlapping rows of the span, the A operand is
//      read at f hop + n and never materialised; the B operand is the folded table (window and scale in it), read from memory
//      (L2).  A wave takes every fourth tile of 16 bins, Re and Im of all RT row tiles in registers;
//   3. the wave turns them into what is stored (stft_value; mode 0: the pair) in registers and transposes its 16 bins x
//      tile frames through its own staging tile (stft_core.h has the layout and its banks): no workgroup barrier;
//   4. consecutive lanes store consecutive frames of one bin, mode 0 consecutive (Re, Im) pairs.  Bins from K on and frames
//      from F on are not stored.
// Every frame's values come from the same chains of operations whatever its place in the tile.
template <int RT>
__device__ __forceinline__ void stft_tile(const pdmp3_mel_desc& d, const float* __restrict__ tab, const pdmp3_stft_params& P, int ch,
                                          long long f0, float* lds) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 15, kq = lane >> 4;
  const unsigned hop = (unsigned)P.hop, pad = (unsigned)P.row_pad, chunk = hop + pad;
  constexpr int FT = 16 * RT;
  const int Kp = P.bins16, S = stft_stage_stride(FT), mode = P.out_mode;
  float* const span = lds;
  float* const st = lds + P.span_floats + wave * stft_stage_floats(FT, mode);
  const float* const row = reinterpret_cast<const float*>(static_cast<uintptr_t>(d.src)) + (size_t)ch * d.src_chan_stride;

  span_load<kStftThreads>(span, row, P.n_in, f0, P.hop, pad, d.lead, (unsigned)(FT - 1) * hop + (unsigned)P.rows, tid);
  __syncthreads();

  float* const out = reinterpret_cast<float*>(static_cast<uintptr_t>(d.dst)) + (size_t)ch * d.dst_chan_stride;
  for (int bt = wave; bt < (Kp >> 4); bt += 4) {
    f32x4 re[RT], im[RT];
    tile_dft<RT>(span, tab, P.rows, Kp, hop, chunk, bt, j, kq, re, im);
    // the lane's four frames of bin j, rt by rt: one 16-byte store a plane
    float* const sp = st + j * S + 4 * kq;
#pragma unroll
    for (int rt = 0; rt < RT; rt++) {
      if (mode == 0) {
        *reinterpret_cast<f32x4*>(sp + 16 * rt) = re[rt];
        *reinterpret_cast<f32x4*>(sp + 16 * S + 16 * rt) = im[rt];
      } else {
        f32x4 v;
#pragma unroll
        for (int r = 0; r < 4; r++) v[r] = stft_value(re[rt][r], im[rt][r], P.floor, mode);
        *reinterpret_cast<f32x4*>(sp + 16 * rt) = v;
      }
    }
    wave_sync();
#pragma unroll
    for (int it = 0; it < 16 * FT / 64; it++) {
      const int i = 64 * it + lane, b = stft_stage_row(i / FT, FT), fl = i % FT, k = (bt << 4) + b;
      const long long f = f0 + fl;
      const float v0 = st[b * S + fl];
      const float v1 = mode == 0 ? st[16 * S + b * S + fl] : 0.0f;
      if (k >= P.bins || f >= P.n_frames) continue;
      const size_t at = (size_t)k * (size_t)P.n_frames + (size_t)f;
      if (mode != 0) out[at] = v0;
      else *reinterpret_cast<f32x2*>(out + 2 * at) = f32x2{v0, v1};
    }
    wave_sync();                                       // (the next tile of bins goes to the same staging tile)
  }
}

// a workgroup's (tile, channel, clip) and its tile of `tile` frames
__device__ __forceinline__ void stft_entry(const pdmp3_mel_desc* __restrict__ descs, const float* __restrict__ tab, const pdmp3_stft_params& P,
                                           int tile, float* lds) {
  const pdmp3_mel_desc d = descs[blockIdx.y];
  const int ch = blockIdx.x % P.channels;
  const long long f0 = (long long)(blockIdx.x / P.channels) * tile;
  if (f0 >= P.n_frames) return;
  if (tile == 32) stft_tile<2>(d, tab, P, ch, f0, lds);
  else stft_tile<1>(d, tab, P, ch, f0, lds);
}

__global__ __launch_bounds__(kStftThreads) void k_clip_stft(const pdmp3_mel_desc* __restrict__ descs, const float* __restrict__ tab,
                                                            pdmp3_stft_params P) {
  extern __shared__ __align__(16) float lds[];
  stft_entry(descs, tab, P, P.tile, lds);
}

// A tile of 16 frames that needs more than the 64 KB a launch can ask for dynamically (n_fft = 1024 at hops from about 900
// on): the same code on a static array of all the LDS a workgroup may have, one workgroup a CU.
__global__ __launch_bounds__(kStftThreads) void k_clip_stft_big(const pdmp3_mel_desc* __restrict__ descs, const float* __restrict__ tab,
                                                                pdmp3_stft_params P) {
  __shared__ __align__(16) float lds[PDMP3_MEL_LDS_MAX / sizeof(float)];
  stft_entry(descs, tab, P, 16, lds);
}

}  // namespace

hipError_t pdmp3_launch_clip_stft(hipStream_t s, const pdmp3_mel_desc* descs, int n_clips, const float* table, const pdmp3_stft_params* params) {
  const pdmp3_stft_params P = *params;
  if (n_clips <= 0 || P.n_frames <= 0) return hipSuccess;
  if (P.lds_bytes > PDMP3_MEL_LDS_SOFT && (P.tile != 16 || P.lds_bytes > PDMP3_MEL_LDS_MAX)) return hipErrorInvalidValue;
  return pdmp3::launch_clip_pair(k_clip_stft, k_clip_stft_big, s, pdmp3::kStftThreads, P.n_frames, P.tile, P.channels, n_clips, P.lds_bytes,
                                 descs, table, P);
}
