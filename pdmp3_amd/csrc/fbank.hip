// fbank.hip -- k_clip_fbank: rows of the resampled signal of a batch of clips (k_clip_audio's output in the stream object's
// third audio stage) to Kaldi-style filterbank features, planar float32 [n_frames][D] per clip and channel, coefficients
// innermost (include/pdmp3_bulk.h pdmp3_amd_bulk_decode_clips_fbank).  Launched by stream.hip
// pdmp3_hip_clip_fbank.  A translation unit of its own; the span's load and the two matrix stages are k_clip_mel's, the energy
// stage, the column sums and the finishing pass k_clip_mfcc's too: all of them clip_tile.h's, one source inlined here, so that
// a change to a stage is made once and k_clip_mfcc's stages 1 .. 4 stay these bit for bit; the indexing and pointwise
// arithmetic are mel_core.h's and fbank_core.h's.
#include <hip/hip_runtime.h>

#include "../../include/pdmp3_hip.h"
#include "clip_tile.h"

namespace {

using namespace pdmp3;

// One workgroup of four waves per (tile of P.tile = 16 RT frames, channel, clip).
//   1. the tile's span -- (tile - 1) hop + rows samples from the clip's row, zeros behind it -- goes to LDS once (mel_lds_at);
//   2. energy (use_energy; tile_energy): a wave per frame, the mean and then sum (s - mean)^2 in a fixed lane and shuffle
//      order; a frame's value does not depend on its place.  It waits in the spare float behind the frame's row of powers;
//   3. DFT (tile_dft_power): the frames are overlapping rows of the span; the B operand is the folded table (DC removal,
//      pre-emphasis, window and zero padding in it) from memory, `rows` rows of it.  Re^2 + Im^2 goes to LDS [frame][bin];
//   4. filterbank (tile_filterbank): A = the powers, B = the transposed padded filterbank from memory; the mel tile goes to LDS
//      [band][frames + 1] over the span, which nobody reads any more;
//   5. floor, logarithm, stores: consecutive lanes write consecutive coefficients of one frame (the odd stride of the mel tile
//      keeps those LDS reads free of bank conflicts); the energy goes into its column;
//   6. subtract_mean: the stored values go back to LDS, and a lane per column adds those of the frames f < valid, in frame
//      order, into the tile's row `ts` of the launch's scratch (tile_sums); k_clip_fbank_finish does the rest.
template <int RT>
__device__ __forceinline__ void fbank_tile(const pdmp3_fbank_desc& d, const float* __restrict__ dft, const float* __restrict__ fbt,
                                           const pdmp3_fbank_params& P, int ch, long long f0, float* __restrict__ ts, float* lds) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 15, kq = lane >> 4;
  const unsigned hop = (unsigned)P.hop, pad = (unsigned)P.row_pad, chunk = hop + pad;
  const int Kp = P.bins16, Mp = P.mels16, PS = Kp + 2, FT = 16 * RT, FTS = FT + 1;
  float* const span = lds;
  float* const pw = lds + P.span_floats;
  const float* const row = reinterpret_cast<const float*>(static_cast<uintptr_t>(d.src)) + (size_t)ch * d.src_chan_stride;

  span_load<kMelThreads>(span, row, P.n_in, f0, P.hop, pad, 0u, (unsigned)(FT - 1) * hop + (unsigned)P.rows, tid);
  __syncthreads();

  tile_energy(span, P, FT, hop, pad, wave, lane, pw, PS, Kp);
  tile_dft_power<RT>(span, dft, P.rows, Kp, hop, chunk, wave, j, kq, pw, PS);
  __syncthreads();

  float* const mt = lds;                               // [Mp][FTS]
  tile_filterbank<RT>(pw, PS, fbt, Kp, Mp, wave, j, kq, mt, FTS);
  __syncthreads();

  float* const out = reinterpret_cast<float*>(static_cast<uintptr_t>(d.dst)) + (size_t)ch * d.dst_chan_stride;
  const int D = P.n_mels + P.use_energy;
  for (int i = tid; i < D * FT; i += kMelThreads) {
    const int fl = i / D, dc = i - fl * D;
    const long long f = f0 + fl;
    if (f >= P.n_frames) break;                        // (frames ascend with i)
    const int m = fbank_column_band(dc, P.n_mels, P.use_energy, P.htk_compat);
    float* const at = m < 0 ? pw + fl * PS + Kp : mt + m * FTS + fl;
    const float v = m < 0 ? fbank_energy_output(*at, P.eps, P.energy_log_floor, P.out_mode) : mel_output(*at, P.eps, P.out_mode);
    if (P.subtract_mean) *at = v;
    out[(size_t)f * (size_t)D + (size_t)dc] = v;
  }
  if (!P.subtract_mean) return;
  __syncthreads();
  tile_sums(ts, D, d.valid, f0, FT, tid, [&](int dc, int* step) -> const float* {
    const int m = fbank_column_band(dc, P.n_mels, P.use_energy, P.htk_compat);
    *step = m < 0 ? PS : 1;
    return m < 0 ? pw + Kp : mt + m * FTS;
  });
}

// a workgroup's (tile, channel, clip), its tile of `tile` frames and its row of the column sums
__device__ __forceinline__ void fbank_entry(const pdmp3_fbank_desc* __restrict__ descs, const float* __restrict__ dft, const float* __restrict__ fbt,
                                            float* __restrict__ sums, const pdmp3_fbank_params& P, int tile, float* lds) {
  const pdmp3_fbank_desc d = descs[blockIdx.y];
  const int ch = blockIdx.x % P.channels;
  const unsigned t = blockIdx.x / P.channels, tiles = gridDim.x / P.channels;
  const long long f0 = (long long)t * tile;
  if (f0 >= P.n_frames) return;
  float* const ts = sums_at(sums, P.channels, P.n_mels + P.use_energy, blockIdx.y, ch, t, tiles);
  if (tile == 32) fbank_tile<2>(d, dft, fbt, P, ch, f0, ts, lds);
  else fbank_tile<1>(d, dft, fbt, P, ch, f0, ts, lds);
}

__global__ __launch_bounds__(kMelThreads) void k_clip_fbank(const pdmp3_fbank_desc* __restrict__ descs, const float* __restrict__ dft,
                                                            const float* __restrict__ fbt, float* __restrict__ sums, pdmp3_fbank_params P) {
  extern __shared__ __align__(16) float lds[];
  fbank_entry(descs, dft, fbt, sums, P, P.tile, lds);
}

// A tile of 16 frames that needs more than the 64 KB a launch can ask for dynamically (Nw = 1024 at hops above 450): the same
// code on a static array of all the LDS a workgroup may have, one workgroup a CU (as k_clip_mel_big).
__global__ __launch_bounds__(kMelThreads) void k_clip_fbank_big(const pdmp3_fbank_desc* __restrict__ descs, const float* __restrict__ dft,
                                                                const float* __restrict__ fbt, float* __restrict__ sums, pdmp3_fbank_params P) {
  __shared__ __align__(16) float lds[PDMP3_MEL_LDS_MAX / sizeof(float)];
  fbank_entry(descs, dft, fbt, sums, P, 16, lds);
}

// subtract_mean, behind k_clip_fbank (tile_sums_finish)
__global__ __launch_bounds__(kMelThreads) void k_clip_fbank_finish(const pdmp3_fbank_desc* __restrict__ descs, const float* __restrict__ sums,
                                                                   unsigned tiles, pdmp3_fbank_params P) {
  tile_sums_finish(descs, sums, tiles, P.n_mels + P.use_energy, P.channels, P.n_frames);
}

}  // namespace

hipError_t pdmp3_launch_clip_fbank(hipStream_t s, const pdmp3_fbank_desc* descs, int n_clips, const float* dft, const float* fbt, float* sums,
                                   const pdmp3_fbank_params* params) {
  const pdmp3_fbank_params P = *params;
  if (n_clips <= 0 || P.n_frames <= 0) return hipSuccess;
  if (P.lds_bytes > PDMP3_MEL_LDS_SOFT && (P.tile != 16 || P.lds_bytes > PDMP3_MEL_LDS_MAX)) return hipErrorInvalidValue;
  const hipError_t e = pdmp3::launch_clip_pair(k_clip_fbank, k_clip_fbank_big, s, pdmp3::kMelThreads, P.n_frames, P.tile, P.channels, n_clips,
                                               P.lds_bytes, descs, dft, fbt, sums, P);
  if (e != hipSuccess || !P.subtract_mean) return e;
  const long long per = (long long)(P.n_mels + P.use_energy) * P.n_frames;
  long long blocks = (per + 16 * pdmp3::kMelThreads - 1) / (16 * pdmp3::kMelThreads);
  if (blocks > 256) blocks = 256;
  hipLaunchKernelGGL(k_clip_fbank_finish, dim3((unsigned)blocks, (unsigned)n_clips), dim3(pdmp3::kMelThreads), 0, s, descs, sums,
                     pdmp3::clip_tiles(P.n_frames, P.tile), P);
  return hipGetLastError();
}
