// mel.hip -- k_clip_mel: rows of the resampled signal of a batch of clips (k_clip_audio's output in the stream object's
// third audio stage) to log-mel features, planar float32 [n_mels][n_frames] per clip and channel
// (include/pdmp3_bulk.h pdmp3_amd_bulk_decode_clips_mel).  Launched by stream.hip pdmp3_hip_clip_mel.
// A translation unit of its own; the span's load and the two matrix stages are clip_tile.h's, one source for this kernel,
// k_clip_fbank and k_clip_mfcc (k_clip_stft has the first two), inlined here; the indexing and pointwise arithmetic are
// mel_core.h's.
#include <hip/hip_runtime.h>

#include "../../include/pdmp3_hip.h"
#include "clip_tile.h"

namespace {

using namespace pdmp3;

// One workgroup of four waves per (tile of P.tile = 16 RT frames, channel, clip).
//   1. the tile's span -- (tile - 1) hop + rows samples, zeros outside the clip's row -- goes to LDS once (mel_lds_at);
//   2. DFT (tile_dft_power): the frames are overlapping rows of the span, the A operand is read at f hop + n and never
//      materialised; the B operand is the table (window folded in), read from memory (L2: every workgroup reads the same
//      table).  A wave takes every fourth tile of 16 bins, Re and Im of all RT row tiles in registers; Re^2 + Im^2 goes to LDS
//      [frame][bin];
//   3. filterbank (tile_filterbank): A = the powers, B = the transposed padded filterbank from memory; the mel tile goes to LDS
//      [band][frame] over the span, which nobody reads any more;
//   4. floor, logarithm, stores: consecutive lanes write consecutive frames of one band.  Mode 3 stores M and takes the
//      row's maximum as an integer maximum of the floats' bits (M >= 0): one LDS atomic a lane, one global atomic a workgroup.
// Every frame's values come from the same chains of operations whatever its place in the tile.
template <int RT>
__device__ __forceinline__ void mel_tile(const pdmp3_mel_desc& d, const float* __restrict__ dft, const float* __restrict__ fbt,
                                         const pdmp3_mel_params& P, int ch, long long f0, unsigned* __restrict__ row_max, float* lds,
                                         unsigned* smax) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 15, kq = lane >> 4;
  const unsigned hop = (unsigned)P.hop, pad = (unsigned)P.row_pad, chunk = hop + pad;
  const int Kp = P.bins16, Mp = P.mels16, PS = Kp + 2, FT = 16 * RT, FTS = FT + 1;
  float* const span = lds;
  float* const pw = lds + P.span_floats;
  const float* const row = reinterpret_cast<const float*>(static_cast<uintptr_t>(d.src)) + (size_t)ch * d.src_chan_stride;

  span_load<kMelThreads>(span, row, P.n_in, f0, P.hop, pad, d.lead, (unsigned)(FT - 1) * hop + (unsigned)P.rows, tid);
  if (tid == 0) *smax = 0u;
  __syncthreads();

  tile_dft_power<RT>(span, dft, P.rows, Kp, hop, chunk, wave, j, kq, pw, PS);
  __syncthreads();

  float* const mt = lds;                               // [Mp][FTS]
  tile_filterbank<RT>(pw, PS, fbt, Kp, Mp, wave, j, kq, mt, FTS);
  __syncthreads();

  float* const out = reinterpret_cast<float*>(static_cast<uintptr_t>(d.dst)) + (size_t)ch * d.dst_chan_stride;
  uint32_t lmax = 0u;
  for (int i = tid; i < P.n_mels * FT; i += kMelThreads) {
    const int m = i / FT, fl = i % FT;
    const long long f = f0 + fl;
    if (f >= P.n_frames) continue;
    const float v = mt[m * FTS + fl];
    if (P.out_mode == 3) { const uint32_t u = mel_bits(v); lmax = u > lmax ? u : lmax; }
    out[(size_t)m * (size_t)P.n_frames + (size_t)f] = mel_output(v, P.floor, P.out_mode);
  }
  if (P.out_mode == 3) {
    atomicMax(smax, lmax);
    __syncthreads();
    if (tid == 0) atomicMax(row_max, *smax);
  }
}

// a workgroup's (tile, channel, clip) and its tile of `tile` frames
__device__ __forceinline__ void mel_entry(const pdmp3_mel_desc* __restrict__ descs, const float* __restrict__ dft, const float* __restrict__ fbt,
                                          unsigned* __restrict__ row_max, const pdmp3_mel_params& P, int tile, float* lds) {
  __shared__ unsigned smax;
  const pdmp3_mel_desc d = descs[blockIdx.y];
  const int ch = blockIdx.x % P.channels;
  const long long f0 = (long long)(blockIdx.x / P.channels) * tile;
  if (f0 >= P.n_frames) return;
  if (tile == 32) mel_tile<2>(d, dft, fbt, P, ch, f0, row_max + blockIdx.y, lds, &smax);
  else mel_tile<1>(d, dft, fbt, P, ch, f0, row_max + blockIdx.y, lds, &smax);
}

__global__ __launch_bounds__(kMelThreads) void k_clip_mel(const pdmp3_mel_desc* __restrict__ descs, const float* __restrict__ dft,
                                                          const float* __restrict__ fbt, unsigned* __restrict__ row_max, pdmp3_mel_params P) {
  extern __shared__ __align__(16) float lds[];
  mel_entry(descs, dft, fbt, row_max, P, P.tile, lds);
}

// A tile of 16 frames that needs more than the 64 KB a launch can ask for dynamically (n_fft = 1024 at hops above 450): the
// same code on a static array of all the LDS a workgroup may have, one workgroup a CU.
__global__ __launch_bounds__(kMelThreads) void k_clip_mel_big(const pdmp3_mel_desc* __restrict__ descs, const float* __restrict__ dft,
                                                              const float* __restrict__ fbt, unsigned* __restrict__ row_max, pdmp3_mel_params P) {
  __shared__ __align__(16) float lds[PDMP3_MEL_LDS_MAX / sizeof(float)];
  mel_entry(descs, dft, fbt, row_max, P, 16, lds);
}

// mode 3, behind k_clip_mel: every M of a row to (max(log10 max(M, floor), g - 8) + 4) / 4 with the row's maximum
__global__ __launch_bounds__(kMelThreads) void k_clip_mel_finish(const pdmp3_mel_desc* __restrict__ descs, const unsigned* __restrict__ row_max,
                                                                 pdmp3_mel_params P) {
  const pdmp3_mel_desc d = descs[blockIdx.y];
  const float top = mel_from_bits(row_max[blockIdx.y]);
  const long long per = (long long)P.n_mels * P.n_frames;
  for (int ch = 0; ch < P.channels; ch++) {
    float* const out = reinterpret_cast<float*>(static_cast<uintptr_t>(d.dst)) + (size_t)ch * d.dst_chan_stride;
    for (long long i = (long long)blockIdx.x * kMelThreads + threadIdx.x; i < per; i += (long long)gridDim.x * kMelThreads)
      out[i] = mel_whisper(out[i], top, P.floor);
  }
}

}  // namespace

hipError_t pdmp3_launch_clip_mel(hipStream_t s, const pdmp3_mel_desc* descs, int n_clips, const float* dft, const float* fbt, unsigned* row_max,
                                 const pdmp3_mel_params* params) {
  const pdmp3_mel_params P = *params;
  if (n_clips <= 0 || P.n_frames <= 0) return hipSuccess;
  if (P.lds_bytes > PDMP3_MEL_LDS_SOFT && (P.tile != 16 || P.lds_bytes > PDMP3_MEL_LDS_MAX)) return hipErrorInvalidValue;
  const hipError_t e = pdmp3::launch_clip_pair(k_clip_mel, k_clip_mel_big, s, pdmp3::kMelThreads, P.n_frames, P.tile, P.channels, n_clips,
                                               P.lds_bytes, descs, dft, fbt, row_max, P);
  if (e != hipSuccess || P.out_mode != 3) return e;
  const long long per = (long long)P.n_mels * P.n_frames;
  long long blocks = (per + pdmp3::kMelThreads - 1) / pdmp3::kMelThreads;
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(k_clip_mel_finish, dim3((unsigned)blocks, (unsigned)n_clips), dim3(pdmp3::kMelThreads), 0, s, descs, row_max, P);
  return hipGetLastError();
}
