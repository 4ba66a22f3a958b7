// mfcc.hip -- k_clip_mfcc: rows of the resampled signal of a batch of clips (k_clip_audio's output in the stream object's
// third audio stage) to Kaldi-style MFCC features, planar float32 [n_frames][n_ceps] per clip and channel, cepstra innermost
// (include/pdmp3_bulk.h pdmp3_amd_bulk_decode_clips_mfcc).  Launched by stream.hip pdmp3_hip_clip_mfcc.
// A translation unit of its own; stages 1 .. 4, the column sums and the finishing pass are k_clip_fbank's (fbank.hip): both
// files call clip_tile.h's, one source inlined here, so that the log-mel values under the DCT are k_clip_fbank's bit for bit
// by construction; the indexing and pointwise arithmetic are mel_core.h's, fbank_core.h's and mfcc_core.h's.
#include <hip/hip_runtime.h>

#include "../../include/pdmp3_hip.h"
#include "clip_tile.h"
#include "mfcc_core.h"

namespace {

using namespace pdmp3;

// One workgroup of four waves per (tile of P.fb.tile = 16 RT frames, channel, clip).
//   1. the tile's span -- (tile - 1) hop + rows samples from the clip's row, zeros behind it -- goes to LDS once (mel_lds_at);
//   2. energy (use_energy; tile_energy): a wave per frame, the mean and then sum (s - mean)^2 in a fixed lane and shuffle
//      order; a frame's value does not depend on its place.  It waits in the spare float behind the frame's row of powers;
//   3. DFT (tile_dft_power): the frames are overlapping rows of the span; the B operand is the folded table from memory.
//      Re^2 + Im^2 goes to LDS [frame][bin];
//   4. filterbank (tile_filterbank): A = the powers, B = the transposed padded filterbank from memory; the mel tile goes to LDS
//      [band][frames + 1] over the span, which nobody reads any more;
//   5. L = ln max(M, eps) in place, every band of the mels16 and every frame of the tile.  The padded bands hold M = 0 (the
//      filterbank's padding is zeros), so L = ln eps there: finite, and it meets the zero rows of the folded DCT table, so the
//      products are +-0 and nothing of it reaches a cepstrum.  The powers are through: lane fl < tile takes frame fl's energy
//      out of their rows into a register in front of this stage's barrier;
//   6. DCT: A = L read as frames x bands (lane (j, kq) reads band k + kq of frame 16 rt + j: consecutive lanes, consecutive
//      floats), B = the folded table [mels16][ceps16] from memory (lifter, htk_compat's sqrt 2 and the column order in it,
//      zeros in the energy's column), k ascending over the mels16; a wave takes every fourth of the RT ceps16 / 16 output
//      tiles.  The cepstra go to LDS [frame][ceps16 + 1] where the powers were; behind the barrier the energy comes out of its
//      register into the spare float behind its frame's cepstra, which the matrix stage does not write;
//   7. stores: consecutive lanes write consecutive cepstra of one frame; the energy's value goes into its column (0, or
//      n_ceps - 1 with htk_compat), where the table gave 0.0;
//   8. subtract_mean: the energy column's stored value goes back to LDS in stage 7, and a lane per column adds those of the
//      frames f < valid, in frame order, into the tile's row `ts` of the launch's scratch (tile_sums); k_clip_mfcc_finish does
//      the rest.
template <int RT>
__device__ __forceinline__ void mfcc_tile(const pdmp3_fbank_desc& d, const float* __restrict__ dft, const float* __restrict__ fbt,
                                          const float* __restrict__ dct, const pdmp3_mfcc_params& Q, int ch, long long f0,
                                          float* __restrict__ ts, float* lds) {
  const pdmp3_fbank_params& P = Q.fb;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 15, kq = lane >> 4;
  const unsigned hop = (unsigned)P.hop, pad = (unsigned)P.row_pad, chunk = hop + pad;
  const int Kp = P.bins16, Mp = P.mels16, Cp = Q.ceps16, PS = Kp + 2, CS = mfcc_ceps_stride(Cp), FT = 16 * RT, FTS = FT + 1;
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

  float energy = 0.0f;
  if (P.use_energy && tid < FT) energy = pw[tid * PS + Kp];
  for (int i = tid; i < Mp * FT; i += kMelThreads) {
    const int m = i / FT, fl = i - m * FT;
    mt[m * FTS + fl] = mel_output(mt[m * FTS + fl], P.eps, 1);
  }
  __syncthreads();

  float* const ct = pw;                                // [FT][CS]
  if (P.use_energy && tid < FT) ct[tid * CS + Cp] = energy;
  for (int t = wave; t < RT * (Cp >> 4); t += 4) {
    const int rt = t % RT, c0 = (t / RT) << 4;
    f32x4 acc = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const float* ap = mt + kq * FTS + 16 * rt + j;
    const float* bp = dct + (size_t)kq * Cp + c0 + j;
#pragma unroll 4
    for (int k = 0; k < Mp; k += 4) acc = mfma16(ap[k * FTS], bp[(size_t)k * Cp], acc);
#pragma unroll
    for (int r = 0; r < 4; r++) ct[(16 * rt + 4 * kq + r) * CS + c0 + j] = acc[r];
  }
  __syncthreads();

  float* const out = reinterpret_cast<float*>(static_cast<uintptr_t>(d.dst)) + (size_t)ch * d.dst_chan_stride;
  const int D = Q.n_ceps, ecol = mfcc_energy_column(D, P.use_energy, P.htk_compat);
  for (int i = tid; i < D * FT; i += kMelThreads) {
    const int fl = i / D, dc = i - fl * D;
    const long long f = f0 + fl;
    if (f >= P.n_frames) break;                        // (frames ascend with i)
    float* const cf = ct + fl * CS;
    const float v = mfcc_output(cf, Cp, dc, ecol, P.eps, P.energy_log_floor);
    if (P.subtract_mean && dc == ecol) cf[dc] = v;
    out[(size_t)f * (size_t)D + (size_t)dc] = v;
  }
  if (!P.subtract_mean) return;
  __syncthreads();
  tile_sums(ts, D, d.valid, f0, FT, tid, [&](int dc, int* step) -> const float* {
    *step = CS;
    return ct + dc;
  });
}

// a workgroup's (tile, channel, clip), its tile of `tile` frames and its row of the column sums
__device__ __forceinline__ void mfcc_entry(const pdmp3_fbank_desc* __restrict__ descs, const float* __restrict__ dft, const float* __restrict__ fbt,
                                           const float* __restrict__ dct, float* __restrict__ sums, const pdmp3_mfcc_params& Q, int tile,
                                           float* lds) {
  const pdmp3_fbank_desc d = descs[blockIdx.y];
  const int ch = blockIdx.x % Q.fb.channels;
  const unsigned t = blockIdx.x / Q.fb.channels, tiles = gridDim.x / Q.fb.channels;
  const long long f0 = (long long)t * tile;
  if (f0 >= Q.fb.n_frames) return;
  float* const ts = sums_at(sums, Q.fb.channels, Q.n_ceps, blockIdx.y, ch, t, tiles);
  if (tile == 32) mfcc_tile<2>(d, dft, fbt, dct, Q, ch, f0, ts, lds);
  else mfcc_tile<1>(d, dft, fbt, dct, Q, ch, f0, ts, lds);
}

__global__ __launch_bounds__(kMelThreads) void k_clip_mfcc(const pdmp3_fbank_desc* __restrict__ descs, const float* __restrict__ dft,
                                                           const float* __restrict__ fbt, const float* __restrict__ dct,
                                                           float* __restrict__ sums, pdmp3_mfcc_params Q) {
  extern __shared__ __align__(16) float lds[];
  mfcc_entry(descs, dft, fbt, dct, sums, Q, Q.fb.tile, lds);
}

// A tile of 16 frames that needs more than the 64 KB a launch can ask for dynamically: the same code on a static array of all
// the LDS a workgroup may have, one workgroup a CU (as k_clip_fbank_big).
__global__ __launch_bounds__(kMelThreads) void k_clip_mfcc_big(const pdmp3_fbank_desc* __restrict__ descs, const float* __restrict__ dft,
                                                               const float* __restrict__ fbt, const float* __restrict__ dct,
                                                               float* __restrict__ sums, pdmp3_mfcc_params Q) {
  __shared__ __align__(16) float lds[PDMP3_MEL_LDS_MAX / sizeof(float)];
  mfcc_entry(descs, dft, fbt, dct, sums, Q, 16, lds);
}

// subtract_mean, behind k_clip_mfcc (tile_sums_finish)
__global__ __launch_bounds__(kMelThreads) void k_clip_mfcc_finish(const pdmp3_fbank_desc* __restrict__ descs, const float* __restrict__ sums,
                                                                  unsigned tiles, pdmp3_mfcc_params Q) {
  tile_sums_finish(descs, sums, tiles, Q.n_ceps, Q.fb.channels, Q.fb.n_frames);
}

}  // namespace

hipError_t pdmp3_launch_clip_mfcc(hipStream_t s, const pdmp3_fbank_desc* descs, int n_clips, const float* dft, const float* fbt, const float* dct,
                                  float* sums, const pdmp3_mfcc_params* params) {
  const pdmp3_mfcc_params Q = *params;
  if (n_clips <= 0 || Q.fb.n_frames <= 0) return hipSuccess;
  if (Q.fb.lds_bytes > PDMP3_MEL_LDS_SOFT && (Q.fb.tile != 16 || Q.fb.lds_bytes > PDMP3_MEL_LDS_MAX)) return hipErrorInvalidValue;
  const hipError_t e = pdmp3::launch_clip_pair(k_clip_mfcc, k_clip_mfcc_big, s, pdmp3::kMelThreads, Q.fb.n_frames, Q.fb.tile, Q.fb.channels,
                                               n_clips, Q.fb.lds_bytes, descs, dft, fbt, dct, sums, Q);
  if (e != hipSuccess || !Q.fb.subtract_mean) return e;
  const long long per = (long long)Q.n_ceps * Q.fb.n_frames;
  long long blocks = (per + 16 * pdmp3::kMelThreads - 1) / (16 * pdmp3::kMelThreads);
  if (blocks > 256) blocks = 256;
  hipLaunchKernelGGL(k_clip_mfcc_finish, dim3((unsigned)blocks, (unsigned)n_clips), dim3(pdmp3::kMelThreads), 0, s, descs, sums,
                     pdmp3::clip_tiles(Q.fb.n_frames, Q.fb.tile), Q);
  return hipGetLastError();
}
