// mfcc.hip -- k_clip_mfcc: rows of the resampled signal of a batch of clips (k_clip_audio's output in the stream object's
// third audio stage) to Kaldi-style MFCC features, planar float32 [n_frames][n_ceps] per clip and channel, cepstra innermost
// (include/pdmp3_bulk.h pdmp3_amd_bulk_decode_clips_mfcc).  Launched by stream.hip pdmp3_hip_clip_mfcc.
// A translation unit of its own, so that every other kernel's code is what it is without it; stages 1 .. 4 are
// k_clip_fbank's (fbank.hip), restated here rather than shared through a header for the same reason; the indexing and
// pointwise arithmetic are mel_core.h's, fbank_core.h's and mfcc_core.h's.
#include <hip/hip_runtime.h>

#include "../../include/pdmp3_hip.h"
#include "mfcc_core.h"

namespace {

using namespace pdmp3;

typedef float f32x4 __attribute__((ext_vector_type(4)));
// v_mfma_f32_16x16x4_f32: lane l = (j = l & 15, kq = l >> 4) holds A[row j][k = kq], B[k = kq][col j] and
// D[row 4 kq + r][col j], r = 0..3; each D element is a fused multiply-add chain over k = 0..3 on top of C
__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
// every lane of the wave gets the sum of the 64 values, added pairwise in one fixed order
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = kFbankWave / 2; off; off >>= 1) v = v + __shfl_xor(v, off, kFbankWave);
  return v;
}

// One workgroup of four waves per (tile of P.fb.tile = 16 RT frames, channel, clip).
//   1. the tile's span -- (tile - 1) hop + rows samples from the clip's row, zeros behind it -- goes to LDS once (mel_lds_at);
//   2. energy (use_energy): a wave per frame, the mean and then sum (s - mean)^2 in a fixed lane and shuffle order; a frame's
//      value does not depend on its place.  It waits in the spare float behind the frame's row of powers;
//   3. DFT: the frames are overlapping rows of the span; the B operand is the folded table from memory.  Re^2 + Im^2 goes to
//      LDS [frame][bin];
//   4. filterbank: A = the powers, B = the transposed padded filterbank from memory; the mel tile goes to LDS [band][frames + 1]
//      over the span, which nobody reads any more;
//   5. L = ln max(M, eps) in place, every band of the mels16 and every frame of the tile.  The padded bands hold M = 0 (the
//      filterbank's padding is zeros), so L = ln eps there: finite, and it meets the zero rows of the folded DCT table, so the
//      products are +-0 and nothing of it reaches a cepstrum.  The powers are through: lane fl < tile takes frame fl's energy out
//      of their rows into a register in front of this stage's barrier;
//   6. DCT: A = L read as frames x bands (lane (j, kq) reads band k + kq of frame 16 rt + j: consecutive lanes, consecutive
//      floats), B = the folded table [mels16][ceps16] from memory (lifter, htk_compat's sqrt 2 and the column order in it, zeros
//      in the energy's column), k ascending over the mels16; a wave takes every fourth of the RT ceps16 / 16 output tiles.  The
//      cepstra go to LDS [frame][ceps16 + 1] where the powers were; behind the barrier the energy comes out of its register
//      into the spare float behind its frame's cepstra, which the matrix stage does not write;
//   7. stores: consecutive lanes write consecutive cepstra of one frame; the energy's value goes into its column (0, or
//      n_ceps - 1 with htk_compat), where the table gave 0.0;
//   8. subtract_mean: the energy column's stored value goes back to LDS in stage 7, and a lane per column adds those of the
//      frames f < valid, in frame order, into the tile's row of `tile_sums`; k_clip_mfcc_finish does the rest.
template <int RT>
__device__ __forceinline__ void mfcc_tile(const pdmp3_fbank_desc& d, const float* __restrict__ dft, const float* __restrict__ fbt,
                                          const float* __restrict__ dct, const pdmp3_mfcc_params& Q, int ch, long long f0,
                                          float* __restrict__ tile_sums, float* lds) {
  const pdmp3_fbank_params& P = Q.fb;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 15, kq = lane >> 4;
  const unsigned hop = (unsigned)P.hop, pad = (unsigned)P.row_pad, chunk = hop + pad;
  const int Kp = P.bins16, Mp = P.mels16, Cp = Q.ceps16, PS = Kp + 2, CS = mfcc_ceps_stride(Cp), FT = 16 * RT, FTS = FT + 1;
  float* const span = lds;
  float* const pw = lds + P.span_floats;
  const float* const row = reinterpret_cast<const float*>(static_cast<uintptr_t>(d.src)) + (size_t)ch * d.src_chan_stride;

  const unsigned n_span = (unsigned)(FT - 1) * hop + (unsigned)P.rows;
  for (unsigned p = tid; p < n_span; p += kMelThreads) span[mel_lds_at(p, hop, pad)] = mel_sample(row, P.n_in, f0, P.hop, 0u, p);
  __syncthreads();

  if (P.use_energy) {
    for (int fl = wave; fl < FT; fl += 4) {
      const unsigned p0 = (unsigned)fl * hop;
      float mean = 0.0f;
      if (P.remove_dc) mean = fbank_mean(wave_sum(fbank_lane_sum(span, p0, P.win, hop, pad, P.scale, lane)), P.win);
      const float e = wave_sum(fbank_lane_squares(span, p0, P.win, hop, pad, P.scale, mean, lane));
      if (lane == 0) pw[fl * PS + Kp] = e;
    }
  }

  const int ld = 2 * Kp;
  for (int bt = wave; bt < (Kp >> 4); bt += 4) {
    f32x4 re[RT], im[RT];
#pragma unroll
    for (int rt = 0; rt < RT; rt++) { re[rt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f}; im[rt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f}; }
    // lane (j, kq) reads frame j's sample n + kq: position j hop + n + kq = c hop + rem
    unsigned c = (unsigned)j + (unsigned)kq / hop, rem = (unsigned)kq % hop;
    const float* bp = dft + (size_t)kq * ld + (bt << 4) + j;
#pragma unroll 2
    for (int n = 0; n < P.rows; n += 4) {
      const float b_re = bp[0], b_im = bp[Kp];
      bp += 4 * ld;
      const float* ap = span + c * chunk + rem;
#pragma unroll
      for (int rt = 0; rt < RT; rt++) {
        const float a = ap[(unsigned)(16 * rt) * chunk];
        re[rt] = mfma16(a, b_re, re[rt]);
        im[rt] = mfma16(a, b_im, im[rt]);
      }
      rem += 4;
      if (rem >= hop) {
        if (hop >= 4) { rem -= hop; c++; }
        else { c += rem / hop; rem %= hop; }
      }
    }
#pragma unroll
    for (int rt = 0; rt < RT; rt++)
#pragma unroll
      for (int r = 0; r < 4; r++) pw[(16 * rt + 4 * kq + r) * PS + (bt << 4) + j] = mel_power(re[rt][r], im[rt][r]);
  }
  __syncthreads();

  float* const mt = lds;                               // [Mp][FTS]
  for (int t = wave; t < RT * (Mp >> 4); t += 4) {
    const int rt = t % RT, m0 = (t / RT) << 4;
    f32x4 acc = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const float* ap = pw + (16 * rt + j) * PS + kq;
    const float* bp = fbt + (size_t)kq * Mp + m0 + j;
#pragma unroll 4
    for (int k = 0; k < Kp; k += 4) acc = mfma16(ap[k], bp[(size_t)k * Mp], acc);
#pragma unroll
    for (int r = 0; r < 4; r++) mt[(m0 + j) * FTS + 16 * rt + 4 * kq + r] = acc[r];
  }
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
  long long cnt = (long long)d.valid - f0;             // (valid <= n_frames)
  cnt = cnt < 0 ? 0 : cnt > FT ? FT : cnt;
  for (int dc = tid; dc < D; dc += kMelThreads) {
    float s = 0.0f;
    for (int fl = 0; fl < (int)cnt; fl++) s = s + ct[fl * CS + dc];
    tile_sums[dc] = s;
  }
}

// the place of a (clip, channel, tile)'s column sums in the launch's scratch
__device__ __forceinline__ float* sums_at(float* sums, const pdmp3_mfcc_params& Q, unsigned clip, int ch, unsigned tile, unsigned tiles) {
  return sums + (((size_t)clip * (size_t)Q.fb.channels + (size_t)ch) * tiles + tile) * (size_t)Q.n_ceps;
}

__global__ __launch_bounds__(kMelThreads) void k_clip_mfcc(const pdmp3_fbank_desc* __restrict__ descs, const float* __restrict__ dft,
                                                           const float* __restrict__ fbt, const float* __restrict__ dct,
                                                           float* __restrict__ sums, pdmp3_mfcc_params Q) {
  extern __shared__ __align__(16) float lds[];
  const pdmp3_fbank_desc d = descs[blockIdx.y];
  const int ch = blockIdx.x % Q.fb.channels;
  const unsigned t = blockIdx.x / Q.fb.channels, tiles = gridDim.x / Q.fb.channels;
  const long long f0 = (long long)t * Q.fb.tile;
  if (f0 >= Q.fb.n_frames) return;
  float* const ts = sums_at(sums, Q, blockIdx.y, ch, t, tiles);
  if (Q.fb.tile == 32) mfcc_tile<2>(d, dft, fbt, dct, Q, ch, f0, ts, lds);
  else mfcc_tile<1>(d, dft, fbt, dct, Q, ch, f0, ts, lds);
}

// A tile of 16 frames that needs more than the 64 KB a launch can ask for dynamically: the same code on a static array of all
// the LDS a workgroup may have, one workgroup a CU (as k_clip_fbank_big).
__global__ __launch_bounds__(kMelThreads) void k_clip_mfcc_big(const pdmp3_fbank_desc* __restrict__ descs, const float* __restrict__ dft,
                                                               const float* __restrict__ fbt, const float* __restrict__ dct,
                                                               float* __restrict__ sums, pdmp3_mfcc_params Q) {
  __shared__ __align__(16) float lds[PDMP3_MEL_LDS_MAX / sizeof(float)];
  const pdmp3_fbank_desc d = descs[blockIdx.y];
  const int ch = blockIdx.x % Q.fb.channels;
  const unsigned t = blockIdx.x / Q.fb.channels, tiles = gridDim.x / Q.fb.channels;
  const long long f0 = (long long)t * 16;
  if (f0 >= Q.fb.n_frames) return;
  mfcc_tile<1>(d, dft, fbt, dct, Q, ch, f0, sums_at(sums, Q, blockIdx.y, ch, t, tiles), lds);
}

// subtract_mean, behind k_clip_mfcc: every column's tile sums added in ascending order, divided by valid, and the mean
// subtracted from every frame of the row.  No atomics: the result does not depend on the order the workgroups ran in.
__global__ __launch_bounds__(kMelThreads) void k_clip_mfcc_finish(const pdmp3_fbank_desc* __restrict__ descs, const float* __restrict__ sums,
                                                                  unsigned tiles, pdmp3_mfcc_params Q) {
  __shared__ float mean[256 + 1];
  const pdmp3_fbank_desc d = descs[blockIdx.y];
  if (!d.valid) return;
  const int D = Q.n_ceps, channels = Q.fb.channels;
  const long long per = (long long)D * Q.fb.n_frames;
  for (int ch = 0; ch < channels; ch++) {
    const float* const ts = sums + ((size_t)blockIdx.y * (size_t)channels + (size_t)ch) * tiles * (size_t)D;
    for (int dc = threadIdx.x; dc < D; dc += kMelThreads) {
      float s = 0.0f;
      for (unsigned t = 0; t < tiles; t++) s = s + ts[(size_t)t * D + dc];
      mean[dc] = fbank_column_mean(s, d.valid);
    }
    __syncthreads();
    float* const out = reinterpret_cast<float*>(static_cast<uintptr_t>(d.dst)) + (size_t)ch * d.dst_chan_stride;
    for (long long i = (long long)blockIdx.x * kMelThreads + threadIdx.x; i < per; i += (long long)gridDim.x * kMelThreads)
      out[i] = out[i] - mean[(int)(i % D)];
    __syncthreads();
  }
}

}  // namespace

hipError_t pdmp3_launch_clip_mfcc(hipStream_t s, const pdmp3_fbank_desc* descs, int n_clips, const float* dft, const float* fbt, const float* dct,
                                  float* sums, const pdmp3_mfcc_params* params) {
  const pdmp3_mfcc_params Q = *params;
  if (n_clips <= 0 || Q.fb.n_frames <= 0) return hipSuccess;
  const unsigned tiles = (unsigned)((Q.fb.n_frames + Q.fb.tile - 1) / Q.fb.tile);
  const dim3 grid(tiles * (unsigned)Q.fb.channels, (unsigned)n_clips);
  if (Q.fb.lds_bytes > PDMP3_MEL_LDS_SOFT) {
    if (Q.fb.tile != 16 || Q.fb.lds_bytes > PDMP3_MEL_LDS_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_clip_mfcc_big, grid, dim3(pdmp3::kMelThreads), 0, s, descs, dft, fbt, dct, sums, Q);
  } else {
    hipLaunchKernelGGL(k_clip_mfcc, grid, dim3(pdmp3::kMelThreads), Q.fb.lds_bytes, s, descs, dft, fbt, dct, sums, Q);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !Q.fb.subtract_mean) return e;
  const long long per = (long long)Q.n_ceps * Q.fb.n_frames;
  long long blocks = (per + 16 * pdmp3::kMelThreads - 1) / (16 * pdmp3::kMelThreads);
  if (blocks > 256) blocks = 256;
  hipLaunchKernelGGL(k_clip_mfcc_finish, dim3((unsigned)blocks, (unsigned)n_clips), dim3(pdmp3::kMelThreads), 0, s, descs, sums, tiles, Q);
  return hipGetLastError();
}
