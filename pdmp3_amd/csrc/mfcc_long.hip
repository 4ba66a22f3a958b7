// mfcc_long.hip -- k_clip_db_max, k_clip_mfcc_long, k_clip_db: librosa-style MFCC with deltas, and the dB mel with top_db, of
// clips (include/pdmp3_bulk.h pdmp3_amd_bulk_decode_clips_mfcc_long).  They read the log10 mel
// k_clip_mel_long wrote into a stage of the stream object and write the caller's rows.  The values, the LDS planes and the
// stencil are mfcc_long_core.h's, one source with the host build of the tests.  Launched by stream.hip
// pdmp3_hip_clip_mfcc_long.  A translation unit of its own.
#include <hip/hip_runtime.h>

#include "../../include/pdmp3_hip.h"
#include "clip_tile.h"
#include "mfcc_long_core.h"

namespace {

using namespace pdmp3;

__device__ __forceinline__ const float* stage_of(const pdmp3_mel_desc& d, int ch) {
  return reinterpret_cast<const float*>(static_cast<uintptr_t>(d.src)) + (size_t)ch * d.src_chan_stride;
}
// the plane's threshold: one float per channel behind the last channel's log-mel
__device__ __forceinline__ float* thr_of(const pdmp3_mel_desc& d, int channels, int ch) {
  return reinterpret_cast<float*>(static_cast<uintptr_t>(d.src)) + (size_t)channels * d.src_chan_stride + ch;
}

// One workgroup of sixteen waves per (channel, clip): the maximum of fl32(10 l) over all bands and the clip's own frames --
// the halo's columns are skipped --, then the threshold.  A wave takes the bands w, w + 16, .., its lanes consecutive frames.
// A maximum is exact in any order: shuffles inside a wave, LDS between the waves, no atomics.
__global__ __launch_bounds__(kDbMaxThreads) void k_clip_db_max(const pdmp3_mel_desc* __restrict__ descs, pdmp3_mfcc_long_params P) {
  __shared__ float wm[kDbMaxThreads / 64];
  const pdmp3_mel_desc d = descs[blockIdx.y];
  const int ch = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const float* const stage = stage_of(d, ch) + P.halo;
  float mx = -INFINITY;
  for (int m = wave; m < P.n_mels; m += kDbMaxThreads / 64) {
    const float* const row = stage + (size_t)m * (size_t)P.n_stage;
#pragma unroll 4
    for (int t = lane; t < P.n_frames; t += 64) mx = fmaxf(mx, mfcc_long_db(row[t]));
  }
#pragma unroll
  for (int off = 32; off; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
  if (lane == 0) wm[wave] = mx;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kDbMaxThreads / 64; w++) mx = fmaxf(mx, wm[w]);
    *thr_of(d, P.channels, ch) = mfcc_long_threshold(mx, P.top_db);
  }
}

// STEPS matrix instructions, bands k0 .. k0 + 4 STEPS - 1 ascending: T's values come from memory, all of them asked for before
// the first instruction needs one, so their latency is paid once a turn
template <int STEPS>
__device__ __forceinline__ void mfcc_long_steps(const float* __restrict__ ap, const float* lds, int k0, int kq, int col0, int j, f32x4& acc) {
  float a[STEPS];
#pragma unroll
  for (int i = 0; i < STEPS; i++) a[i] = ap[4 * i];
#pragma unroll
  for (int i = 0; i < STEPS; i++) acc = mfma16(a[i], lds[mfcc_long_b_at(k0 + 4 * i, kq, col0, j)], acc);
}

// One workgroup of four waves per (tile of 64 frames, channel, clip).
//   1. the tile with its halo -- stage frames f0 .. f0 + 64 + 2 h - 1, rounded up to whole column tiles of 16 -- goes to the D
//      plane as dB values, clamped: wave w takes the bands w, w + 4, .., its lanes consecutive frames; the padded bands and
//      the frames behind the stage become zeros;
//   2. c = T d on v_mfma_f32_16x16x4_f32: a wave takes every fourth (16 cepstra x 16 columns) tile; A = T's fragment from
//      memory (lane (j, kq): T[q0 + j][k + kq]), B = d's from LDS (band k + kq, column col0 + j), k ascending over the mels16:
//      a column's cepstrum is the same chain wherever the column lies in the tile.  The result goes to the C plane;
//   3. wave w takes the cepstra w, w + 4, .., lane l frame f0 + l: c and both stencils from the C plane, the stores --
//      consecutive lanes store consecutive frames.
// Two barriers.  Frames from F on are not stored.
__device__ __forceinline__ void mfcc_long_tile(const pdmp3_mel_desc& d, const float* __restrict__ dct, const pdmp3_mfcc_long_params& P, float* lds) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 15, kq = lane >> 4;
  const int ch = (int)(blockIdx.x % (unsigned)P.channels);
  const long long f0 = (long long)(blockIdx.x / (unsigned)P.channels) * kMfccLongFrames;
  if (f0 >= P.n_frames) return;
  const float* const stage = stage_of(d, ch);
  float* const out = reinterpret_cast<float*>(static_cast<uintptr_t>(d.dst)) + (size_t)ch * d.dst_chan_stride;
  const float thr = P.use_top ? *thr_of(d, P.channels, ch) : -INFINITY;
  const int Mp = P.mels16, cols = mfcc_long_cols16(P.halo);

  for (int m = wave; m < Mp; m += kMfccLongThreads / 64)
    for (int c = lane; c < cols; c += 64) lds[mfcc_long_d_at(m, c)] = mfcc_long_load(stage, P, f0, m, c, thr);
  __syncthreads();

  const int nct = cols >> 4;
  for (int t = wave; t < nct * (P.ceps16 >> 4); t += kMfccLongThreads / 64) {
    const int col0 = (t % nct) << 4, q0 = (t / nct) << 4;
    f32x4 acc = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const float* const ap = dct + (size_t)(q0 + j) * (size_t)Mp + kq;
    // mels16 is a multiple of 16: turns of 64 bands, then of 16; the order of the bands is the same either way
    int k0 = 0;
    for (; k0 + 64 <= Mp; k0 += 64) mfcc_long_steps<16>(ap + k0, lds, k0, kq, col0, j, acc);
    for (; k0 < Mp; k0 += 16) mfcc_long_steps<4>(ap + k0, lds, k0, kq, col0, j, acc);
#pragma unroll
    for (int r = 0; r < 4; r++) lds[mfcc_long_result_at(Mp, q0, kq, r, col0, j)] = acc[r];
  }
  __syncthreads();

  for (int q = wave; q < P.n_mfcc; q += kMfccLongThreads / 64) mfcc_long_store(lds + mfcc_long_c_at(Mp, q, 0), out, P, q, lane, f0 + lane);
}

__global__ __launch_bounds__(kMfccLongThreads) void k_clip_mfcc_long(const pdmp3_mel_desc* __restrict__ descs, const float* __restrict__ dct,
                                                                     pdmp3_mfcc_long_params P) {
  extern __shared__ __align__(16) float lds[];
  mfcc_long_tile(descs[blockIdx.y], dct, P, lds);
}
// the planes of many bands or cepstra need more than the 64 KB a launch can ask for dynamically: the same code on a static
// array of all the LDS a workgroup may have (as k_clip_mel_big)
__global__ __launch_bounds__(kMfccLongThreads) void k_clip_mfcc_long_big(const pdmp3_mel_desc* __restrict__ descs, const float* __restrict__ dct,
                                                                         pdmp3_mfcc_long_params P) {
  __shared__ __align__(16) float lds[PDMP3_MEL_LDS_MAX / sizeof(float)];
  mfcc_long_tile(descs[blockIdx.y], dct, P, lds);
}

// out_mode 1: d itself.  No halo, so a channel's plane is n_mels F consecutive floats in the stage and in the destination; a
// workgroup takes 1024 of them, a lane four, 256 apart.
__global__ __launch_bounds__(kMfccLongThreads) void k_clip_db(const pdmp3_mel_desc* __restrict__ descs, pdmp3_mfcc_long_params P) {
  const pdmp3_mel_desc d = descs[blockIdx.y];
  const int ch = (int)(blockIdx.x % (unsigned)P.channels);
  const unsigned total = (unsigned)P.n_mels * (unsigned)P.n_frames;
  const unsigned base = (blockIdx.x / (unsigned)P.channels) * (unsigned)kDbElems;
  const float* const stage = stage_of(d, ch);
  float* const out = reinterpret_cast<float*>(static_cast<uintptr_t>(d.dst)) + (size_t)ch * d.dst_chan_stride;
  const float thr = P.use_top ? *thr_of(d, P.channels, ch) : -INFINITY;
#pragma unroll
  for (int r = 0; r < kDbElems / kMfccLongThreads; r++) {
    const unsigned i = base + (unsigned)r * kMfccLongThreads + threadIdx.x;
    if (i < total) out[i] = mfcc_long_clamp(mfcc_long_db(stage[i]), thr);
  }
}

}  // namespace

hipError_t pdmp3_launch_clip_mfcc_long(hipStream_t s, const pdmp3_mel_desc* descs, int n_clips, const float* dct,
                                       const pdmp3_mfcc_long_params* params) {
  const pdmp3_mfcc_long_params P = *params;
  if (n_clips <= 0 || P.n_frames <= 0) return hipSuccess;
  if (P.use_top) {
    hipLaunchKernelGGL(k_clip_db_max, dim3((unsigned)P.channels, (unsigned)n_clips), dim3(pdmp3::kDbMaxThreads), 0, s, descs, P);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  if (P.out_mode == 1) {
    const unsigned blocks = (unsigned)(((long long)P.n_mels * P.n_frames + pdmp3::kDbElems - 1) / pdmp3::kDbElems);
    hipLaunchKernelGGL(k_clip_db, dim3(blocks * (unsigned)P.channels, (unsigned)n_clips), dim3(pdmp3::kMfccLongThreads), 0, s, descs, P);
    return hipGetLastError();
  }
  if (P.tile != pdmp3::kMfccLongFrames || P.d_pitch != pdmp3::kMfccLongDPitch || P.c_pitch != pdmp3::kMfccLongCPitch ||
      P.lds_bytes != pdmp3::mfcc_long_lds_floats(P.mels16, P.ceps16) * sizeof(float) || P.lds_bytes > PDMP3_MEL_LDS_MAX || !dct)
    return hipErrorInvalidValue;
  return pdmp3::launch_clip_pair(k_clip_mfcc_long, k_clip_mfcc_long_big, s, pdmp3::kMfccLongThreads, P.n_frames, P.tile, P.channels, n_clips,
                                 P.lds_bytes, descs, dct, P);
}
