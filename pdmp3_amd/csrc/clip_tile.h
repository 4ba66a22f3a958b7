// clip_tile.h -- device code shared by the clip feature kernels (mel.hip, fbank.hip, mfcc.hip, stft.hip, stft_long.hip,
// mel_long.hip, cqt.hip, chroma.hip): the matrix instruction and the wave's primitives, the span's load, the overlapping-frames
// DFT, the filterbank product, the fbank family's energy stage, column sums and finishing pass, and the launch of a
// k_clip_X / k_clip_X_big pair.  One source, so that a stage is changed in one place and a value that two kernels both form
// (mfcc on fbank's stages) is the same binary32 number in both.  Every function is inlined into its caller: the translation
// units stay separate, and a helper takes the lane's coordinates (wave, j, kq) from its caller, it does not derive them again.
// HIP only; the indexing and the arithmetic that the host build shares are the *_core.h headers'.
#ifndef PDMP3_CLIP_TILE_H
#define PDMP3_CLIP_TILE_H
#include <hip/hip_runtime.h>

#include "fbank_core.h"

namespace pdmp3 {

typedef float f32x4 __attribute__((ext_vector_type(4)));
// a (Re, Im) pair of the output: one 8-byte store; a row may start at any float, and the device stores 8 bytes at 4-byte alignment
typedef float f32x2 __attribute__((ext_vector_type(2), aligned(4)));
// v_mfma_f32_16x16x4_f32: lane l = (j = l & 15, kq = l >> 4) holds A[row j][k = kq], B[k = kq][col j] and
// D[row 4 kq + r][col j], r = 0..3; each D element is a fused multiply-add chain over k = 0..3 on top of C
__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
// what a wave's lanes wrote to its staging tile or plane is there for its other lanes (LDS operations of a wave complete in order)
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// every lane of the wave gets the sum of the 64 values, added pairwise in one fixed order
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = kFbankWave / 2; off; off >>= 1) v = v + __shfl_xor(v, off, kFbankWave);
  return v;
}

// The tile's span -- n_span samples from frame f0's first on, zeros outside the clip's row -- to LDS, once: padded
// (mel_lds_at: row_pad floats between two hops' worth) ...
template <int THREADS>
__device__ __forceinline__ void span_load(float* span, const float* row, long long n_in, long long f0, int hop, unsigned pad, unsigned lead,
                                          unsigned n_span, int tid) {
  for (unsigned p = tid; p < n_span; p += THREADS) span[mel_lds_at(p, (unsigned)hop, pad)] = mel_sample(row, n_in, f0, hop, lead, p);
}
// ... or plain, as the long transform reads it
template <int THREADS>
__device__ __forceinline__ void span_load_plain(float* span, const float* row, long long n_in, long long f0, int hop, unsigned lead,
                                                unsigned n_span, int tid) {
  for (unsigned p = tid; p < n_span; p += THREADS) span[p] = mel_sample(row, n_in, f0, hop, lead, p);
}

// The DFT of 16 RT overlapping frames of the padded span on the matrix instruction, one tile bt of 16 bins.  The A operand is
// read at f hop + n and never materialised; the B operand is the table [rows][2 Kp] (Re of the Kp bins, then Im), read from
// memory (L2: every workgroup reads the same table).  Re and Im of all RT row tiles in registers, each a chain over n ascending
// from +0: lane (j, kq) holds bin 16 bt + j of frames 16 rt + 4 kq + r.  A wave takes every fourth tile: the loop over bt and
// what becomes of re, im are the caller's.  (With the loop inside and a sink for a parameter the compiler laid k_clip_stft's
// blocks out otherwise, and the kernel's time left the copies' range: profiles/clip_tile_ab.txt.)
template <int RT>
__device__ __forceinline__ void tile_dft(const float* span, const float* __restrict__ table, int rows, int Kp, unsigned hop, unsigned chunk,
                                         int bt, int j, int kq, f32x4 (&re)[RT], f32x4 (&im)[RT]) {
  const int ld = 2 * Kp;
#pragma unroll
  for (int rt = 0; rt < RT; rt++) { re[rt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f}; im[rt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f}; }
  // lane (j, kq) reads frame j's sample n + kq: position j hop + n + kq = c hop + rem
  unsigned c = (unsigned)j + (unsigned)kq / hop, rem = (unsigned)kq % hop;
  const float* bp = table + (size_t)kq * ld + (bt << 4) + j;
#pragma unroll 2
  for (int n = 0; n < rows; n += 4) {
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
}
// every fourth tile of bins of a wave through tile_dft, Re^2 + Im^2 to LDS [frame][bin], PS floats a frame
template <int RT>
__device__ __forceinline__ void tile_dft_power(const float* span, const float* __restrict__ table, int rows, int Kp, unsigned hop, unsigned chunk,
                                               int wave, int j, int kq, float* pw, int PS) {
  for (int bt = wave; bt < (Kp >> 4); bt += 4) {
    f32x4 re[RT], im[RT];
    tile_dft<RT>(span, table, rows, Kp, hop, chunk, bt, j, kq, re, im);
#pragma unroll
    for (int rt = 0; rt < RT; rt++)
#pragma unroll
      for (int r = 0; r < 4; r++) pw[(16 * rt + 4 * kq + r) * PS + (bt << 4) + j] = mel_power(re[rt][r], im[rt][r]);
  }
}

// The filterbank: A = the powers [frame][PS], B = the transposed padded filterbank [Kp][Mp] from memory, k ascending over the
// bins; a wave takes every fourth of the RT Mp / 16 output tiles.  The mel tile goes to LDS [band][FTS].
template <int RT>
__device__ __forceinline__ void tile_filterbank(const float* pw, int PS, const float* __restrict__ fbt, int Kp, int Mp, int wave, int j, int kq,
                                                float* mt, int FTS) {
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
}

// The fbank family's energy (use_energy): a wave per frame of the tile's FT, the mean and then sum (s - mean)^2 in a fixed lane
// and shuffle order; a frame's value does not depend on its place.  It waits in the spare float behind the frame's row of
// powers.
__device__ __forceinline__ void tile_energy(const float* span, const pdmp3_fbank_params& P, int FT, unsigned hop, unsigned pad, int wave, int lane,
                                            float* pw, int PS, int Kp) {
  if (!P.use_energy) return;
  for (int fl = wave; fl < FT; fl += 4) {
    const unsigned p0 = (unsigned)fl * hop;
    float mean = 0.0f;
    if (P.remove_dc) mean = fbank_mean(wave_sum(fbank_lane_sum(span, p0, P.win, hop, pad, P.scale, lane)), P.win);
    const float e = wave_sum(fbank_lane_squares(span, p0, P.win, hop, pad, P.scale, mean, lane));
    if (lane == 0) pw[fl * PS + Kp] = e;
  }
}

// the place of a (clip, channel, tile)'s D column sums in the launch's scratch
__device__ __forceinline__ float* sums_at(float* sums, int channels, int D, unsigned clip, int ch, unsigned tile, unsigned tiles) {
  return sums + (((size_t)clip * (size_t)channels + (size_t)ch) * tiles + tile) * (size_t)D;
}
// subtract_mean in the tile: a lane per column adds the column's values of the frames f < valid, in frame order, into the
// tile's row of the scratch.  col(dc, &step): the column's value of the tile's first frame in LDS, `step` floats a frame.
template <class Col>
__device__ __forceinline__ void tile_sums(float* __restrict__ ts, int D, unsigned valid, long long f0, int FT, int tid, Col col) {
  long long cnt = (long long)valid - f0;               // (valid <= n_frames)
  cnt = cnt < 0 ? 0 : cnt > FT ? FT : cnt;
  for (int dc = tid; dc < D; dc += kMelThreads) {
    int step;
    const float* const at = col(dc, &step);
    float s = 0.0f;
    for (int fl = 0; fl < (int)cnt; fl++) s = s + at[fl * step];
    ts[dc] = s;
  }
}
// subtract_mean, behind the tile kernel: every column's tile sums added in ascending order, divided by valid, and the mean
// subtracted from every frame of the row.  No atomics: the result does not depend on the order the workgroups ran in.
__device__ __forceinline__ void tile_sums_finish(const pdmp3_fbank_desc* __restrict__ descs, const float* __restrict__ sums, unsigned tiles, int D,
                                                 int channels, int n_frames) {
  __shared__ float mean[256 + 1];
  const pdmp3_fbank_desc d = descs[blockIdx.y];
  if (!d.valid) return;
  const long long per = (long long)D * n_frames;
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

// Host side.  The tiles of a row of n_frames frames ...
inline unsigned clip_tiles(long long n_frames, int tile) { return (unsigned)((n_frames + tile - 1) / tile); }
// ... and the launch of a k_clip_X / k_clip_X_big pair: a workgroup per (tile, channel, clip); up to PDMP3_MEL_LDS_SOFT the LDS
// is asked for with the launch, above it `big` has a static array of PDMP3_MEL_LDS_MAX bytes.  What a plan may ask of `big` its
// caller checks.
template <class Kernel, class... Args>
inline hipError_t launch_clip_pair(Kernel soft, Kernel big, hipStream_t s, int threads, long long n_frames, int tile, int channels, int n_clips,
                                   unsigned lds_bytes, Args... args) {
  const dim3 grid(clip_tiles(n_frames, tile) * (unsigned)channels, (unsigned)n_clips);
  if (lds_bytes > PDMP3_MEL_LDS_SOFT) hipLaunchKernelGGL(big, grid, dim3(threads), 0, s, args...);
  else hipLaunchKernelGGL(soft, grid, dim3(threads), lds_bytes, s, args...);
  return hipGetLastError();
}

}  // namespace pdmp3
#endif
