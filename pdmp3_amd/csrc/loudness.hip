// loudness.hip -- the loudness of clips (include/pdmp3_bulk.h pdmp3_amd_bulk_decode_clips_loudness):
// rows of the resampled signal of a batch of clips (k_clip_audio's output in the stream object's third audio stage) through
// the K-weighting's two biquads as a blocked matrix product, the squares into sub-block sums of 100 ms, the gated mean of the
// 400 ms blocks, and the rows times the gain.  Launched by stream.hip pdmp3_hip_clip_loudness.  A translation unit of its own.
// The recurrence's states at the block starts are a binary64 scan (k_loud_states, k_loud_chain); the blocks themselves run on
// v_mfma_f32_16x16x4_f32 (k_loud_blocks).  Every sum has one fixed order and nothing is added atomically: two runs are
// bit-equal and a clip's numbers do not depend on the batch around it.  The arithmetic shared with the host build is
// loudness_core.h's.
#include <hip/hip_runtime.h>

#include "../../include/pdmp3_hip.h"
#include "cqt_rows.h"
#include "loudness_core.h"

namespace {

using namespace pdmp3;

struct LoudArgs {
  const pdmp3_mel_desc* descs;       // the grid's clips
  int clip0;                         // ... of which the first is the launch's clip0
  const pdmp3_loud_tables* tab;
  const uint64_t* stats_dst;         // per clip of the launch
  const uint64_t* mom_dst;
  double* states;                    // [row][n_chunks * 64][4]: after block b, from rest at its chunk's start
  double* starts;                    // [row][n_chunks][4]: k_loud_states the chunk's end from rest, k_loud_chain the state at its start
  float* part;                       // [row][n_chunks * 4][4]: a wave's three partial sums and its peak
  float* sub;                        // [row][n_sub]
  float* gains;                      // [clip]
  pdmp3_loud_params P;
};

__device__ __forceinline__ const float* loud_row(const pdmp3_mel_desc& d, int ch) {
  return reinterpret_cast<const float*>(static_cast<uintptr_t>(d.src)) + (size_t)ch * d.src_chan_stride;
}
// four samples from t on (t a multiple of 4; the row 16-byte aligned), zeros from T on
__device__ __forceinline__ float4 loud_load4(const float* row, long long T, long long t) {
  if (t + 4 <= T) return *reinterpret_cast<const float4*>(row + t);
  return float4{loud_sample(row, T, t), loud_sample(row, T, t + 1), loud_sample(row, T, t + 2), loud_sample(row, T, t + 3)};
}

// An inclusive scan over the wave's lanes of s_l = Phi^d s_(l - d) + s_l, d = 1, 2, .. 32 lanes: lane l ends with
// sum over m <= l of Phi^((l - m) n) e_m, n = 1 block (level 0) or 64 blocks (level 1)
template <bool kUnroll>
__device__ __forceinline__ void loud_scan(const pdmp3_loud_tables* tab, int level, int lane, double s[4]) {
  const auto step = [&](int k) {
    const int d = 1 << k;
    double v[4];
#pragma unroll
    for (int m = 0; m < 4; m++) v[m] = __shfl_up(s[m], d);
    if (lane >= d) loud_mat_acc(tab->pow[loud_pow_of(level, k)], v, s);
  };
  if (kUnroll) {
#pragma unroll
    for (int k = 0; k < 6; k++) step(k);
  } else {
#pragma unroll 1
    for (int k = 0; k < 6; k++) step(k);
  }
}

// One wave per (chunk, clip, channel): lane l takes block l of the chunk.
__global__ __launch_bounds__(64) void k_loud_states(LoudArgs a) {
  __shared__ float lds[kLoudChunk * kLoudRowS];
  const pdmp3_loud_params& P = a.P;
  const int lane = threadIdx.x, chunk = blockIdx.x;
  const pdmp3_mel_desc d = a.descs[blockIdx.y];
  const size_t row_i = (size_t)(a.clip0 + blockIdx.y) * P.channels + blockIdx.z;
  const float* const row = loud_row(d, blockIdx.z);
  const long long t0 = (long long)chunk * kLoudSpan;
#pragma unroll 4
  for (int it = 0; it < kLoudSpan / 256; it++) {
    const int idx = it * 256 + 4 * lane;
    const float4 v = loud_load4(row, P.n_in, t0 + idx);
    float* const p = lds + loud_at_s(idx >> 6, idx & 63);
    p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
  }
  __syncthreads();
  double s[4];
  loud_w(a.tab->R, lds + loud_at_s(lane, 0), s);
  loud_scan<true>(a.tab, 0, lane, s);
  double* const out = a.states + ((row_i * P.n_chunks + chunk) * kLoudChunk + lane) * 4;
#pragma unroll
  for (int m = 0; m < 4; m++) out[m] = s[m];
  if (lane == kLoudChunk - 1) {
    double* const e = a.starts + (row_i * P.n_chunks + chunk) * 4;
#pragma unroll
    for (int m = 0; m < 4; m++) e[m] = s[m];
  }
}

// One wave per (clip, channel): 64 chunks a step, the state behind them carried into the next step's first chunk.
__global__ __launch_bounds__(64) void k_loud_chain(LoudArgs a) {
  const pdmp3_loud_params& P = a.P;
  const int lane = threadIdx.x;
  const size_t row_i = (size_t)(a.clip0 + blockIdx.y) * P.channels + blockIdx.z;
  double* const e = a.starts + row_i * P.n_chunks * 4;
  double carry[4] = {0.0, 0.0, 0.0, 0.0};
  for (int c0 = 0; c0 < P.n_chunks; c0 += 64) {
    const int c = c0 + lane;
    double s[4];
#pragma unroll
    for (int m = 0; m < 4; m++) s[m] = c < P.n_chunks ? e[(size_t)c * 4 + m] : 0.0;
    if (lane == 0) loud_mat_acc(a.tab->pow[kLoudChunk], carry, s);
    loud_scan<false>(a.tab, 1, lane, s);
    double first[4];
#pragma unroll
    for (int m = 0; m < 4; m++) {
      first[m] = __shfl_up(s[m], 1);
      if (lane == 0) first[m] = carry[m];
      carry[m] = __shfl(s[m], 63);
    }
    if (c < P.n_chunks) {
#pragma unroll
      for (int m = 0; m < 4; m++) e[(size_t)c * 4 + m] = first[m];
    }
  }
}

// Four waves per (chunk, clip, channel): wave w takes blocks 16 w .. 16 w + 15 of the chunk -- it alone writes and reads
// their rows of LDS.  Y [64 samples x 16 blocks] = Hm U + O S_hi + O S_lo: for the four tiles of 16 samples, the steps of four
// columns of Hm up to the diagonal, then the two steps of the state.
__global__ __launch_bounds__(256) void k_loud_blocks(LoudArgs a) {
  __shared__ __align__(16) float lds[PDMP3_LOUD_LDS_BYTES / sizeof(float)];
  const pdmp3_loud_params& P = a.P;
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, j = lane & 15, kq = lane >> 4;
  const int chunk = blockIdx.x;
  const pdmp3_mel_desc d = a.descs[blockIdx.y];
  const size_t row_i = (size_t)(a.clip0 + blockIdx.y) * P.channels + blockIdx.z;
  const float* const row = loud_row(d, blockIdx.z);
  const long long tw = (long long)chunk * kLoudSpan + (long long)wave * kLoudWave;      // the wave's first sample

  float peak = 0.0f;
#pragma unroll
  for (int it = 0; it < kLoudWave / 256; it++) {
    const int idx = it * 256 + 4 * lane;                         // (of the wave's 1024 samples)
    const float4 v = loud_load4(row, P.n_in, tw + idx);
    peak = fmaxf(fmaxf(peak, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
    *reinterpret_cast<float4*>(lds + loud_at(16 * wave + (idx >> 6), idx & 63)) = v;
  }
  wave_sync();

  const int bl = 16 * wave + j;                                  // the lane's block of the chunk
  float u[16];
#pragma unroll
  for (int ks = 0; ks < 16; ks++) u[ks] = lds[loud_at(bl, 4 * ks + kq)];
  // the state at the block's start, component kq: Phi^bl times the chunk's, plus what the chunk's blocks before it left
  float hi, lo;
  {
    const double* const sc = a.starts + (row_i * P.n_chunks + chunk) * 4;
    const double v[4] = {sc[0], sc[1], sc[2], sc[3]};
    const double from_rest = bl ? a.states[((row_i * P.n_chunks + chunk) * kLoudChunk + bl - 1) * 4 + kq] : 0.0;
    loud_split(loud_row_acc(a.tab->pow[bl], kq, v, from_rest), &hi, &lo);
  }
  const float* const Hm = &a.tab->Hm[0][0];
  float h[16];                                                   // Hm[i][k] of a step, i - k = d + j - kq, d = -12, -8, .. 48
#pragma unroll
  for (int n = 0; n < 16; n++) h[n] = loud_hm(Hm, 4 * n - 12 + j - kq);

  float p[3] = {0.0f, 0.0f, 0.0f};
  const long long tb = tw + (long long)j * kLoudB;               // the block's first sample
  const long long ib = tb / P.q, edge = (ib + 1) * P.q;
  const int bin0 = (int)(ib - tw / P.q);
#pragma unroll
  for (int mt = 0; mt < 4; mt++) {
    f32x4 acc = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int ks = 0; ks < 4 * (mt + 1); ks++) acc = mfma16(h[4 * mt - ks + 3], u[ks], acc);
    const float o = a.tab->O[16 * mt + j][kq];
    acc = mfma16(o, hi, acc);
    acc = mfma16(o, lo, acc);
#pragma unroll
    for (int r = 0; r < 4; r++) loud_square(acc[r], tb + 16 * mt + 4 * kq + r, edge, bin0, p);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
    for (int n = 0; n < 3; n++) p[n] += __shfl_xor(p[n], off);
    peak = fmaxf(peak, __shfl_xor(peak, off));
  }
  if (lane == 0) {
    float* const out = a.part + ((row_i * P.n_chunks + chunk) * 4 + wave) * 4;
    out[0] = p[0]; out[1] = p[1]; out[2] = p[2]; out[3] = peak;
  }
}

// the sum or the maximum of the workgroup's 256 values in one fixed tree; every thread gets it
__device__ __forceinline__ double loud_reduce(double* red, double v, bool is_max) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int n = kLoudGateThreads / 2; n >= 1; n >>= 1) {
    if (tid < n) red[tid] = is_max ? fmax(red[tid], red[tid + n]) : red[tid] + red[tid + n];
    __syncthreads();
  }
  return red[0];
}

// One workgroup per clip.
__global__ __launch_bounds__(kLoudGateThreads) void k_loud_gate(LoudArgs a) {
  __shared__ double red[kLoudGateThreads];
  const pdmp3_loud_params& P = a.P;
  const int tid = threadIdx.x, C = P.channels;
  const size_t clip = (size_t)(a.clip0 + blockIdx.x);
  const float* const part = a.part + clip * C * P.n_chunks * 16;
  float* const sub = a.sub + clip * C * (size_t)P.n_sub;
  float* const stats = reinterpret_cast<float*>(static_cast<uintptr_t>(a.stats_dst[clip]));
  float* const mom = reinterpret_cast<float*>(static_cast<uintptr_t>(a.mom_dst[clip]));

  float pk = 0.0f;
  for (int c = 0; c < C; c++) {
    const float* const pc = part + (size_t)c * P.n_chunks * 16;
    for (long long i = tid; i < P.n_sub; i += kLoudGateThreads) sub[(size_t)c * P.n_sub + i] = loud_sub_sum(pc, i, P.q);
    for (long long w = tid; w < (long long)P.n_chunks * 4; w += kLoudGateThreads) pk = fmaxf(pk, pc[w * 4 + 3]);
  }
  const double peak = loud_reduce(red, (double)pk, true);        // (the barriers inside: the sub-block sums are there)

  double n_abs = 0.0, sum_abs = 0.0, top = -INFINITY;
  for (long long j = tid; j < P.n_mom; j += kLoudGateThreads) {
    const double z = loud_z(sub, P.n_sub, C, P.dual_mono, j, P.q), l = loud_l(z);
    if (mom) mom[j] = (float)l;
    top = fmax(top, l);
    if (l > -70.0) { n_abs += 1.0; sum_abs += z; }
  }
  n_abs = loud_reduce(red, n_abs, false);
  sum_abs = loud_reduce(red, sum_abs, false);
  top = loud_reduce(red, top, true);
  const double gamma = n_abs > 0.0 ? loud_l(sum_abs / n_abs) - 10.0 : -INFINITY;

  double n_rel = 0.0, sum_rel = 0.0;
  for (long long j = tid; j < P.n_mom; j += kLoudGateThreads) {
    const double z = loud_z(sub, P.n_sub, C, P.dual_mono, j, P.q), l = loud_l(z);
    if (l > -70.0 && l > gamma) { n_rel += 1.0; sum_rel += z; }
  }
  n_rel = loud_reduce(red, n_rel, false);
  sum_rel = loud_reduce(red, sum_rel, false);
  if (tid) return;
  const double L = n_rel > 0.0 ? loud_l(sum_rel / n_rel) : -INFINITY;
  const float g = loud_gain(L, peak, P.target, P.peak_limit);
  stats[0] = (float)L; stats[1] = (float)top; stats[2] = (float)peak; stats[3] = g;
  stats[4] = (float)gamma; stats[5] = (float)P.n_mom; stats[6] = (float)n_abs; stats[7] = (float)n_rel;
  a.gains[clip] = g;
}

// dst = x g: a workgroup per 1024 samples of a row
__global__ __launch_bounds__(256) void k_loud_scale(LoudArgs a) {
  const pdmp3_loud_params& P = a.P;
  const pdmp3_mel_desc d = a.descs[blockIdx.y];
  const float g = a.gains[a.clip0 + blockIdx.y];
  const float* const row = loud_row(d, blockIdx.z);
  float* const out = reinterpret_cast<float*>(static_cast<uintptr_t>(d.dst)) + (size_t)blockIdx.z * d.dst_chan_stride;
#pragma unroll
  for (int e = 0; e < 4; e++) {
    const long long t = (long long)blockIdx.x * 1024 + e * 256 + threadIdx.x;
    if (t < P.n_in) out[t] = row[t] * g;
  }
}

}  // namespace

hipError_t pdmp3_launch_clip_loudness(hipStream_t s, const pdmp3_mel_desc* descs, int n_clips, int clip0, const pdmp3_loud_tables* tab,
                                      const uint64_t* stats_dst, const uint64_t* mom_dst, double* states, double* starts, float* part, float* sub,
                                      float* gains, const pdmp3_loud_params* params) {
  const pdmp3_loud_params& P = *params;
  if (n_clips <= 0 || P.n_in <= 0) return hipSuccess;
  // a plan this file has no kernel for
  if (P.n_in > 0x7fffffffLL || (P.channels != 1 && P.channels != 2) || P.q < 800 || P.n_chunks != (P.n_in + kLoudSpan - 1) / kLoudSpan ||
      P.n_sub != P.n_in / P.q || P.n_mom != (P.n_sub > 3 ? P.n_sub - 3 : 0))
    return hipErrorInvalidValue;
  const LoudArgs a = {descs, clip0, tab, stats_dst, mom_dst, states, starts, part, sub, gains, P};
  const dim3 chunks((unsigned)P.n_chunks, (unsigned)n_clips, (unsigned)P.channels);
  hipLaunchKernelGGL(k_loud_states, chunks, dim3(64), 0, s, a);
  hipLaunchKernelGGL(k_loud_chain, dim3(1, (unsigned)n_clips, (unsigned)P.channels), dim3(64), 0, s, a);
  hipLaunchKernelGGL(k_loud_blocks, chunks, dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_loud_gate, dim3((unsigned)n_clips), dim3(kLoudGateThreads), 0, s, a);
  hipLaunchKernelGGL(k_loud_scale, dim3((unsigned)((P.n_in + 1023) / 1024), (unsigned)n_clips, (unsigned)P.channels), dim3(256), 0, s, a);
  return hipGetLastError();
}
