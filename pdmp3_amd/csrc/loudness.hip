// loudness.hip -- the loudness of clips (include/pdmp3_bulk.h pdmp3_amd_bulk_decode_clips_loudness):
// rows of the resampled signal of a batch of clips (k_clip_audio's output in the stream object's third audio stage) through
// the K-weighting's two biquads as a blocked matrix product, the squares into sub-block sums of 100 ms, the gated mean of the
// 400 ms blocks, and the rows times the gain.  Launched by stream.hip pdmp3_hip_clip_loudness.  A translation unit of its own.
// The recurrence's states at the block starts are a binary64 scan (k_loud_states, k_loud_chain); the blocks themselves run on
// v_mfma_f32_16x16x4_f32 (k_loud_blocks).  Every sum has one fixed order and nothing is added atomically: two runs are
// bit-equal and a clip's numbers do not depend on the batch around it.  The arithmetic shared with the host build is
// loudness_core.h's.  The true peak, the short-term loudness and the loudness range (pdmp3_amd_bulk_decode_clips_r128; DESIGN.md
// section 19) are the second instantiations of k_loud_blocks and k_loud_gate: the K-weighting stays one piece of code, the
// interpolator's three phases multiply the operands it already holds; their pointwise pieces are r128_core.h's.
#include <hip/hip_runtime.h>

#include "../../include/pdmp3_hip.h"
#include "cqt_rows.h"
#include "loudness_core.h"
#include "r128_core.h"

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
  float* part;                       // [row][n_chunks * 4][4]: a wave's three partial sums and its peak ([8] with the true peak: r128_core.h)
  float* sub;                        // [row][n_sub]
  float* gains;                      // [clip]
  pdmp3_loud_params P;
  // the true-peak call alone (k_loud_blocks<true>, k_loud_gate<true>)
  const float* taps;                 // [3][12]: c_p[d] of phases 1 .. 3
  const uint64_t* st_dst;            // per clip of the launch: its short-term values, or 0
  int n_st, n_rng, limit_tp;         // Js, Jr; the gain is held to TP
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
// kTruePeak: phases p = 1 .. 3 of the interpolator on the same B operands, Yp [64 samples x 16 blocks] = Tp U', Tp[i][k] =
// c_p[i - k] a band 12 wide: a tile of 16 samples takes the seven steps of four columns 16 mt - 12 .. 16 mt + 15, the columns
// below 0 being the last 12 samples of the block before -- the wave's own LDS rows but for its first block, whose lanes read
// them from the row in memory (zeros in front of the row).  max |Yp| over the samples t < T goes the peak's way.
template <bool kTruePeak>
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
  float tp = 0.0f;
  if constexpr (kTruePeak) {
    float v[3];                                                  // the block before: its samples 52 + 4 n + kq
#pragma unroll
    for (int n = 0; n < 3; n++)
      v[n] = j ? lds[loud_at(bl - 1, 52 + 4 * n + kq)] : r128_sample(row, P.n_in, tw - 12 + 4 * n + kq);
    const long long left = P.n_in - tb;                          // samples of the block inside the row
#pragma unroll
    for (int ph = 1; ph <= 3; ph++) {
      float c[kR128Steps];                                       // Tp[i][k] of a step, i - k = 4 (n - 3) + j - kq
#pragma unroll
      for (int n = 0; n < kR128Steps; n++) c[n] = r128_tap(a.taps, ph, 4 * (n - 3) + j - kq);
#pragma unroll
      for (int mt = 0; mt < 4; mt++) {
        f32x4 acc = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int s = 0; s < kR128Steps; s++) {
          const int ks = 4 * mt - 3 + s;
          acc = mfma16(c[6 - s], ks < 0 ? v[ks + 3] : u[ks], acc);
        }
#pragma unroll
        for (int r = 0; r < 4; r++) tp = 16 * mt + 4 * kq + r < left ? fmaxf(tp, fabsf(acc[r])) : tp;
      }
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
    for (int n = 0; n < 3; n++) p[n] += __shfl_xor(p[n], off);
    peak = fmaxf(peak, __shfl_xor(peak, off));
    if constexpr (kTruePeak) tp = fmaxf(tp, __shfl_xor(tp, off));
  }
  if (lane == 0) {
    float* const out = a.part + ((row_i * P.n_chunks + chunk) * 4 + wave) * (kTruePeak ? kR128Part : 4);
    out[0] = p[0]; out[1] = p[1]; out[2] = p[2]; out[3] = peak;
    if constexpr (kTruePeak) { out[4] = tp; out[5] = out[6] = out[7] = 0.0f; }
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
// kR128: besides the loudness call's numbers, TP from the waves' interpolated maxima, the windows of 30 sub-blocks S_j as the
// blocks of four, Smax, the range's two gates over the windows a second apart, and its two order statistics by counting: the
// gated S_j lie in LDS (+inf: not in the set), every thread ranks its own and the two whose ranks are asked for leave.
template <bool kR128>
__global__ __launch_bounds__(kLoudGateThreads) void k_loud_gate(LoudArgs a) {
  constexpr int kPart = kR128 ? kR128Part : 4;
  __shared__ double red[kLoudGateThreads];
  const pdmp3_loud_params& P = a.P;
  const int tid = threadIdx.x, C = P.channels;
  const size_t clip = (size_t)(a.clip0 + blockIdx.x);
  const float* const part = a.part + clip * C * P.n_chunks * 4 * kPart;
  float* const sub = a.sub + clip * C * (size_t)P.n_sub;
  float* const stats = reinterpret_cast<float*>(static_cast<uintptr_t>(a.stats_dst[clip]));
  float* const mom = reinterpret_cast<float*>(static_cast<uintptr_t>(a.mom_dst[clip]));

  float pk = 0.0f, tpk = 0.0f;
  for (int c = 0; c < C; c++) {
    const float* const pc = part + (size_t)c * P.n_chunks * 4 * kPart;
    for (long long i = tid; i < P.n_sub; i += kLoudGateThreads) sub[(size_t)c * P.n_sub + i] = loud_sub_sum(pc, i, P.q, kPart);
    for (long long w = tid; w < (long long)P.n_chunks * 4; w += kLoudGateThreads) {
      pk = fmaxf(pk, pc[w * kPart + 3]);
      if constexpr (kR128) tpk = fmaxf(tpk, pc[w * kPart + 4]);
    }
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
  double tp = 0.0, s_top = -INFINITY, gamma_r = -INFINITY, lra = 0.0, n_ar = 0.0, n_gr = 0.0;
  if constexpr (kR128) {
    __shared__ double vals[kR128MaxRange];
    __shared__ double pick[2];
    float* const st = reinterpret_cast<float*>(static_cast<uintptr_t>(a.st_dst[clip]));
    tp = fmax(peak, loud_reduce(red, (double)tpk, true));
    double sum_ar = 0.0;
    for (long long j = tid; j < a.n_st; j += kLoudGateThreads) {
      const double w = loud_zn(sub, P.n_sub, C, P.dual_mono, j, P.q, kR128Window), S = loud_l(w);
      if (st) st[j] = (float)S;
      s_top = fmax(s_top, S);
      if (j % kR128Every == 0 && S > -70.0) { n_ar += 1.0; sum_ar += w; }
    }
    s_top = loud_reduce(red, s_top, true);
    n_ar = loud_reduce(red, n_ar, false);
    sum_ar = loud_reduce(red, sum_ar, false);
    gamma_r = n_ar > 0.0 ? loud_l(sum_ar / n_ar) - 20.0 : -INFINITY;
    for (int m = tid; m < a.n_rng; m += kLoudGateThreads) {
      const double S = loud_l(loud_zn(sub, P.n_sub, C, P.dual_mono, (long long)m * kR128Every, P.q, kR128Window));
      const bool in = S > -70.0 && S > gamma_r;
      vals[m] = in ? S : INFINITY;
      n_gr += in ? 1.0 : 0.0;
    }
    if (tid < 2) pick[tid] = 0.0;
    n_gr = loud_reduce(red, n_gr, false);                        // (the barriers inside: the gated values are there)
    if (n_gr > 0.0) {
      const long long hi = r128_hi_index((long long)n_gr), lo = r128_lo_index((long long)n_gr);
      for (int m = tid; m < a.n_rng; m += kLoudGateThreads) {
        if (vals[m] == INFINITY) continue;
        const long long r = r128_rank(vals, a.n_rng, m);
        if (r == hi) pick[0] = vals[m];
        if (r == lo) pick[1] = vals[m];
      }
    }
    __syncthreads();
    lra = n_gr > 0.0 ? pick[0] - pick[1] : 0.0;
  }
  if (tid) return;
  const double L = n_rel > 0.0 ? loud_l(sum_rel / n_rel) : -INFINITY;
  const float g = loud_gain(L, kR128 && a.limit_tp ? tp : peak, P.target, P.peak_limit);
  stats[0] = (float)L; stats[1] = (float)top; stats[2] = (float)peak; stats[3] = g;
  stats[4] = (float)gamma; stats[5] = (float)P.n_mom; stats[6] = (float)n_abs; stats[7] = (float)n_rel;
  if constexpr (kR128) {
    stats[8] = (float)tp; stats[9] = (float)s_top; stats[10] = (float)lra; stats[11] = (float)gamma_r;
    stats[12] = (float)a.n_st; stats[13] = (float)a.n_rng; stats[14] = (float)n_ar; stats[15] = (float)n_gr;
  }
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

// a plan this file has no kernel for
static bool loud_plan_ok(const pdmp3_loud_params& P) {
  return P.n_in <= 0x7fffffffLL && (P.channels == 1 || P.channels == 2) && P.q >= 800 && P.n_chunks == (P.n_in + kLoudSpan - 1) / kLoudSpan &&
         P.n_sub == P.n_in / P.q && P.n_mom == (P.n_sub > 3 ? P.n_sub - 3 : 0);
}
template <bool kR128>
static hipError_t loud_launch(hipStream_t s, int n_clips, const LoudArgs& a) {
  const pdmp3_loud_params& P = a.P;
  const dim3 chunks((unsigned)P.n_chunks, (unsigned)n_clips, (unsigned)P.channels);
  hipLaunchKernelGGL(k_loud_states, chunks, dim3(64), 0, s, a);
  hipLaunchKernelGGL(k_loud_chain, dim3(1, (unsigned)n_clips, (unsigned)P.channels), dim3(64), 0, s, a);
  hipLaunchKernelGGL(k_loud_blocks<kR128>, chunks, dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_loud_gate<kR128>, dim3((unsigned)n_clips), dim3(kLoudGateThreads), 0, s, a);
  hipLaunchKernelGGL(k_loud_scale, dim3((unsigned)((P.n_in + 1023) / 1024), (unsigned)n_clips, (unsigned)P.channels), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t pdmp3_launch_clip_loudness(hipStream_t s, const pdmp3_mel_desc* descs, int n_clips, int clip0, const pdmp3_loud_tables* tab,
                                      const uint64_t* stats_dst, const uint64_t* mom_dst, double* states, double* starts, float* part, float* sub,
                                      float* gains, const pdmp3_loud_params* params) {
  const pdmp3_loud_params& P = *params;
  if (n_clips <= 0 || P.n_in <= 0) return hipSuccess;
  if (!loud_plan_ok(P)) return hipErrorInvalidValue;
  return loud_launch<false>(s, n_clips, LoudArgs{descs, clip0, tab, stats_dst, mom_dst, states, starts, part, sub, gains, P, nullptr, nullptr, 0, 0, 0});
}

// part: 8 floats a wave
hipError_t pdmp3_launch_clip_r128(hipStream_t s, const pdmp3_mel_desc* descs, int n_clips, int clip0, const pdmp3_loud_tables* tab, const float* taps,
                                  const uint64_t* stats_dst, const uint64_t* mom_dst, const uint64_t* st_dst, double* states, double* starts,
                                  float* part, float* sub, float* gains, const pdmp3_r128_params* params) {
  const pdmp3_loud_params& P = params->loud;
  if (n_clips <= 0 || P.n_in <= 0) return hipSuccess;
  const int n_st = P.n_sub > kR128Window - 1 ? P.n_sub - (kR128Window - 1) : 0;
  if (!loud_plan_ok(P) || params->n_st != n_st || params->n_rng != (n_st + kR128Every - 1) / kR128Every || params->n_rng > kR128MaxRange ||
      (params->limit_true_peak & ~1))
    return hipErrorInvalidValue;
  return loud_launch<true>(s, n_clips, LoudArgs{descs, clip0, tab, stats_dst, mom_dst, states, starts, part, sub, gains, P, taps, st_dst,
                                                params->n_st, params->n_rng, params->limit_true_peak});
}
