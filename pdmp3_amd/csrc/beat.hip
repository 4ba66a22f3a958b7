// beat.hip -- k_clip_beat_score, k_clip_beat_dp and k_clip_beat_pick: the onset envelope that k_clip_onset wrote into a stage to
// the local score, the dynamic programme's cumulative score and back-links, and the beats (include/pdmp3_bulk.h
// pdmp3_amd_bulk_decode_clips_beats).  Launched by stream.hip pdmp3_hip_clip_beat.  A translation unit of
// its own, so that every other kernel's code is what it is without it.  The kernels' phases are beat_core.h's, shared with the
// host build of the tests; here: the device's operations, the barriers between the phases and the launches.
#include <hip/hip_runtime.h>

#include "../../include/pdmp3_hip.h"
#include "beat_core.h"

#pragma clang fp contract(off)

namespace {

using namespace pdmp3;

// beat_core.h's operations on the device
struct DevOps {
  double* d;
  __device__ __forceinline__ unsigned ldu(unsigned i) const { return reinterpret_cast<unsigned*>(d)[i]; }
  __device__ __forceinline__ void stu(unsigned i, unsigned v) const { reinterpret_cast<unsigned*>(d)[i] = v; }
  __device__ __forceinline__ double ldd(unsigned i) const { return d[i]; }
  __device__ __forceinline__ void std(unsigned i, double v) const { d[i] = v; }
  __device__ __forceinline__ int shfl_xor(int v, int m) const { return __shfl_xor(v, m); }
};

template <class T>
__device__ __forceinline__ T* at(uint64_t address) { return reinterpret_cast<T*>(static_cast<uintptr_t>(address)); }

// what a (clip, channel) of the launch works on
struct Row {
  pdmp3_beat_desc d;
  int ch, n;
  const float* env;
  double* hdr;
  double* cum;
  double* lmv;
  float* ls;
  int* back;
  int* bt;
  float* dst;
  float* stats;
};
__device__ __forceinline__ Row row_of(const pdmp3_beat_desc* descs, double* work, int first, const pdmp3_beat_params& P) {
  Row r;
  r.d = descs[blockIdx.y];
  r.ch = (int)blockIdx.x;
  r.n = (int)r.d.n < P.n_frames ? (int)r.d.n : P.n_frames;
  r.env = at<const float>(r.d.env) + (size_t)r.ch * (size_t)P.env_stride;
  const beat_work w = beat_work_of(P.n_frames);
  r.hdr = work + ((size_t)(first + (int)blockIdx.y) * (size_t)P.channels + (size_t)r.ch) * (size_t)P.work_stride;
  r.cum = r.hdr + w.cum; r.lmv = r.hdr + w.lmv;
  r.ls = reinterpret_cast<float*>(r.hdr) + w.ls;
  r.back = reinterpret_cast<int*>(r.hdr) + w.back;
  r.bt = reinterpret_cast<int*>(r.hdr) + w.bt;
  r.dst = at<float>(r.d.dst) + (size_t)r.ch * (size_t)r.d.dst_chan_stride;
  r.stats = r.d.stats ? at<float>(r.d.stats) + (size_t)r.ch * 8u : nullptr;
  return r;
}

// One workgroup per (channel, clip).  No atomics.
__global__ __launch_bounds__(kBeatThreads) void k_clip_beat_score(const pdmp3_beat_desc* __restrict__ descs, const double* __restrict__ tab,
                                                                  double* __restrict__ work, int first, pdmp3_beat_params P) {
  extern __shared__ __align__(16) double lds[];
  const Row r = row_of(descs, work, first, P);
  const unsigned tid = threadIdx.x;
  const DevOps o{lds};
  const int F = P.n_frames, n = r.n, Pd = beat_period(P, r.hdr);
  const beat_score_layout L = beat_score_lds(P.p_max, F);
  double norm = -1.0;
  bool run = Pd > 0 && n >= 2;
  if (run) {                                                    // (the same for every thread of the workgroup)
    const double* const g = tab + beat_table_at(P.p_min, Pd);
    beat_score_sums(o, L, r.env, n, Pd, g, 0.0, 0, tid);
    __syncthreads();
    const double m = beat_score_total(o, L, n) / (double)n;
    __syncthreads();
    beat_score_sums(o, L, r.env, n, Pd, g, m, 1, tid);
    __syncthreads();
    norm = sqrt(beat_score_total(o, L, n) / (double)(n - 1));
    run = beat_norm_ok(norm);
  }
  if (tid == 0) {
    r.hdr[2] = norm; r.hdr[3] = run ? 1.0 : 0.0;
    if (r.stats) {
      r.stats[0] = beat_bpm(P, r.hdr); r.stats[1] = (float)Pd; r.stats[2] = 0.0f; r.stats[3] = -1.0f; r.stats[4] = -1.0f;
      r.stats[5] = run ? (float)norm : -1.0f; r.stats[6] = -1.0f; r.stats[7] = (float)n;
    }
  }
  const int lim = P.out_mode == 0 ? F : n;
  for (int t0 = 0; t0 < lim; t0 += kBeatTile) {
    if (run && t0 < n) {
      __syncthreads();
      beat_score_load(o, L, r.env, n, Pd, norm, t0, tid);
      __syncthreads();
    }
    const int i = t0 + (int)tid;
    if (i < lim) {
      const float v = run && i < n ? beat_score_frame(o, L, Pd, tid) : 0.0f;
      if (i < n) r.ls[i] = v;
      if (P.out_mode == 0) r.dst[i] = v;
    }
  }
}

// One workgroup per (channel, clip), sequential over the steps of h frames; one barrier a step.
__global__ __launch_bounds__(kBeatThreads) void k_clip_beat_dp(const pdmp3_beat_desc* __restrict__ descs, const double* __restrict__ tab,
                                                               double* __restrict__ work, int first, pdmp3_beat_params P) {
  extern __shared__ __align__(16) double lds[];
  const Row r = row_of(descs, work, first, P);
  const unsigned tid = threadIdx.x;
  const DevOps o{lds};
  const int F = P.n_frames, Pd = beat_period(P, r.hdr);
  const bool run = r.hdr[3] == 1.0;
  const int n = run ? r.n : 0;
  if (run) {
    const beat_dp_layout L = beat_dp_lds(P.p_max);
    beat_dp_head(o, L, tab + beat_table_at(P.p_min, Pd) + (size_t)Pd + 1u, r.ls, n, Pd, tid);
    __syncthreads();
    const double mx = beat_dp_red(o, L, true);
    __syncthreads();
    beat_dp_first(o, L, r.ls, n, mx, tid);
    __syncthreads();
    const int i0 = (int)beat_dp_red(o, L, false);
    const int h = beat_half(Pd);
    for (int s0 = 0; s0 < n; s0 += h) {
      beat_dp_step(o, P, L, Pd, n, i0, s0, r.ls, r.cum, r.back, r.dst, tid);
      __syncthreads();
    }
  }
  if (P.out_mode == 1)
    for (int i = n + (int)tid; i < F; i += kBeatThreads) { r.dst[i] = 0.0f; r.dst[(size_t)F + (size_t)i] = -1.0f; }
}

// One workgroup per (channel, clip).
__global__ __launch_bounds__(kBeatThreads) void k_clip_beat_pick(const pdmp3_beat_desc* __restrict__ descs, double* __restrict__ work, int first,
                                                                 pdmp3_beat_params P) {
  __shared__ __align__(16) double lds[kBeatPickWords / 2];
  const Row r = row_of(descs, work, first, P);
  const unsigned tid = threadIdx.x;
  const DevOps o{lds};
  const int F = P.n_frames, n = r.n;
  float* const mask = r.dst;
  float* const list = r.dst + (size_t)F;
  for (int i = (int)tid; i < F; i += kBeatThreads) { mask[i] = 0.0f; list[i] = -1.0f; }
  if (r.hdr[3] != 1.0) return;                                  // (the same for every thread of the workgroup)
  beat_pick_count(o, r.cum, n, tid);
  __syncthreads();
  const unsigned M = beat_pick_before(o, (unsigned)kBeatThreads);
  if (!M) return;
  beat_pick_gather(o, r.cum, r.lmv, n, tid);
  __syncthreads();
  beat_pick_rank(o, r.lmv, M, tid);
  __syncthreads();
  beat_pick_last(o, r.cum, n, beat_pick_median(o, M), tid);
  __syncthreads();
  if (tid == 0) beat_pick_walk(o, P, r.ls, r.back, r.bt);
  __syncthreads();
  const int t_first = (int)o.ldd(2u), t_last = (int)o.ldd(3u), q = (int)o.ldd(4u);
  for (int t = t_first + (int)tid; t <= t_last; t += kBeatThreads) {
    const int b = r.bt[q - 1 - t];
    mask[b] = 1.0f;
    list[t - t_first] = (float)b;
  }
  if (tid == 0 && r.stats) {
    r.stats[2] = t_last >= t_first ? (float)(t_last - t_first + 1) : 0.0f;
    r.stats[3] = (float)q; r.stats[4] = (float)o.ldd(5u); r.stats[6] = (float)o.ldd(6u);
  }
}

}  // namespace

hipError_t pdmp3_launch_clip_beat(hipStream_t s, const pdmp3_beat_desc* descs, int n_clips, int first, const double* tables, double* work,
                                  const pdmp3_beat_params* params) {
  const pdmp3_beat_params P = *params;
  if (n_clips <= 0 || P.n_frames <= 0) return hipSuccess;
  if (P.p_min < 1 || P.p_max > kBeatMaxPeriod || P.p_min > P.p_max || P.n_frames > kBeatMaxFrames || P.score_lds_bytes > PDMP3_MEL_LDS_SOFT ||
      P.dp_lds_bytes > PDMP3_MEL_LDS_SOFT)
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)P.channels, (unsigned)n_clips), block((unsigned)kBeatThreads);
  hipLaunchKernelGGL(k_clip_beat_score, grid, block, P.score_lds_bytes, s, descs, tables, work, first, P);
  if (const hipError_t e = hipGetLastError(); e != hipSuccess || P.out_mode == 0) return e;
  hipLaunchKernelGGL(k_clip_beat_dp, grid, block, P.dp_lds_bytes, s, descs, tables, work, first, P);
  if (const hipError_t e = hipGetLastError(); e != hipSuccess || P.out_mode == 1) return e;
  hipLaunchKernelGGL(k_clip_beat_pick, grid, block, 0, s, descs, work, first, P);
  return hipGetLastError();
}
