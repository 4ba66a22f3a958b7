// tempogram.hip -- k_clip_onset, k_clip_tempogram, k_clip_tempo: the log-mel batch that k_clip_mel_long wrote into the stream
// object's fourth audio stage to the onset envelope, its autocorrelation tempogram and the tempo estimate (include/pdmp3_bulk.h
// pdmp3_amd_bulk_decode_clips_tempogram).  Launched by stream.hip pdmp3_hip_clip_tempogram.  A translation
// unit of its own, so that every other kernel's code is what it is without it.  The kernels' phases are tempogram_core.h's,
// shared with the host build of the tests; here: the device's operations, the barriers between the phases and the launches.
#include <hip/hip_runtime.h>

#include "../../include/pdmp3_hip.h"
#include "tempogram_core.h"

namespace {

using namespace pdmp3;

typedef float f32x4 __attribute__((ext_vector_type(4)));

// pitch_core.h's operations on the device (as pitch.hip's)
struct DevOps {
  typedef f32x4 acc4;
  float* f;
  double* d;
  __device__ __forceinline__ float ldf(unsigned i) const { return f[i]; }
  __device__ __forceinline__ void stf(unsigned i, float v) const { f[i] = v; }
  __device__ __forceinline__ double ldd(unsigned i) const { return d[i]; }
  __device__ __forceinline__ void std(unsigned i, double v) const { d[i] = v; }
  __device__ __forceinline__ acc4 zero() const { return f32x4{0.0f, 0.0f, 0.0f, 0.0f}; }
  __device__ __forceinline__ void mfma(float a, float b, acc4& c) const { c = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
  // what a wave's lanes wrote to LDS is there for its other lanes (LDS operations of a wave complete in order)
  __device__ __forceinline__ void sync() const {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  __device__ __forceinline__ void issued() const { __builtin_amdgcn_sched_barrier(0); }
};

template <class T>
__device__ __forceinline__ T* at(uint64_t address) { return reinterpret_cast<T*>(static_cast<uintptr_t>(address)); }
// where the envelope and the tempogram of a clip lie: the destination in the mode that returns them, else the stage
__device__ __forceinline__ float* env_of(const pdmp3_tempogram_desc& d, const pdmp3_tempogram_params& P, int ch) {
  return at<float>(d.env) + (size_t)ch * (P.out_mode == 0 ? (size_t)d.dst_chan_stride : (size_t)P.env_stride);
}
__device__ __forceinline__ float* tg_of(const pdmp3_tempogram_desc& d, const pdmp3_tempogram_params& P, int ch) {
  return at<float>(d.tg) + (size_t)ch * (P.out_mode == 1 ? (size_t)d.dst_chan_stride : (size_t)P.win * (size_t)P.n_frames);
}

// A lane a frame: consecutive lanes read consecutive floats of every band's row.  No LDS, no atomics.
__global__ __launch_bounds__(kOnsetThreads) void k_clip_onset(const pdmp3_tempogram_desc* __restrict__ descs, pdmp3_tempogram_params P) {
  const pdmp3_tempogram_desc d = descs[blockIdx.y];
  const int ch = blockIdx.x % P.channels;
  const long long e = (long long)(blockIdx.x / P.channels) * kOnsetThreads + threadIdx.x;
  if (e >= P.n_env) return;
  const float* const l = at<const float>(d.mel) + (size_t)ch * (size_t)P.n_mels * (size_t)P.n_mel_frames;
  env_of(d, P, ch)[e] = onset_value(l, P, e);
}

// One workgroup of frames_wg waves per (frames_wg consecutive frames, channel, clip), one frame a wave: the wave's own span,
// its matrix products, its quotients; after the barrier consecutive threads store consecutive frames.  Every frame's values
// come from the same chains of operations whatever its place in the workgroup.  No atomics.
template <int TILES>
__device__ __forceinline__ void tempogram_workgroup(const pdmp3_tempogram_desc& d, const pdmp3_tempogram_params& P, const float* w, int ch,
                                                    long long f0, float* lds) {
  const unsigned tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
  const DevOps o{lds, reinterpret_cast<double*>(lds)};
  const tempogram_layout L = tempogram_lds(P);
  if (f0 + wave < P.n_frames) tempogram_frame<TILES>(o, P, L, env_of(d, P, ch), w, f0 + wave, wave, lane);
  __syncthreads();
  tempogram_store(o, P, L, tg_of(d, P, ch), f0, tid);
}

__device__ __forceinline__ void tempogram_tiles(const pdmp3_tempogram_desc* __restrict__ descs, const float* __restrict__ w,
                                                const pdmp3_tempogram_params& P, float* lds) {
  const pdmp3_tempogram_desc d = descs[blockIdx.y];
  const int ch = blockIdx.x % P.channels;
  const long long f0 = (long long)(blockIdx.x / P.channels) * P.frames_wg;
  if (f0 >= P.n_frames) return;
  switch (P.tiles) {
    case 1: tempogram_workgroup<1>(d, P, w, ch, f0, lds); break;
    case 2: tempogram_workgroup<2>(d, P, w, ch, f0, lds); break;
    case 3: tempogram_workgroup<3>(d, P, w, ch, f0, lds); break;
    default: tempogram_workgroup<4>(d, P, w, ch, f0, lds); break;
  }
}

__global__ __launch_bounds__(kTempogramMaxThreads) void k_clip_tempogram(const pdmp3_tempogram_desc* __restrict__ descs,
                                                                         const float* __restrict__ w, pdmp3_tempogram_params P) {
  extern __shared__ __align__(16) float lds[];
  tempogram_tiles(descs, w, P, lds);
}

// more than the 64 KB a launch can ask for dynamically: the same code on a static array, as the other kernels' _big forms
__global__ __launch_bounds__(kTempogramMaxThreads) void k_clip_tempogram_big(const pdmp3_tempogram_desc* __restrict__ descs,
                                                                             const float* __restrict__ w, pdmp3_tempogram_params P) {
  __shared__ __align__(16) float lds[PDMP3_MEL_LDS_MAX / sizeof(float)];
  tempogram_tiles(descs, w, P, lds);
}

// One workgroup per (channel, clip), a thread a lag; the decision is wave 0's.
__global__ __launch_bounds__(kTempoThreads) void k_clip_tempo(const pdmp3_tempogram_desc* __restrict__ descs, const double* __restrict__ prior,
                                                              pdmp3_tempogram_params P) {
  __shared__ __align__(16) double s[kTempoMaxWin + 128];
  const pdmp3_tempogram_desc d = descs[blockIdx.y];
  const int ch = blockIdx.x;
  const DevOps o{reinterpret_cast<float*>(s), s};
  tempo_scores(o, P, tg_of(d, P, ch), prior, threadIdx.x);
  __syncthreads();
  if (threadIdx.x < 64u) tempo_decide(o, P, at<float>(d.dst) + (size_t)ch * (size_t)d.dst_chan_stride, threadIdx.x);
}

}  // namespace

hipError_t pdmp3_launch_clip_tempogram(hipStream_t s, const pdmp3_tempogram_desc* descs, int n_clips, const float* window, const double* prior,
                                       const pdmp3_tempogram_params* params) {
  const pdmp3_tempogram_params P = *params;
  if (n_clips <= 0 || P.n_frames <= 0) return hipSuccess;
  if (P.tiles < 1 || P.tiles > 4 || P.frames_wg < 1 || P.frames_wg > 8 || P.win > kTempoMaxWin || P.lds_bytes > PDMP3_MEL_LDS_MAX) return hipErrorInvalidValue;
  {
    const unsigned groups = (unsigned)((P.n_env + kOnsetThreads - 1) / kOnsetThreads);
    hipLaunchKernelGGL(k_clip_onset, dim3(groups * (unsigned)P.channels, (unsigned)n_clips), dim3(kOnsetThreads), 0, s, descs, P);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess || P.out_mode == 0) return e;
  }
  {
    const unsigned groups = (unsigned)((P.n_frames + P.frames_wg - 1) / P.frames_wg);
    const dim3 grid(groups * (unsigned)P.channels, (unsigned)n_clips), block(64u * (unsigned)P.frames_wg);
    if (P.lds_bytes > PDMP3_MEL_LDS_SOFT) hipLaunchKernelGGL(k_clip_tempogram_big, grid, block, 0, s, descs, window, P);
    else hipLaunchKernelGGL(k_clip_tempogram, grid, block, P.lds_bytes, s, descs, window, P);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess || P.out_mode == 1) return e;
  }
  hipLaunchKernelGGL(k_clip_tempo, dim3((unsigned)P.channels, (unsigned)n_clips), dim3(kTempoThreads), 0, s, descs, prior, P);
  return hipGetLastError();
}
