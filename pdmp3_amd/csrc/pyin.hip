// pyin.hip -- k_clip_pyin_obs and k_clip_pyin_path: the cumulative-mean-normalised difference curves that k_clip_pitch wrote
// into a stage to pYIN's observation probabilities and voicing probability, and from those the most probable path through
// the pitch bins' voiced and unvoiced states (include/pdmp3_bulk.h pdmp3_amd_bulk_decode_clips_pyin).
// Launched by stream.hip pdmp3_hip_clip_pyin.  A translation unit of its own, so that every other kernel's code is what it
// is without it.  The kernels' phases are pyin_core.h's, shared with the host build of the tests; here: the device's
// operations, the barriers between the phases and the launches.
#include <hip/hip_runtime.h>

#include "../../include/pdmp3_hip.h"
#include "pyin_core.h"

namespace {

using namespace pdmp3;

// pyin_core.h's operations on the device
struct DevOps {
  float* f;
  double* d;
  __device__ __forceinline__ float ldf(unsigned i) const { return f[i]; }
  __device__ __forceinline__ void stf(unsigned i, float v) const { f[i] = v; }
  __device__ __forceinline__ unsigned ldu(unsigned i) const { return reinterpret_cast<unsigned*>(f)[i]; }
  __device__ __forceinline__ void stu(unsigned i, unsigned v) const { reinterpret_cast<unsigned*>(f)[i] = v; }
  __device__ __forceinline__ double ldd(unsigned i) const { return d[i]; }
  __device__ __forceinline__ void std(unsigned i, double v) const { d[i] = v; }
  // what a wave's lanes wrote to LDS is there for its other lanes (LDS operations of a wave complete in order)
  __device__ __forceinline__ void sync() const {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  __device__ __forceinline__ unsigned long long ballot(bool c) const { return __builtin_amdgcn_ballot_w64(c); }
  __device__ __forceinline__ int shfl_xor(int v, int m) const { return __shfl_xor(v, m); }
  __device__ __forceinline__ double log(double x) const { return ::log(x); }
};

// One workgroup of frames_wg waves per (frames_wg consecutive frames, channel, clip), one frame a wave.  No atomics.
__global__ __launch_bounds__(kPyinObsMaxThreads) void k_clip_pyin_obs(const pdmp3_pyin_desc* __restrict__ descs, const double* __restrict__ tab,
                                                                     pdmp3_pyin_params P) {
  extern __shared__ __align__(16) float lds[];
  const pdmp3_pyin_desc d = descs[blockIdx.y];
  const int ch = blockIdx.x % P.channels;
  const long long f0 = (long long)(blockIdx.x / P.channels) * P.frames_wg;
  if (f0 >= P.n_frames) return;
  const unsigned tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
  const DevOps o{lds, reinterpret_cast<double*>(lds)};
  const size_t F = (size_t)P.n_frames;
  const float* const curve = reinterpret_cast<const float*>(static_cast<uintptr_t>(d.curve)) + (size_t)ch * ((size_t)P.tmax + 1u) * F;
  float* const out = reinterpret_cast<float*>(static_cast<uintptr_t>(d.obs)) +
                     (size_t)ch * (P.out_mode == 1 ? (size_t)d.dst_chan_stride : ((size_t)P.n_bins + 1u) * F);
  pyin_obs_load(o, P, curve, f0, tid);
  __syncthreads();
  if (f0 + wave < P.n_frames) pyin_obs_frame(o, P, tab, wave, lane);
  __syncthreads();
  pyin_obs_store(o, P, out, f0, tid);
}

// One workgroup per (clip, channel), sequential over the frames; one barrier a frame.
__device__ __forceinline__ void pyin_path(const pdmp3_pyin_desc* __restrict__ descs, const double* __restrict__ tab, const pdmp3_pyin_params& P,
                                          double* lds) {
  const pdmp3_pyin_desc d = descs[blockIdx.y];
  const int ch = blockIdx.x;
  const unsigned tid = threadIdx.x;
  const DevOps o{reinterpret_cast<float*>(lds), lds};
  const size_t F = (size_t)P.n_frames, nb = (size_t)P.n_bins;
  const float* const obs = reinterpret_cast<const float*>(static_cast<uintptr_t>(d.obs)) + (size_t)ch * (nb + 1u) * F;
  uint16_t* const bp = reinterpret_cast<uint16_t*>(static_cast<uintptr_t>(d.bp)) + (size_t)ch * 2u * nb * F;
  float* const out = reinterpret_cast<float*>(static_cast<uintptr_t>(d.dst)) + (size_t)ch * (size_t)d.dst_chan_stride;
  pyin_path_window(o, P, tab, tid);
  __syncthreads();
  for (long long f = 0; f < P.n_frames; f++) {
    pyin_path_step(o, P, tab, obs + (size_t)f * (nb + 1u), bp + (size_t)f * 2u * nb, f, tid);
    __syncthreads();
  }
  if (tid == 0) pyin_path_back(o, P, bp);
  __syncthreads();
  pyin_path_store(P, tab, obs, bp, out, tid);
}

__global__ __launch_bounds__(kPyinPathMaxThreads) void k_clip_pyin_path(const pdmp3_pyin_desc* __restrict__ descs, const double* __restrict__ tab,
                                                                       pdmp3_pyin_params P) {
  extern __shared__ __align__(16) double lds_d[];
  pyin_path(descs, tab, P, lds_d);
}

// More states than the 64 KB a launch can ask for dynamically hold: the same code on a static array of all the LDS a
// workgroup may have, as the other kernels' _big forms.
__global__ __launch_bounds__(kPyinPathMaxThreads) void k_clip_pyin_path_big(const pdmp3_pyin_desc* __restrict__ descs,
                                                                           const double* __restrict__ tab, pdmp3_pyin_params P) {
  __shared__ __align__(16) double lds_d[PDMP3_MEL_LDS_MAX / sizeof(double)];
  pyin_path(descs, tab, P, lds_d);
}

}  // namespace

hipError_t pdmp3_launch_clip_pyin(hipStream_t s, const pdmp3_pyin_desc* descs, int n_clips, const double* tables, const pdmp3_pyin_params* params) {
  const pdmp3_pyin_params P = *params;
  if (n_clips <= 0 || P.n_frames <= 0) return hipSuccess;
  if (P.frames_wg < 1 || P.frames_wg > 8 || P.obs_lds_bytes > PDMP3_MEL_LDS_SOFT || P.path_lds_bytes > PDMP3_MEL_LDS_MAX || P.path_threads < 64 ||
      P.path_threads > kPyinPathMaxThreads || (P.path_threads & 63))
    return hipErrorInvalidValue;
  const unsigned groups = (unsigned)((P.n_frames + P.frames_wg - 1) / P.frames_wg);
  hipLaunchKernelGGL(k_clip_pyin_obs, dim3(groups * (unsigned)P.channels, (unsigned)n_clips), dim3(64u * (unsigned)P.frames_wg), P.obs_lds_bytes, s,
                     descs, tables, P);
  if (const hipError_t e = hipGetLastError(); e != hipSuccess || P.out_mode != 0) return e;
  const dim3 grid((unsigned)P.channels, (unsigned)n_clips), block((unsigned)P.path_threads);
  if (P.path_lds_bytes > PDMP3_MEL_LDS_SOFT) hipLaunchKernelGGL(k_clip_pyin_path_big, grid, block, 0, s, descs, tables, P);
  else hipLaunchKernelGGL(k_clip_pyin_path, grid, block, P.path_lds_bytes, s, descs, tables, P);
  return hipGetLastError();
}
