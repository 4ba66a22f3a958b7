// pitch.hip -- k_clip_pitch: rows of the resampled signal of a batch of clips (k_clip_audio's output in the stream object's
// third audio stage) to their YIN pitch -- f0, aperiodicity and lag, or the cumulative-mean-normalised difference curve --
// planar float32 [rows][n_frames] per clip and channel (include/pdmp3_bulk.h pdmp3_amd_bulk_decode_clips_pitch; DESIGN.md
// section 20).  Launched by stream.hip pdmp3_hip_clip_pitch.  A translation unit of its own, so that every other kernel's code is
// what it is without it.  The kernel's phases are pitch_core.h's, shared with the host build of the tests; here: the device's
// operations, the barriers between the phases and the launch.
#include <hip/hip_runtime.h>

#include "../../include/pdmp3_hip.h"
#include "pitch_core.h"

namespace {

using namespace pdmp3;

typedef float f32x4 __attribute__((ext_vector_type(4)));

// pitch_core.h's operations on the device
struct DevOps {
  typedef f32x4 acc4;
  float* f;
  double* d;
  __device__ __forceinline__ float ldf(unsigned i) const { return f[i]; }
  __device__ __forceinline__ void stf(unsigned i, float v) const { f[i] = v; }
  __device__ __forceinline__ double ldd(unsigned i) const { return d[i]; }
  __device__ __forceinline__ void std(unsigned i, double v) const { d[i] = v; }
  __device__ __forceinline__ acc4 zero() const { return f32x4{0.0f, 0.0f, 0.0f, 0.0f}; }
  // v_mfma_f32_16x16x4_f32: lane l = (j = l & 15, kq = l >> 4) holds A[row j][k = kq], B[k = kq][col j] and D[row 4 kq + r][col j]
  __device__ __forceinline__ void mfma(float a, float b, acc4& c) const { c = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
  // what a wave's lanes wrote to LDS is there for its other lanes (LDS operations of a wave complete in order)
  __device__ __forceinline__ void sync() const {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  __device__ __forceinline__ void issued() const { __builtin_amdgcn_sched_barrier(0); }
  __device__ __forceinline__ bool any(bool c) const { return __builtin_amdgcn_ballot_w64(c) != 0; }
  __device__ __forceinline__ int shfl_xor(int v, int m) const { return __shfl_xor(v, m); }
};

// One workgroup of frames_wg waves per (frames_wg consecutive frames, channel, clip), one frame a wave:
//   1. the workgroup's span -- (frames_wg - 1) hop + N samples, zeros outside the clip's row, zeros around it as far as the
//      matrix operands reach -- goes to LDS once, skewed (pitch_at);
//   2. the binary64 prefix sums of its squares, one scan a workgroup;
//   3. a wave: r^ of 256 lags a tile on v_mfma_f32_16x16x4_f32, every accumulator element a distinct lag, B loaded once a
//      k-step for all tiles; then d, S and d' in binary64 and the decision on the binary32 curve;
//   4. consecutive threads store consecutive frames.
// Every frame's values come from the same chains of operations whatever its place in the workgroup.  No atomics.
template <int TILES>
__device__ __forceinline__ void pitch_workgroup(const pdmp3_mel_desc& d, const pdmp3_pitch_params& P, int ch, long long f0, float* lds) {
  const unsigned tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
  const DevOps o{lds, reinterpret_cast<double*>(lds)};
  const pitch_layout L = pitch_lds(P);
  const float* const row = reinterpret_cast<const float*>(static_cast<uintptr_t>(d.src)) + (size_t)ch * d.src_chan_stride;
  float* const out = reinterpret_cast<float*>(static_cast<uintptr_t>(d.dst)) + (size_t)ch * d.dst_chan_stride;
  pitch_load(o, P, row, f0, d.lead, tid);
  __syncthreads();
  pitch_sq_pieces(o, P, L, tid);
  __syncthreads();
  if (wave == 0) pitch_sq_scan(o, P, L, lane);
  __syncthreads();
  pitch_sq_write(o, P, L, tid);
  __syncthreads();
  if (f0 + wave < P.n_frames) pitch_frame<TILES>(o, P, L, wave, lane);
  __syncthreads();
  pitch_store(o, P, L, out, f0, tid);
}

__device__ __forceinline__ void pitch_tiles(const pdmp3_mel_desc* __restrict__ descs, const pdmp3_pitch_params& P, float* lds) {
  const pdmp3_mel_desc d = descs[blockIdx.y];
  const int ch = blockIdx.x % P.channels;
  const long long f0 = (long long)(blockIdx.x / P.channels) * P.frames_wg;
  if (f0 >= P.n_frames) return;
  switch (P.tiles) {
    case 1: pitch_workgroup<1>(d, P, ch, f0, lds); break;
    case 2: pitch_workgroup<2>(d, P, ch, f0, lds); break;
    case 3: pitch_workgroup<3>(d, P, ch, f0, lds); break;
    case 4: pitch_workgroup<4>(d, P, ch, f0, lds); break;
    case 5: pitch_workgroup<5>(d, P, ch, f0, lds); break;
    case 6: pitch_workgroup<6>(d, P, ch, f0, lds); break;
    case 7: pitch_workgroup<7>(d, P, ch, f0, lds); break;
    default: pitch_workgroup<8>(d, P, ch, f0, lds); break;
  }
}

__global__ __launch_bounds__(kPitchMaxThreads) void k_clip_pitch(const pdmp3_mel_desc* __restrict__ descs, pdmp3_pitch_params P) {
  extern __shared__ __align__(16) float lds[];
  pitch_tiles(descs, P, lds);
}

// A workgroup that needs more than the 64 KB a launch can ask for dynamically (the default frame at eight frames a workgroup
// among them): the same code on a static array of all the LDS a workgroup may have, as the other kernels' _big forms.
__global__ __launch_bounds__(kPitchMaxThreads) void k_clip_pitch_big(const pdmp3_mel_desc* __restrict__ descs, pdmp3_pitch_params P) {
  __shared__ __align__(16) float lds[PDMP3_MEL_LDS_MAX / sizeof(float)];
  pitch_tiles(descs, P, lds);
}

}  // namespace

hipError_t pdmp3_launch_clip_pitch(hipStream_t s, const pdmp3_mel_desc* descs, int n_clips, const pdmp3_pitch_params* params) {
  const pdmp3_pitch_params P = *params;
  if (n_clips <= 0 || P.n_frames <= 0) return hipSuccess;
  if (P.tiles < 1 || P.tiles > 8 || P.frames_wg < 1 || P.frames_wg > 8 || P.lds_bytes > PDMP3_MEL_LDS_MAX) return hipErrorInvalidValue;
  const unsigned groups = (unsigned)((P.n_frames + P.frames_wg - 1) / P.frames_wg);
  const dim3 grid(groups * (unsigned)P.channels, (unsigned)n_clips), block(64u * (unsigned)P.frames_wg);
  if (P.lds_bytes > PDMP3_MEL_LDS_SOFT) hipLaunchKernelGGL(k_clip_pitch_big, grid, block, 0, s, descs, P);
  else hipLaunchKernelGGL(k_clip_pitch, grid, block, P.lds_bytes, s, descs, P);
  return hipGetLastError();
}
