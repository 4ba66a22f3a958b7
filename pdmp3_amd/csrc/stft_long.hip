// stft_long.hip -- k_clip_stft_long: the short-time Fourier transform of clips at n_fft 2048 and 4096 as a two-stage
// transform N = 64 N2 (include/pdmp3_bulk.h pdmp3_amd_bulk_decode_clips_stft_long).  Rows in, layouts
// out and the pointwise arithmetic are k_clip_stft's (stft.hip, stft_core.h); the index maps, the LDS layouts with their
// banks, the twiddle step and the Nyquist bin's chain are stft_long_core.h's.  Launched by stream.hip
// pdmp3_hip_clip_stft_long.  A translation unit of its own; the two stages are stft_long_stages.h's, one source for this
// kernel and k_clip_mel_long, inlined here.
#include <hip/hip_runtime.h>

#include "../../include/pdmp3_hip.h"
#include "stft_long_stages.h"

namespace {

using namespace pdmp3;

// One workgroup of eight waves per (tile of FT frames, 16 values k1 = 16 kt .. 16 kt + 15, channel, clip); n = N2 n1 + n2,
// k = k1 + 64 k2.
//   0. the tile's span -- (FT - 1) hop + N samples, zeros outside the clip's row -- goes to LDS once, plain;
//   1. stage 1 (stftl_stage1), rows (frame, n2), columns k1: the window product, the 64-term chains and the twiddle, into Z
//      in LDS;
//   2. the Nyquist bin, in the workgroups with kt = 0: lane fl of wave 0 runs the chain over Z[fl][.][k1 = 0] and stores it;
//   3. stage 2 (stftl_stage2_operand, stftl_stage2_chains), rows (frame, k1), columns k2 < N2 / 2: the chains of 2 N2 terms out
//      of Z; what is stored (stft_value; mode 0: the pair) goes to the workgroup's staging tile, which lies where the span lay;
//   4. consecutive lanes store consecutive frames of one bin, mode 0 consecutive (Re, Im) pairs.  Frames from F on are not
//      stored; the bins are exactly 0 .. N / 2.
// Every frame's values come from the same chains of operations whatever its place in the tile.
template <int N2, int FT>
__device__ __forceinline__ void stft_long_tile(const pdmp3_mel_desc& d, const float* __restrict__ tab, const pdmp3_stft_long_params& P,
                                               int ch, int kt, long long f0, float* lds) {
  constexpr int N = 64 * N2, K2 = N2 / 2, NCT = K2 / 16;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 15, kq = lane >> 4;
  const int mode = P.out_mode;
  float* const span = lds;
  float* const stage = lds;
  float* const z = lds + P.span_floats;
  const float* const row = reinterpret_cast<const float*>(static_cast<uintptr_t>(d.src)) + (size_t)ch * d.src_chan_stride;
  float* const out = reinterpret_cast<float*>(static_cast<uintptr_t>(d.dst)) + (size_t)ch * d.dst_chan_stride;

  span_load_plain<kStftLongThreads>(span, row, P.n_in, f0, P.hop, d.lead, stftl_span(FT, P.hop, N), tid);
  __syncthreads();

  stftl_stage1<N2, FT>(span, tab, (unsigned)P.hop, kt, wave, j, kq, z);
  __syncthreads();

  if (kt == 0 && tid < FT && f0 + tid < P.n_frames) {
    float re, im;
    stftl_nyquist(z, tid, N2, &re, &im);
    const size_t at = (size_t)(N / 2) * (size_t)P.n_frames + (size_t)(f0 + tid);
    if (mode != 0) out[at] = stft_value(re, im, P.floor, mode);
    else *reinterpret_cast<f32x2*>(out + 2 * at) = f32x2{re, im};
  }

  {
    const int ct = wave % NCT;
    float b_re[N2 / 2], b_im[N2 / 2];
    stftl_stage2_operand<N2>(tab, ct, j, kq, b_re, b_im);
    for (int fl = wave / NCT; fl < FT; fl += 8 / NCT) {
      f32x4 re, im;
      stftl_stage2_chains<N2>(z, fl, j, kq, b_re, b_im, re, im);
#pragma unroll
      for (int r = 0; r < 4; r++) {
        if (mode == 0) {
          stage[stftl_stage_at(0, 4 * kq + r, 16 * ct + j, fl, FT, N2)] = re[r];
          stage[stftl_stage_at(1, 4 * kq + r, 16 * ct + j, fl, FT, N2)] = im[r];
        } else {
          stage[stftl_stage_at(0, 4 * kq + r, 16 * ct + j, fl, FT, N2)] = stft_value(re[r], im[r], P.floor, mode);
        }
      }
    }
  }
  __syncthreads();

  for (int i = tid; i < 16 * K2 * FT; i += kStftLongThreads) {
    const int rw = i / FT, fl = i % FT, k1l = rw / K2, k2 = rw % K2, k = 16 * kt + k1l + 64 * k2;
    const long long f = f0 + fl;
    const float v0 = stage[stftl_stage_at(0, k1l, k2, fl, FT, N2)];
    const float v1 = mode == 0 ? stage[stftl_stage_at(1, k1l, k2, fl, FT, N2)] : 0.0f;
    if (f >= P.n_frames) continue;
    const size_t at = (size_t)k * (size_t)P.n_frames + (size_t)f;
    if (mode != 0) out[at] = v0;
    else *reinterpret_cast<f32x2*>(out + 2 * at) = f32x2{v0, v1};
  }
}

// Every plan needs more than the 64 KB a launch can ask for dynamically (Z alone is 32 to 64 KB, the span 8 to 96 KB): a
// static array of all the LDS a workgroup may have, one workgroup a CU, as the other kernels' _big forms.
__global__ __launch_bounds__(kStftLongThreads) void k_clip_stft_long(const pdmp3_mel_desc* __restrict__ descs, const float* __restrict__ tab,
                                                                     pdmp3_stft_long_params P) {
  __shared__ __align__(16) float lds[PDMP3_MEL_LDS_MAX / sizeof(float)];
  const pdmp3_mel_desc d = descs[blockIdx.y];
  const int kt = blockIdx.x & 3;
  const unsigned rest = blockIdx.x >> 2;
  const int ch = (int)(rest % (unsigned)P.channels);
  const long long f0 = (long long)(rest / (unsigned)P.channels) * P.tile;
  if (f0 >= P.n_frames) return;
  if (P.n2 == 32) {
    if (P.tile == 16) stft_long_tile<32, 16>(d, tab, P, ch, kt, f0, lds);
    else stft_long_tile<32, 8>(d, tab, P, ch, kt, f0, lds);
  } else {
    if (P.tile == 8) stft_long_tile<64, 8>(d, tab, P, ch, kt, f0, lds);
    else stft_long_tile<64, 4>(d, tab, P, ch, kt, f0, lds);
  }
}

}  // namespace

hipError_t pdmp3_launch_clip_stft_long(hipStream_t s, const pdmp3_mel_desc* descs, int n_clips, const float* tables,
                                       const pdmp3_stft_long_params* params) {
  const pdmp3_stft_long_params P = *params;
  if (n_clips <= 0 || P.n_frames <= 0) return hipSuccess;
  const bool path = P.n2 == 32 ? (P.tile == 16 || P.tile == 8) : P.n2 == 64 ? (P.tile == 8 || P.tile == 4) : false;
  if (!path || P.n_fft != 64 * P.n2 || P.lds_bytes > PDMP3_MEL_LDS_MAX) return hipErrorInvalidValue;
  const unsigned tiles = (unsigned)((P.n_frames + P.tile - 1) / P.tile);
  const dim3 grid(tiles * 4u * (unsigned)P.channels, (unsigned)n_clips);
  hipLaunchKernelGGL(k_clip_stft_long, grid, dim3(pdmp3::kStftLongThreads), 0, s, descs, tables, P);
  return hipGetLastError();
}
