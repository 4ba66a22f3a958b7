// spectral.hip -- k_clip_spectral: the per-frame spectral descriptors of clips at n_fft 2048 and 4096 (include/pdmp3_bulk.h
// pdmp3_amd_bulk_decode_clips_spectral): rms, zero-crossing rate, spectral centroid, bandwidth, roll-off
// and flatness from section 14's two-stage transform N = 64 N2, the whole spectrum of a tile of frames kept in LDS and reduced
// there, never leaving the CU.  Rows in are k_clip_stft_long's; the transform's index maps, Z's layout and the twiddle step
// are stft_long_core.h's, the plane's layout, the lanes' runs and the descriptors' arithmetic spectral_core.h's.  Launched by
// stream.hip pdmp3_hip_clip_spectral.  A translation unit of its own; the two stages are stft_long_stages.h's, one source for
// this kernel, k_clip_stft_long and k_clip_mel_long, inlined here: a bin's Re and Im are the same binary32 numbers in all three.
#include <hip/hip_runtime.h>

#include "../../include/pdmp3_hip.h"
#include "spectral_core.h"
#include "stft_long_stages.h"

namespace {

using namespace pdmp3;

// the 64 lanes' binary64 sums, every lane the same tree (spectral_core.h)
__device__ __forceinline__ double wave_sum64(double v) {
#pragma unroll
  for (int off = 32; off; off >>= 1) v = v + __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int off = 32; off; off >>= 1) v = v + __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ int wave_min_int(int v) {
#pragma unroll
  for (int off = 32; off; off >>= 1) { const int o = __shfl_xor(v, off, 64); v = o < v ? o : v; }
  return v;
}
// the scan over the lanes' totals, l ascending: -> the lane's prefix; *total: the last value
__device__ __forceinline__ double wave_scan64(double t, int lane, double* total) {
  double p = 0.0, mine = 0.0;
  for (int l = 0; l < 64; l++) {
    if (l == lane) mine = p;
    p = p + __shfl(t, l, 64);
  }
  *total = p;
  return mine;
}

// One workgroup of eight waves per (tile of FT frames, channel, clip); n = N2 n1 + n2, k = k1 + 64 k2.  As k_clip_mel_long
// it takes kt = 0 .. 3 one after the other: a frame's sums run over all bins.
//   0. the tile's span -- (FT - 1) hop + N samples, zeros outside the clip's row -- goes to LDS once, plain, and stays; rows 0
//      and 1 come from it: wave `wave` takes the frames wave, wave + 8, .., its lanes the samples (spec_lane_frame);
//   then for each kt:
//   1. stage 1 as in k_clip_stft_long (stftl_stage1) into Z;
//   2. kt = 0: the Nyquist bin's chain over Z (stftl_nyquist), lane fl of wave 0, its power into column N / 2 of the plane;
//   3. stage 2 as there (stftl_stage2_operand, stftl_stage2_chains); the power of what a lane holds of X goes to the plane at
//      spec_col(bin): the plane stays for all four kt;
//   4. the reductions, wave `wave` the frames wave, wave + 8, ..: pass A (P -> S in place; the sums of S, f S, ln, max(P, amin)),
//      the scan of the magnitudes, pass B (the bandwidth's sum, the first crossing of the cumulative sum); the six values of a
//      frame wait in LDS [row][frame];
//   5. consecutive lanes store consecutive frames of a row.  Frames from F on are not stored.
// Barriers: Z is written in step 1 and read in steps 2 and 3: one barrier behind step 1 and one behind step 3 (before the
// next kt's step 1 writes Z again); the latter also orders the plane's writes before step 4, and one more the results before
// step 5.  Steps 0's results and 4's lie in their own floats: nothing else is shared.
template <int N2, int FT>
__device__ __forceinline__ void spectral_tile(const pdmp3_mel_desc& d, const float* __restrict__ tab, const pdmp3_spectral_params& P, int ch,
                                              long long f0, float* lds) {
  constexpr int N = 64 * N2, NCT = N2 / 32, K = N / 2 + 1;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 15, kq = lane >> 4;
  float* const span = lds;
  float* const z = lds + P.span_floats;
  float* const plane = z + stftl_z_floats(FT, N2);
  float* const res = plane + spec_plane_floats(FT, N);
  const float* const row = reinterpret_cast<const float*>(static_cast<uintptr_t>(d.src)) + (size_t)ch * d.src_chan_stride;
  float* const out = reinterpret_cast<float*>(static_cast<uintptr_t>(d.dst)) + (size_t)ch * d.dst_chan_stride;

  span_load_plain<kSpectralThreads>(span, row, P.n_in, f0, P.hop, d.lead, stftl_span(FT, P.hop, N), tid);
  __syncthreads();

  for (int fl = wave; fl < FT; fl += 8) {
    double sq;
    int cross;
    spec_lane_frame(span + (unsigned)fl * (unsigned)P.hop, N, lane, P.zcr_threshold, &sq, &cross);
    sq = wave_sum64(sq);
    cross = wave_sum_int(cross);
    if (lane == 0) {
      res[0 * FT + fl] = spec_rms(sq, N);
      res[1 * FT + fl] = spec_zcr(cross, N);
    }
  }

  for (int kt = 0; kt < 4; kt++) {
    stftl_stage1<N2, FT>(span, tab, (unsigned)P.hop, kt, wave, j, kq, z);
    __syncthreads();

    if (kt == 0 && tid < FT) {
      float re, im;
      stftl_nyquist(z, tid, N2, &re, &im);
      plane[tid * K + (int)spec_col(N / 2)] = mel_power(re, im);
    }
    {
      const int ct = wave % NCT;
      float b_re[N2 / 2], b_im[N2 / 2];
      stftl_stage2_operand<N2>(tab, ct, j, kq, b_re, b_im);
      for (int fl = wave / NCT; fl < FT; fl += 8 / NCT) {
        f32x4 re, im;
        stftl_stage2_chains<N2>(z, fl, j, kq, b_re, b_im, re, im);
#pragma unroll
        for (int r = 0; r < 4; r++) plane[fl * K + (int)spec_col(16 * kt + 4 * kq + r + 64 * (16 * ct + j))] = mel_power(re[r], im[r]);
      }
    }
    __syncthreads();
  }

  for (int fl = wave; fl < FT; fl += 8) {
    float* const pr = plane + fl * K;
    double ts, tfs, tln, tp, total, tbw;
    int first;
    spec_lane_pass_a(pr, N, lane, P.bin_hz, P.amin, &ts, &tfs, &tln, &tp);
    const double prefix = wave_scan64(ts, lane, &total);
    tfs = wave_sum64(tfs);
    tln = wave_sum64(tln);
    tp = wave_sum64(tp);
    const double c = spec_centroid(tfs, total);
    spec_lane_pass_b(pr, N, lane, P.bin_hz, c, prefix, spec_threshold(P.roll_percent, total), &tbw, &first);
    tbw = wave_sum64(tbw);
    first = wave_min_int(first < 0 ? N : first);
    if (lane == 0) {
      res[2 * FT + fl] = (float)c;
      res[3 * FT + fl] = spec_bandwidth(tbw, total);
      res[4 * FT + fl] = spec_rolloff(first, P.bin_hz);
      res[5 * FT + fl] = spec_flatness(tln, tp, N);
    }
  }
  __syncthreads();

  if (tid < kSpectralRows * FT) {
    const int rw = tid / FT, fl = tid % FT;
    const long long f = f0 + fl;
    if (f < P.n_frames) out[(size_t)rw * (size_t)P.n_frames + (size_t)f] = res[rw * FT + fl];
  }
}

// Every plan needs more than the 64 KB a launch can ask for dynamically: a static array of all the LDS a workgroup may have,
// one workgroup a CU, as k_clip_stft_long.
__global__ __launch_bounds__(kSpectralThreads) void k_clip_spectral(const pdmp3_mel_desc* __restrict__ descs, const float* __restrict__ tab,
                                                                    pdmp3_spectral_params P) {
  __shared__ __align__(16) float lds[PDMP3_MEL_LDS_MAX / sizeof(float)];
  const pdmp3_mel_desc d = descs[blockIdx.y];
  const int ch = (int)(blockIdx.x % (unsigned)P.channels);
  const long long f0 = (long long)(blockIdx.x / (unsigned)P.channels) * P.tile;
  if (f0 >= P.n_frames) return;
  if (P.n2 == 32) spectral_tile<32, 8>(d, tab, P, ch, f0, lds);
  else spectral_tile<64, 4>(d, tab, P, ch, f0, lds);
}

}  // namespace

hipError_t pdmp3_launch_clip_spectral(hipStream_t s, const pdmp3_mel_desc* descs, int n_clips, const float* tables,
                                      const pdmp3_spectral_params* params) {
  const pdmp3_spectral_params P = *params;
  if (n_clips <= 0 || P.n_frames <= 0) return hipSuccess;
  const bool path = (P.n2 == 32 && P.tile == 8) || (P.n2 == 64 && P.tile == 4);
  if (!path || P.n_fft != 64 * P.n2 || P.lds_bytes > PDMP3_MEL_LDS_MAX) return hipErrorInvalidValue;
  const unsigned tiles = (unsigned)((P.n_frames + P.tile - 1) / P.tile);
  const dim3 grid(tiles * (unsigned)P.channels, (unsigned)n_clips);
  hipLaunchKernelGGL(k_clip_spectral, grid, dim3(pdmp3::kSpectralThreads), 0, s, descs, tables, P);
  return hipGetLastError();
}
