// mel_long.hip -- k_clip_mel_long: log-mel features of clips at n_fft 2048 and 4096 (include/pdmp3_bulk.h
// pdmp3_amd_bulk_decode_clips_mel_long): section 14's two-stage transform N = 64 N2, the power of every
// bin and the mel filterbank in one workgroup, the spectrum never leaving the CU.  Rows in are k_clip_stft_long's, the layout
// out and the pointwise arithmetic k_clip_mel's (mel_core.h); the transform's index maps, Z's layout and the twiddle step are
// stft_long_core.h's, the order of the bins and the power tile's layout mel_long_core.h's.  Launched by stream.hip
// pdmp3_hip_clip_mel_long.  A translation unit of its own; the two stages are stft_long_stages.h's, one source for this
// kernel and k_clip_stft_long, inlined here.
#include <hip/hip_runtime.h>

#include "../../include/pdmp3_hip.h"
#include "mel_long_core.h"
#include "stft_long_stages.h"

namespace {

using namespace pdmp3;

// One workgroup of eight waves per (tile of FT frames, channel, clip); n = N2 n1 + n2, k = k1 + 64 k2.  A band's sum runs over
// all bins, so the four tiles of k1 cannot go to four workgroups as in k_clip_stft_long (floating-point atomics between them
// would make a value depend on scheduling): this workgroup takes kt = 0 .. 3 one after the other.
//   0. the tile's span -- (FT - 1) hop + N samples, zeros outside the clip's row -- goes to LDS once, plain, and stays;
//   then for each kt:
//   1. stage 1 as in k_clip_stft_long (stftl_stage1): the window product, the 64-term chains, the twiddle, into Z;
//   2. stage 2 as there (stftl_stage2_operand, stftl_stage2_chains): the chains of 2 N2 terms; what a lane holds of X goes
//      through mel_power into the power tile, at the slot mel_long_core.h gives the bin;
//   3. the filterbank: M^T = W^T P^T on the matrix instruction, rows the bands of one tile of 16, columns the frames, k the
//      slots ascending -- A from the operand in memory (its rows are in slot order: 16 consecutive floats a row and band
//      tile), B from the power tile.  A wave takes the band tiles wave and wave + 8 and carries their accumulators in
//      registers from one kt to the next: a band's chain runs over kt ascending, slots ascending, the same for every frame.
//   4. the floor and the logarithm (mel_output); lane (j, kq) holds bands 4 kq + r of frame j: sixteen consecutive lanes
//      store sixteen consecutive frames of one band, plain stores.  Frames from F on are not stored.
// The Nyquist bin is not computed, and stftl_nyquist is not called: pdmp3_amd_mel_long_check requires f_max <= sr / 2 and the
// planner pins the last band's upper edge to f_max, so W[m][N / 2] is exactly 0 in every accepted filterbank
// (tests/test_clip_mel_long_host.py asserts it).
// At FT 8 and 4 the columns j >= FT of step 3 are idle (zeros in, nothing stored): accepted, section 15 has the count.
// Barriers: Z is written in step 1 and read in step 2, the power tile written in step 2 and read in step 3: one barrier
// behind step 1 and one behind step 2 order all four (step 3 of kt lies between step 2's barrier and step 1's of kt + 1).
template <int N2, int FT>
__device__ __forceinline__ void mel_long_tile(const pdmp3_mel_desc& d, const float* __restrict__ tab, const float* __restrict__ op,
                                              const pdmp3_mel_long_params& P, int ch, long long f0, float* lds) {
  constexpr int N = 64 * N2, NCT = N2 / 32, SLOTS = 8 * N2;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 15, kq = lane >> 4;
  const int mp = P.mels16, nbt = mp >> 4;
  float* const span = lds;
  float* const z = lds + P.span_floats;
  float* const pw = z + stftl_z_floats(FT, N2);
  const float* const row = reinterpret_cast<const float*>(static_cast<uintptr_t>(d.src)) + (size_t)ch * d.src_chan_stride;
  float* const out = reinterpret_cast<float*>(static_cast<uintptr_t>(d.dst)) + (size_t)ch * d.dst_chan_stride;

  span_load_plain<kMelLongThreads>(span, row, P.n_in, f0, P.hop, d.lead, stftl_span(FT, P.hop, N), tid);
  __syncthreads();

  f32x4 acc0 = f32x4{0.0f, 0.0f, 0.0f, 0.0f}, acc1 = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  for (int kt = 0; kt < 4; kt++) {
    stftl_stage1<N2, FT>(span, tab, (unsigned)P.hop, kt, wave, j, kq, z);
    __syncthreads();

    {
      const int ct = wave % NCT;
      float b_re[N2 / 2], b_im[N2 / 2];
      stftl_stage2_operand<N2>(tab, ct, j, kq, b_re, b_im);
      for (int fl = wave / NCT; fl < FT; fl += 8 / NCT) {
        f32x4 re, im;
        stftl_stage2_chains<N2>(z, fl, j, kq, b_re, b_im, re, im);
#pragma unroll
        for (int r = 0; r < 4; r++) pw[mell_p_at(fl, mell_slot(4 * kq + r, 16 * ct + j, N2), N2)] = mel_power(re[r], im[r]);
      }
    }
    __syncthreads();

    {
      const float* const wk = op + (size_t)(SLOTS * kt + kq) * (size_t)mp + j;
      const float* const pj = pw + mell_p_at(j < FT ? j : 0, kq, N2);
      if (wave < nbt) {
        const float* const wb = wk + 16 * wave;
#pragma unroll 8
        for (int s = 0; s < SLOTS / 4; s++) acc0 = mfma16(wb[(size_t)(4 * s) * (size_t)mp], j < FT ? pj[4 * s] : 0.0f, acc0);
      }
      if (wave + 8 < nbt) {
        const float* const wb = wk + 16 * (wave + 8);
#pragma unroll 8
        for (int s = 0; s < SLOTS / 4; s++) acc1 = mfma16(wb[(size_t)(4 * s) * (size_t)mp], j < FT ? pj[4 * s] : 0.0f, acc1);
      }
    }
  }

  const long long f = f0 + j;
  if (j < FT && f < P.n_frames) {
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int m0 = 16 * wave + 4 * kq + r, m1 = m0 + 128;
      if (m0 < P.n_mels) out[(size_t)m0 * (size_t)P.n_frames + (size_t)f] = mel_output(acc0[r], P.floor, P.out_mode);
      if (m1 < P.n_mels) out[(size_t)m1 * (size_t)P.n_frames + (size_t)f] = mel_output(acc1[r], P.floor, P.out_mode);
    }
  }
}

// Every plan needs more than the 64 KB a launch can ask for dynamically: a static array of all the LDS a workgroup may have,
// one workgroup a CU, as k_clip_stft_long.
__global__ __launch_bounds__(kMelLongThreads) void k_clip_mel_long(const pdmp3_mel_desc* __restrict__ descs, const float* __restrict__ tab,
                                                                   const float* __restrict__ op, pdmp3_mel_long_params P) {
  __shared__ __align__(16) float lds[PDMP3_MEL_LDS_MAX / sizeof(float)];
  const pdmp3_mel_desc d = descs[blockIdx.y];
  const int ch = (int)(blockIdx.x % (unsigned)P.channels);
  const long long f0 = (long long)(blockIdx.x / (unsigned)P.channels) * P.tile;
  if (f0 >= P.n_frames) return;
  if (P.n2 == 32) {
    if (P.tile == 16) mel_long_tile<32, 16>(d, tab, op, P, ch, f0, lds);
    else mel_long_tile<32, 8>(d, tab, op, P, ch, f0, lds);
  } else {
    if (P.tile == 8) mel_long_tile<64, 8>(d, tab, op, P, ch, f0, lds);
    else mel_long_tile<64, 4>(d, tab, op, P, ch, f0, lds);
  }
}

}  // namespace

hipError_t pdmp3_launch_clip_mel_long(hipStream_t s, const pdmp3_mel_desc* descs, int n_clips, const float* tables, const float* operand,
                                      const pdmp3_mel_long_params* params) {
  const pdmp3_mel_long_params P = *params;
  if (n_clips <= 0 || P.n_frames <= 0) return hipSuccess;
  const bool path = P.n2 == 32 ? (P.tile == 16 || P.tile == 8) : P.n2 == 64 ? (P.tile == 8 || P.tile == 4) : false;
  if (!path || P.n_fft != 64 * P.n2 || P.lds_bytes > PDMP3_MEL_LDS_MAX) return hipErrorInvalidValue;
  const unsigned tiles = (unsigned)((P.n_frames + P.tile - 1) / P.tile);
  const dim3 grid(tiles * (unsigned)P.channels, (unsigned)n_clips);
  hipLaunchKernelGGL(k_clip_mel_long, grid, dim3(pdmp3::kMelLongThreads), 0, s, descs, tables, operand, P);
  return hipGetLastError();
}
