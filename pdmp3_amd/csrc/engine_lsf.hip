// engine_lsf.hip -- the LSF instantiations of the device Huffman stage's kernels (unpack_kernels.h), launched by
// engine.hip unpack_window_head / _carry (stream.hip submit_bits) for windows of MPEG-2 LSF / MPEG-2.5 frames (pdmp3_hip_stream_set_lsf).  A translation unit of
// their own, so that the MPEG-1 kernels' code is what it is without them (unpack_kernels.h).
#include <hip/hip_runtime.h>

#include "unpack_kernels.h"

using namespace pdmp3;

hipError_t pdmp3_launch_unpack_lsf(dim3 grid, hipStream_t s, const UnpackTables* tabs, const pdmp3_frame_bits* bits, const uint8_t* res,
                                   int n_frames, int16_t* spectra, GcRaw* raw, int tab_n16, unsigned long long* prof) {
  hipLaunchKernelGGL(k_unpack<true>, grid, dim3(kUnpackThreads), 0, s, tabs, bits, res, n_frames, spectra, raw, tab_n16, prof);
  return hipGetLastError();
}

hipError_t pdmp3_launch_merge_apply_lsf(dim3 grid, hipStream_t s, const GcRaw* raw, const pdmp3_frame_bits* bits, int n_frames, const uint32_t* outc,
                                        const uint32_t* sup, const uint16_t* state_in, uint16_t* state_out, pdmp3_gc_side* side) {
  hipLaunchKernelGGL(k_merge_apply<true>, grid, dim3(kMergeLanes), 0, s, raw, bits, n_frames, outc, sup, state_in, state_out, side);
  return hipGetLastError();
}
