// clip.hip -- k_clip_pack: the PCM of a window of clips (include/pdmp3_bulk.h pdmp3_amd_bulk_decode_clips) from the slot's
// frame-major buffer to where each kept frame belongs.  Launched by stream.hip submit_bits for
// pdmp3_hip_stream_submit_bits_clips.  A translation unit of its own, so that the decode, unpack and merge kernels' code is
// what it is without it (as engine_lsf.hip).
#include <hip/hip_runtime.h>

#include "../../include/pdmp3_hip.h"

namespace {

constexpr int kClipThreads = 256;   // a piece is at most one frame place (4608 bytes = 288 vectors of 16 bytes)

// One workgroup per piece: `bytes` bytes from src + piece.src to piece.dst.  The pieces of a window never overlap each
// other's destinations (the host gives every kept frame its own byte range), and no destination overlaps the source.
// Plain loads and stores: 16 bytes a lane where both ends are 16-byte aligned and the count is a multiple of 16 (every
// frame's PCM is 1152, 2304 or 4608 bytes), 2 bytes a lane where they are even, single bytes otherwise (a destination
// that ends inside a sample: the caller's capacity).
__global__ __launch_bounds__(kClipThreads) void k_clip_pack(const pdmp3_clip_piece* __restrict__ pieces, int n_pieces,
                                                             const uint8_t* __restrict__ src) {
  const int p = blockIdx.x;
  if (p >= n_pieces) return;
  const pdmp3_clip_piece q = pieces[p];
  const uint8_t* s = src + q.src;
  uint8_t* d = reinterpret_cast<uint8_t*>(static_cast<uintptr_t>(q.dst));
  const unsigned nb = q.bytes;
  const uintptr_t al = reinterpret_cast<uintptr_t>(s) | reinterpret_cast<uintptr_t>(d) | nb;
  if ((al & 15) == 0) {
    const uint4* s4 = reinterpret_cast<const uint4*>(s);
    uint4* d4 = reinterpret_cast<uint4*>(d);
    for (unsigned i = threadIdx.x; i < (nb >> 4); i += kClipThreads) d4[i] = s4[i];
  } else if ((al & 1) == 0) {
    const uint16_t* s2 = reinterpret_cast<const uint16_t*>(s);
    uint16_t* d2 = reinterpret_cast<uint16_t*>(d);
    for (unsigned i = threadIdx.x; i < (nb >> 1); i += kClipThreads) d2[i] = s2[i];
  } else {
    for (unsigned i = threadIdx.x; i < nb; i += kClipThreads) d[i] = s[i];
  }
}

}  // namespace

hipError_t pdmp3_launch_clip_pack(hipStream_t s, const pdmp3_clip_piece* pieces, int n_pieces, const void* src) {
  if (n_pieces <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_clip_pack, dim3((unsigned)n_pieces), dim3(kClipThreads), 0, s, pieces, n_pieces,
                     static_cast<const uint8_t*>(src));
  return hipGetLastError();
}
