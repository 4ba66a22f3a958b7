// What a launch of the granule kernel's SHAPE costs with nothing in it (256 workgroups x 1024 threads x 157 KB of LDS, and the 8-wave
// shape), back-to-back on one stream, HIP events around 200 launches: the floor under k_decode_g's 8.7 us "everything off" time.
//   hipcc --offload-arch=gfx950 -O3 tools/ubench/launch_floor.cpp -o /tmp/launch_floor && /tmp/launch_floor
#include <hip/hip_runtime.h>
#include <cstdio>
extern __shared__ unsigned char smem[];
__global__ void __launch_bounds__(1024) k_empty(int* out) { if (out && threadIdx.x == 0 && blockIdx.x == 0x7fffffff) out[0] = smem[0]; }
// touches its LDS block, reads a granule's records (2 x (128 + 1152) B) and writes its PCM (2304 B) per wave: C2's algorithmic bytes
__global__ void __launch_bounds__(1024) k_touch(const uint4* in, uint4* out) {
  const int w = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  uint4 a = in[(size_t)w * 160 + lane], b = in[(size_t)w * 160 + 64 + lane], c = lane < 32 ? in[(size_t)w * 160 + 128 + lane] : uint4{0, 0, 0, 0};
  reinterpret_cast<uint4*>(smem)[threadIdx.x] = a;
  __syncthreads();
  uint4 s = reinterpret_cast<uint4*>(smem)[threadIdx.x ^ 64];
  s.x ^= b.x ^ c.y;
  out[(size_t)w * 144 + lane] = s; out[(size_t)w * 144 + 64 + lane] = b;
  if (lane < 16) out[(size_t)w * 144 + 128 + lane] = c;
}
// The same body with the 2304 B of PCM per wave stored in the four flavours a kernel can choose from, with and without about
// 12 us of arithmetic in front of the stores (so that all stores of the launch come in a burst at its end, as in k_decode_g):
// what is it worth to write the PCM THROUGH (sc1) instead of leaving it dirty in the L2s until the kernel ends, and what does
// the width of such a store cost?  FORM 0: plain dword (9 per lane), 1: device-scope (sc1) dword, 2: plain 16 bytes (2 1/4 per
// lane), 3: sc1 16 bytes.
template <int FORM, bool SPIN>
__global__ void __launch_bounds__(1024) k_store(const uint4* in, uint4* out) {
  const int w = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  uint4 a = in[(size_t)w * 160 + lane], b = in[(size_t)w * 160 + 64 + lane], c = lane < 32 ? in[(size_t)w * 160 + 128 + lane] : uint4{0, 0, 0, 0};
  reinterpret_cast<uint4*>(smem)[threadIdx.x] = a;
  __syncthreads();
  uint4 s = reinterpret_cast<uint4*>(smem)[threadIdx.x ^ 64];
  s.x ^= b.x ^ c.y;
  if (SPIN) {
    float x = __uint_as_float((s.y & 0xffff) | 0x3f800000u), y = 1.0f;
    const unsigned long long t0 = wall_clock64();          // (100 MHz)
    while (wall_clock64() - t0 < 1200) {
#pragma unroll
      for (int i = 0; i < 64; i++) y = __builtin_fmaf(y, x, -0.25f);
    }
    s.z ^= __float_as_uint(y) & 1u;
  }
  if (FORM == 2) {
    out[(size_t)w * 144 + lane] = s; out[(size_t)w * 144 + 64 + lane] = b;
    if (lane < 16) out[(size_t)w * 144 + 128 + lane] = c;
  } else if (FORM == 3) {
    typedef unsigned v4u __attribute__((vector_size(16)));
    const unsigned long long p = (unsigned long long)(out + (size_t)w * 144);
    const auto rs = __builtin_amdgcn_make_buffer_rsrc((void*)(((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(p >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)p)), (short)0, 2304, 0x00020000);
    __builtin_amdgcn_raw_buffer_store_b128((v4u){s.x, s.y, s.z, s.w}, rs, lane * 16, 0, 16);
    __builtin_amdgcn_raw_buffer_store_b128((v4u){b.x, b.y, b.z, b.w}, rs, 1024 + lane * 16, 0, 16);
    if (lane < 16) __builtin_amdgcn_raw_buffer_store_b128((v4u){c.x, c.y, c.z, c.w}, rs, 2048 + lane * 16, 0, 16);
  } else {
    unsigned* o = reinterpret_cast<unsigned*>(out + (size_t)w * 144);
    const unsigned v[9] = {s.x, s.y, s.z, s.w, b.x, b.y, b.z, b.w, c.x};
#pragma unroll
    for (int q = 0; q < 9; q++) {
      if (FORM == 0) o[64 * q + lane] = v[q];
      else __hip_atomic_store(&o[64 * q + lane], v[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}
template <typename F> static float time_us(F f) {
  hipEvent_t a, b; hipEventCreate(&a); hipEventCreate(&b);
  for (int i = 0; i < 20; i++) f();
  hipDeviceSynchronize();
  hipEventRecord(a, 0);
  for (int i = 0; i < 200; i++) f();
  hipEventRecord(b, 0); hipEventSynchronize(b);
  float ms; hipEventElapsedTime(&ms, a, b);
  return ms * 1e3f / 200;
}
int main() {
  uint4 *in, *out;
  hipMalloc(&in, (size_t)4096 * 160 * 16); hipMalloc(&out, (size_t)4096 * 144 * 16);
  hipMemset(in, 1, (size_t)4096 * 160 * 16);
  hipFuncSetAttribute((const void*)k_empty, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  hipFuncSetAttribute((const void*)k_touch, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  const struct { int wgs, thr, lds; } shapes[] = {{256, 1024, 157 * 1024}, {512, 512, 80 * 1024}, {256, 1024, 16 * 1024}, {4096, 64, 0}, {1, 64, 0}};
  for (auto s : shapes) {
    float e = time_us([&] { hipLaunchKernelGGL(k_empty, dim3(s.wgs), dim3(s.thr), s.lds, 0, (int*)nullptr); });
    float t = s.thr * s.wgs == 262144 ? time_us([&] { hipLaunchKernelGGL(k_touch, dim3(s.wgs), dim3(s.thr), s.lds > 16384 ? s.lds : 16384, 0, in, out); }) : 0.f;
    printf("%4d workgroups x %4d threads, %3d KB LDS: empty %.2f us per launch, records in + PCM out only %.2f us\n", s.wgs, s.thr, s.lds / 1024, e, t);
  }
  // the store flavours, at the granule kernel's shape (256 x 1024 x 157 KB): two runs of 200 launches each
  typedef void (*Kern)(const uint4*, uint4*);
  const struct { const char* name; Kern bare, spin; } forms[] = {
      {"plain dword ", k_store<0, false>, k_store<0, true>}, {"sc1 dword   ", k_store<1, false>, k_store<1, true>},
      {"plain 16 B  ", k_store<2, false>, k_store<2, true>}, {"sc1 16 B    ", k_store<3, false>, k_store<3, true>}};
  for (auto& f : forms) {
    hipFuncSetAttribute((const void*)f.bare, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    hipFuncSetAttribute((const void*)f.spin, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  }
  printf("PCM stores of 2304 B per wave, 256 workgroups x 1024 threads x 157 KB (us per launch, run 1 / run 2)\n");
  for (auto& f : forms) {
    float t[4];
    for (int run = 0; run < 2; run++) {
      t[run] = time_us([&] { hipLaunchKernelGGL(f.bare, dim3(256), dim3(1024), 157 * 1024, 0, in, out); });
      t[2 + run] = time_us([&] { hipLaunchKernelGGL(f.spin, dim3(256), dim3(1024), 157 * 1024, 0, in, out); });
    }
    printf("  %s stores at once %.2f / %.2f   behind 12 us of arithmetic %.2f / %.2f\n", f.name, t[0], t[1], t[2], t[3]);
  }
  return hipDeviceSynchronize() == hipSuccess ? 0 : 1;
}
