// sqrtf_ulp -- is the device's sqrtf correctly rounded?  For mode 1 of the short-time Fourier transform's error bound
// (tests/clip_stft_ref.py), which counts the square root as one rounding.  It runs the device function
// as the engine's build compiles it and nothing of k_clip_stft, on EVERY positive finite binary32 value, subnormals included.
// The test is exact: r = sqrtf(x) is the correctly rounded root iff m_lo^2 < x < m_hi^2 with m_lo, m_hi the midpoints between
// r and its two neighbours -- 25-bit numbers whose squares binary64 holds exactly (a root is never a midpoint itself).
// Built like the engine: hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off sqrtf_ulp.cpp -o sqrtf_ulp
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

__global__ void k_sqrt(unsigned long long* bad, unsigned* first_bad) {
  const uint32_t last = 0x7f7fffffu;                                    // the largest finite value
  unsigned long long mine = 0;
  for (uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x + 1; u <= last; u += (uint64_t)gridDim.x * blockDim.x) {
    const float x = __uint_as_float((uint32_t)u);
    const float r = sqrtf(x);
    const double lo = 0.5 * ((double)r + (double)nextafterf(r, 0.0f)), hi = 0.5 * ((double)r + (double)nextafterf(r, INFINITY));
    if (!(lo * lo < (double)x && (double)x < hi * hi)) { mine++; atomicMin(first_bad, (unsigned)u); }
  }
  if (mine) atomicAdd(bad, mine);
}

#define CHECK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_)); return 1; } } while (0)

int main() {
  unsigned long long* d_bad;
  unsigned* d_first;
  unsigned long long bad = 0;
  unsigned first = 0xffffffffu;
  CHECK(hipMalloc((void**)&d_bad, sizeof bad));
  CHECK(hipMalloc((void**)&d_first, sizeof first));
  CHECK(hipMemcpy(d_bad, &bad, sizeof bad, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(d_first, &first, sizeof first, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_sqrt, dim3(4096), dim3(256), 0, 0, d_bad, d_first);
  CHECK(hipGetLastError());
  CHECK(hipDeviceSynchronize());
  CHECK(hipMemcpy(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(&first, d_first, sizeof first, hipMemcpyDeviceToHost));
  printf("sqrtf on all %u positive finite binary32 values: %llu not correctly rounded", 0x7f7fffffu, bad);
  if (bad) printf(" (the first: bits 0x%08x)", first);
  printf("\n");
  return bad ? 3 : 0;
}
