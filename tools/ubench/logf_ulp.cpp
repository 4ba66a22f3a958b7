// logf_ulp -- the device's logf and log10f on a file of binary32 values, for the constant c of the log-mel tests' error bound
// (tests/clip_mel_ref.py LOG_C).  It runs the two device functions and nothing of k_clip_mel; the
// comparison with binary64 is the caller's (numpy).  Built like the engine: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off.
//   logf_ulp in.f32 out_ln.f32 out_log10.f32        the values of in.f32
//   logf_ulp - out_x.f32 out_ln.f32 out_log10.f32   a sweep: 4096 values in every binade from 2^-40 to 2^40, written to out_x.f32
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

__global__ void k_logs(const float* x, float* ln, float* l10, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  ln[i] = logf(x[i]);
  l10[i] = log10f(x[i]);
}

#define CHECK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_)); return 1; } } while (0)

static int put(const char* path, const std::vector<float>& v) {
  FILE* f = fopen(path, "wb");
  if (!f || fwrite(v.data(), sizeof(float), v.size(), f) != v.size()) { fprintf(stderr, "cannot write %s\n", path); return 1; }
  fclose(f);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 5) { fprintf(stderr, "usage: logf_ulp in.f32|- out_x.f32 out_ln.f32 out_log10.f32\n"); return 2; }
  std::vector<float> x;
  if (!strcmp(argv[1], "-")) {
    for (int e = -40; e < 40; e++)
      for (int i = 0; i < 4096; i++) x.push_back(ldexpf(1.0f + (float)(i * 2048 + (i * 37) % 2048) / 8388608.0f, e));
  } else {
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 1; }
    float buf[4096];
    size_t got;
    while ((got = fread(buf, sizeof(float), 4096, f)) > 0) x.insert(x.end(), buf, buf + got);
    fclose(f);
  }
  const size_t n = x.size();
  if (!n) return put(argv[2], x) || put(argv[3], x) || put(argv[4], x);
  float *dx, *dl, *d10;
  CHECK(hipMalloc((void**)&dx, n * sizeof(float)));
  CHECK(hipMalloc((void**)&dl, n * sizeof(float)));
  CHECK(hipMalloc((void**)&d10, n * sizeof(float)));
  CHECK(hipMemcpy(dx, x.data(), n * sizeof(float), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_logs, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, dx, dl, d10, n);
  CHECK(hipGetLastError());
  CHECK(hipDeviceSynchronize());
  std::vector<float> ln(n), l10(n);
  CHECK(hipMemcpy(ln.data(), dl, n * sizeof(float), hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(l10.data(), d10, n * sizeof(float), hipMemcpyDeviceToHost));
  return put(argv[2], x) || put(argv[3], ln) || put(argv[4], l10);
}
