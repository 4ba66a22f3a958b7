/* Sanitizer run of the true-peak call's planning (pdmp3_amd/host/clip_r128.c on top of clip_loudness.c) on the CPU: the taps into
 * buffers of exactly the size asked for (AddressSanitizer sees one float too many), the check and its refusals, the plan over
 * rates and the edge lengths -- the first window, the first second window of the range, the last length the range's order
 * statistic takes and the first it does not.  A stand-alone program, no GPU:
 *   gcc -O1 -g -fsanitize=address,undefined -Iinclude -Ipdmp3_amd/csrc -o r128_plan tools/sanitize/r128_plan.c \
 *       pdmp3_amd/host/clip_r128.c pdmp3_amd/host/clip_loudness.c -lm && ./r128_plan
 * (tests/test_clip_r128_host.py builds and runs it.) */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../pdmp3_amd/host/bulk_internal.h"

static int fails;
#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "r128_plan: line %d: %s\n", __LINE__, #c); fails++; } } while (0)

static pdmp3_amd_r128_spec spec_of(long long n_samples, double target, double peak_limit, int limit_true_peak) {
  pdmp3_amd_r128_spec s;
  memset(&s, 0, sizeof s);
  s.loudness.n_samples = n_samples; s.loudness.target = target; s.loudness.peak_limit = peak_limit; s.limit_true_peak = limit_true_peak;
  return s;
}

static void one(long fs) {
  const long long q = (fs + 5) / 10, last = (10LL * PDMP3_R128_MAX_RANGE + 29) * q + q - 1;
  const long long Ts[] = {0, 1, 30 * q - 1, 30 * q, 39 * q + 5, 40 * q - 1, 40 * q, 40 * q + 35, last};
  for (unsigned i = 0; i < sizeof Ts / sizeof *Ts; i++) {
    if (Ts[i] > 0x7fffffffLL - 3) continue;
    int B = 0, chunk = 0, qq = 0;
    unsigned lds = 0;
    long long nc = -1, I = -1, J = -1, Js = -1, Jr = -1, Jsmax = -1;
    EXPECT(pdmp3_amd_r128_plan(fs, Ts[i], &B, &chunk, &lds, &qq, &nc, &I, &J, &Js, &Jr, &Jsmax) == 0);
    EXPECT(pdmp3_amd_r128_plan(fs, Ts[i], NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == 0);
    EXPECT(B == 64 && chunk == 64 && lds == PDMP3_LOUD_LDS_BYTES && qq == q && nc == (Ts[i] + 4095) / 4096 && I == Ts[i] / q);
    EXPECT(J == (I > 3 ? I - 3 : 0) && Js == (I > 29 ? I - 29 : 0) && Jr == (Js + 9) / 10 && Jsmax == Js && Jr <= PDMP3_R128_MAX_RANGE);
    pdmp3_amd_r128_spec s = spec_of(Ts[i], -23.0, 0.89, 1);
    EXPECT(pdmp3_amd_r128_check(&s, fs, 1) == 0 && pdmp3_amd_r128_check(&s, fs, 2) == 0);
  }
  if (last + 1 <= 0x7fffffffLL - 3) {
    long long Jr = -7;
    pdmp3_amd_r128_spec s = spec_of(last + 1, -23.0, 0.89, 1);
    EXPECT(pdmp3_amd_r128_plan(fs, last + 1, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, &Jr, NULL) == -1 && Jr == -7);
    EXPECT(pdmp3_amd_r128_check(&s, fs, 1) == -1);
  }
}

int main(void) {
  static const long rates[] = {8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 96000, 192000};
  for (unsigned i = 0; i < sizeof rates / sizeof *rates; i++) one(rates[i]);
  double* h = (double*)malloc(49 * sizeof *h);
  float* ph = (float*)malloc(3 * PDMP3_R128_TAPS * sizeof *ph);
  EXPECT(pdmp3_amd_r128_taps(h, ph) == 0 && pdmp3_amd_r128_taps(NULL, NULL) == 0 && pdmp3_amd_r128_taps(h, NULL) == 0 && pdmp3_amd_r128_taps(NULL, ph) == 0);
  int nz = 0;
  double sum[4] = {0.0, 0.0, 0.0, 0.0};
  for (int j = 0; j < 49; j++) { nz += h[j] != 0.0; sum[j & 3] += fabs(h[j]); EXPECT(fabs(h[j] - h[48 - j]) < 1e-15); }
  EXPECT(nz == 37 && h[24] == 1.0 && sum[0] == 1.0 && fabs(sum[1] - 1.63118) < 1e-5 && fabs(sum[2] - 1.86418) < 1e-5 && fabs(sum[3] - 1.63118) < 1e-5);
  for (int p = 1; p < 4; p++)
    for (int d = 0; d < PDMP3_R128_TAPS; d++) EXPECT(ph[(p - 1) * PDMP3_R128_TAPS + d] == (float)h[4 * d + p]);
  free(h); free(ph);
  pdmp3_amd_r128_spec s = spec_of(1000, NAN, 0.0, 0);
  EXPECT(pdmp3_amd_r128_check(&s, 48000, 1) == 0 && pdmp3_amd_r128_check(NULL, 48000, 1) == -1);
  EXPECT(pdmp3_amd_r128_check(&s, 7999, 1) == -1 && pdmp3_amd_r128_check(&s, 192001, 1) == -1 && pdmp3_amd_r128_check(&s, 48000, 3) == -1);
  s = spec_of(1000, -23.0, 0.89, 2);
  EXPECT(pdmp3_amd_r128_check(&s, 48000, 1) == -1);
  s = spec_of(1000, -23.0, 0.89, -1);
  EXPECT(pdmp3_amd_r128_check(&s, 48000, 1) == -1);
  s = spec_of(1000, -70.5, 0.89, 1);
  EXPECT(pdmp3_amd_r128_check(&s, 48000, 1) == -1);
  s = spec_of(1000, -23.0, -1.0, 1);
  EXPECT(pdmp3_amd_r128_check(&s, 48000, 1) == -1);
  s = spec_of(-1, -23.0, 0.89, 1);
  EXPECT(pdmp3_amd_r128_check(&s, 48000, 1) == -1);
  EXPECT(pdmp3_amd_r128_plan(48000, -1, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == -1);
  EXPECT(pdmp3_amd_r128_plan(100, 10, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == -1);
  if (fails) return 1;
  printf("r128_plan: ok\n");
  return 0;
}
