/* Sanitizer run of the loudness call's planning (pdmp3_amd/host/clip_loudness.c) on the CPU: the check and its refusals, the
 * coefficients and the tables into buffers of exactly the size asked for (AddressSanitizer sees one float too many), the plan
 * over rates and lengths.  A stand-alone program, no GPU:
 *   gcc -O1 -g -fsanitize=address,undefined -Iinclude -Ipdmp3_amd/csrc -o loudness_plan tools/sanitize/loudness_plan.c \
 *       pdmp3_amd/host/clip_loudness.c -lm && ./loudness_plan
 * (tests/test_clip_loudness_host.py builds and runs it.) */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../pdmp3_amd/host/bulk_internal.h"

static int fails;
#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "loudness_plan: line %d: %s\n", __LINE__, #c); fails++; } } while (0)

static pdmp3_amd_loudness_spec spec_of(double target, double peak_limit, int dual_mono) {
  pdmp3_amd_loudness_spec s;
  memset(&s, 0, sizeof s);
  s.n_samples = 1000; s.target = target; s.peak_limit = peak_limit; s.dual_mono = dual_mono;
  return s;
}

static void one(long fs) {
  double* coef = (double*)malloc(12 * sizeof *coef);
  float* Hm = (float*)malloc(64 * 64 * sizeof *Hm);
  float* O = (float*)malloc(64 * 4 * sizeof *O);
  double* Phi = (double*)malloc(16 * sizeof *Phi);
  double* R = (double*)malloc(4 * 64 * sizeof *R);
  double* pows = (double*)malloc(PDMP3_LOUD_POWS * 16 * sizeof *pows);
  EXPECT(pdmp3_amd_loudness_coefficients(fs, coef) == 0);
  EXPECT(coef[3] == 1.0 && coef[9] == 1.0 && coef[6] == 1.0 && coef[7] == -2.0 && coef[8] == 1.0);
  EXPECT(pdmp3_amd_loudness_tables(fs, Hm, O, Phi, R, pows) == 0);
  EXPECT(pdmp3_amd_loudness_tables(fs, NULL, NULL, NULL, NULL, NULL) == 0);
  EXPECT(Hm[0] == (float)coef[0] && Hm[1] == 0.0f && Hm[63 * 64 + 63] == Hm[0]);
  for (int i = 0; i < 16; i++) EXPECT(pows[16 + i] == Phi[i] && isfinite(pows[(PDMP3_LOUD_POWS - 1) * 16 + i]));
  for (int i = 0; i < 4 * 64; i++) EXPECT(isfinite(R[i]) && isfinite(O[i]));
  const long long Ts[] = {0, 1, 4095, 4096, 4097, 123457, 0x7fffffffLL - 3};
  for (unsigned i = 0; i < sizeof Ts / sizeof *Ts; i++) {
    int B = 0, chunk = 0, q = 0;
    unsigned lds = 0;
    long long nc = -1, I = -1, J = -1;
    EXPECT(pdmp3_amd_loudness_plan(fs, Ts[i], &B, &chunk, &lds, &q, &nc, &I, &J) == 0);
    EXPECT(pdmp3_amd_loudness_plan(fs, Ts[i], NULL, NULL, NULL, NULL, NULL, NULL, NULL) == 0);
    EXPECT(B == 64 && chunk == 64 && lds == PDMP3_LOUD_LDS_BYTES && q == (fs + 5) / 10);
    EXPECT(nc == (Ts[i] + 4095) / 4096 && I == Ts[i] / q && J == (I > 3 ? I - 3 : 0));
  }
  free(coef); free(Hm); free(O); free(Phi); free(R); free(pows);
}

int main(void) {
  static const long rates[] = {8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 96000, 192000};
  for (unsigned i = 0; i < sizeof rates / sizeof *rates; i++) one(rates[i]);
  pdmp3_amd_loudness_spec s = spec_of(NAN, 0.0, 0);
  EXPECT(pdmp3_amd_loudness_check(&s, 48000, 1) == 0 && pdmp3_amd_loudness_check(&s, 48000, 2) == 0);
  EXPECT(pdmp3_amd_loudness_check(NULL, 48000, 1) == -1 && pdmp3_amd_loudness_check(&s, 7999, 1) == -1 && pdmp3_amd_loudness_check(&s, 192001, 1) == -1);
  EXPECT(pdmp3_amd_loudness_check(&s, 48000, 0) == -1 && pdmp3_amd_loudness_check(&s, 48000, 3) == -1);
  s = spec_of(-70.0, 0.5, 1);
  EXPECT(pdmp3_amd_loudness_check(&s, 8000, 1) == 0 && pdmp3_amd_loudness_check(&s, 8000, 2) == -1);
  const double bad_targets[] = {-70.5, 0.5, INFINITY, -INFINITY};
  for (unsigned i = 0; i < 4; i++) { s = spec_of(bad_targets[i], 0.0, 0); EXPECT(pdmp3_amd_loudness_check(&s, 48000, 1) == -1); }
  const double bad_limits[] = {-1.0, INFINITY, NAN};
  for (unsigned i = 0; i < 3; i++) { s = spec_of(-14.0, bad_limits[i], 0); EXPECT(pdmp3_amd_loudness_check(&s, 48000, 1) == -1); }
  s = spec_of(-14.0, 0.0, 2);
  EXPECT(pdmp3_amd_loudness_check(&s, 48000, 1) == -1);
  double c[12];
  EXPECT(pdmp3_amd_loudness_coefficients(7999, c) == -1 && pdmp3_amd_loudness_coefficients(48000, NULL) == -1);
  EXPECT(pdmp3_amd_loudness_tables(192001, NULL, NULL, NULL, NULL, NULL) == -1);
  EXPECT(pdmp3_amd_loudness_plan(48000, -1, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == -1);
  EXPECT(pdmp3_amd_loudness_plan(48000, 0x7fffffffLL - 2, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == -1);
  EXPECT(pdmp3_amd_loudness_plan(100, 10, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == -1);
  if (fails) return 1;
  printf("loudness_plan: ok\n");
  return 0;
}
