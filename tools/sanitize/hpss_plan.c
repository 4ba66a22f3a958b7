/* Sanitizer run of the separation call's planning (pdmp3_amd/host/clip_hpss.c) on the CPU: the check and its refusals one by
 * one, with windows at the edges of what is read, and the plan over every pair of kernel sizes and over bad arguments.
 * A stand-alone program, no GPU:
 *   gcc -O1 -g -fsanitize=address,undefined -Iinclude -Ipdmp3_amd/csrc -o hpss_plan tools/sanitize/hpss_plan.c \
 *       pdmp3_amd/host/clip_hpss.c pdmp3_amd/host/clip_stft_long.c -lm && ./hpss_plan
 * (tests/test_clip_hpss_host.py builds and runs it.) */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../pdmp3_amd/host/bulk_internal.h"

static int fails;
#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "hpss_plan: line %d: %s\n", __LINE__, #c); fails++; } } while (0)

static pdmp3_amd_hpss_spec spec_of(int n_fft, int hop) {
  pdmp3_amd_hpss_spec s;
  memset(&s, 0, sizeof s);
  s.n_fft = n_fft; s.hop = hop; s.n_frames = 10; s.channels = 1;
  s.kernel_harm = 31; s.kernel_perc = 31; s.margin_harm = 1.0; s.margin_perc = 1.0; s.power = 2.0;
  return s;
}

int main(void) {
  pdmp3_amd_hpss_spec s = spec_of(2048, 512);
  int v[5] = {-7, -7, -7, -7, -7};
  unsigned lds = 7;
  EXPECT(pdmp3_amd_hpss_check(&s, 22050) == 0);
  EXPECT(pdmp3_amd_hpss_plan(31, 31, &v[0], &v[1], &v[2], &v[3], &v[4], &lds) == 0);
  EXPECT(v[0] == 15 && v[1] == 15 && v[2] == 64 && v[3] == 64 && v[4] == 94 && lds == 94u * 94u * 4u);
  EXPECT(pdmp3_amd_hpss_plan(31, 31, NULL, NULL, NULL, NULL, NULL, NULL) == 0);
  EXPECT(pdmp3_amd_hpss_check(NULL, 22050) == -1);
  EXPECT(pdmp3_amd_hpss_check(&s, 0) == -1 && pdmp3_amd_hpss_check(&s, -1) == -1);
  /* the refusals, one by one */
  static const int bad_n[] = {0, 1, 64, 400, 1024, 2047, 2049, 4095, 4097, 8192, -2048, 1 << 30};
  for (unsigned i = 0; i < sizeof bad_n / sizeof *bad_n; i++) { s = spec_of(bad_n[i], 512); EXPECT(pdmp3_amd_hpss_check(&s, 22050) == -1); }
  static const int bad_hop[] = {0, -1, 2049, 4096, 1 << 30, -(1 << 30)};
  for (unsigned i = 0; i < sizeof bad_hop / sizeof *bad_hop; i++) { s = spec_of(2048, bad_hop[i]); EXPECT(pdmp3_amd_hpss_check(&s, 22050) == -1); }
  static const int bad_kernel[] = {0, 1, 2, 4, 30, 32, 33, 63, -3, -31, 1 << 30, -(1 << 30) - 1};
  for (unsigned i = 0; i < sizeof bad_kernel / sizeof *bad_kernel; i++) {
    s = spec_of(2048, 512); s.kernel_harm = bad_kernel[i]; EXPECT(pdmp3_amd_hpss_check(&s, 22050) == -1);
    s = spec_of(2048, 512); s.kernel_perc = bad_kernel[i]; EXPECT(pdmp3_amd_hpss_check(&s, 22050) == -1);
    EXPECT(pdmp3_amd_hpss_plan(bad_kernel[i], 31, &v[0], &v[1], &v[2], &v[3], &v[4], &lds) == -1);
    EXPECT(pdmp3_amd_hpss_plan(31, bad_kernel[i], &v[0], &v[1], &v[2], &v[3], &v[4], &lds) == -1);
    EXPECT(v[0] == 15 && v[1] == 15 && v[2] == 64 && v[3] == 64 && v[4] == 94 && lds == 94u * 94u * 4u);
  }
  static const double bad_margin[] = {0.0, 0.999999, -1.0, NAN, INFINITY, -INFINITY};
  for (unsigned i = 0; i < sizeof bad_margin / sizeof *bad_margin; i++) {
    s = spec_of(2048, 512); s.margin_harm = bad_margin[i]; EXPECT(pdmp3_amd_hpss_check(&s, 22050) == -1);
    s = spec_of(2048, 512); s.margin_perc = bad_margin[i]; EXPECT(pdmp3_amd_hpss_check(&s, 22050) == -1);
  }
  static const double bad_power[] = {0.0, 0.5, 1.5, 3.0, -1.0, -2.0, NAN, -INFINITY, 1e308};
  for (unsigned i = 0; i < sizeof bad_power / sizeof *bad_power; i++) { s = spec_of(2048, 512); s.power = bad_power[i]; EXPECT(pdmp3_amd_hpss_check(&s, 22050) == -1); }
  static const int bad_mode[] = {-1, 4, 5, 1 << 30, -(1 << 30)};
  for (unsigned i = 0; i < sizeof bad_mode / sizeof *bad_mode; i++) { s = spec_of(2048, 512); s.out_mode = bad_mode[i]; EXPECT(pdmp3_amd_hpss_check(&s, 22050) == -1); }
  s = spec_of(2048, 512); s.n_frames = -1; EXPECT(pdmp3_amd_hpss_check(&s, 22050) == -1);
  s = spec_of(2048, 512); s.win_length = 2049; EXPECT(pdmp3_amd_hpss_check(&s, 22050) == -1);
  s = spec_of(2048, 512); s.win_length = -1; EXPECT(pdmp3_amd_hpss_check(&s, 22050) == -1);
  /* a row beyond 2^31 - 1 floats: the output's 2 e K F, the stage's e K (F + Lh - 1) */
  s = spec_of(2048, 512); s.n_frames = 0x7fffffffLL / (2 * 1025); EXPECT(pdmp3_amd_hpss_check(&s, 22050) == 0);
  s.n_frames++; EXPECT(pdmp3_amd_hpss_check(&s, 22050) == -1);
  s = spec_of(2048, 512); s.out_mode = 2; s.n_frames = 0x7fffffffLL / (4 * 1025); EXPECT(pdmp3_amd_hpss_check(&s, 22050) == 0);
  s.n_frames++; EXPECT(pdmp3_amd_hpss_check(&s, 22050) == -1);
  s = spec_of(4096, 512); s.n_frames = 0x7fffffffLL / (2 * 2049) + 1; EXPECT(pdmp3_amd_hpss_check(&s, 22050) == -1);
  s = spec_of(2048, 512); s.n_frames = 0x7fffffffffffffffLL; EXPECT(pdmp3_amd_hpss_check(&s, 22050) == -1);
  /* the edge values that are accepted */
  s = spec_of(2048, 1); s.kernel_harm = 3; s.kernel_perc = 3; s.margin_harm = 1.7976931348623157e308; s.power = 1.0; s.out_mode = 3; EXPECT(pdmp3_amd_hpss_check(&s, 1) == 0);
  s = spec_of(4096, 4096); s.power = INFINITY; s.margin_perc = 3.5; s.n_frames = 0; s.out_mode = 2; EXPECT(pdmp3_amd_hpss_check(&s, 0x7fffffffL) == 0);
  /* a caller's window: exactly win_length values are read (the allocation ends behind them), a value that is not finite is refused */
  static const int wins[] = {1, 1764, 1920, 2048};
  for (unsigned i = 0; i < sizeof wins / sizeof *wins; i++) {
    float* w = (float*)malloc((size_t)wins[i] * sizeof *w);
    if (!w) return 2;
    for (int n = 0; n < wins[i]; n++) w[n] = 0.25f + (float)(n % 7);
    s = spec_of(2048, 441); s.win_length = wins[i]; s.window = w;
    EXPECT(pdmp3_amd_hpss_check(&s, 22050) == 0);
    w[wins[i] - 1] = NAN;
    EXPECT(pdmp3_amd_hpss_check(&s, 22050) == -1);
    w[wins[i] - 1] = INFINITY;
    EXPECT(pdmp3_amd_hpss_check(&s, 22050) == -1);
    free(w);
  }
  {
    float* w = (float*)malloc(4096 * sizeof *w);
    if (!w) return 2;
    for (int n = 0; n < 4096; n++) w[n] = 1.0f;
    s = spec_of(4096, 1024); s.win_length = 0; s.window = w;             /* (0 = n_fft: all 4096 are read) */
    EXPECT(pdmp3_amd_hpss_check(&s, 48000) == 0);
    w[4095] = NAN;
    EXPECT(pdmp3_amd_hpss_check(&s, 48000) == -1);
    free(w);
  }
  /* the plan over every pair of sizes: one tile, one layout; the widening follows the harmonic kernel */
  for (int lh = 3; lh <= 31; lh += 2)
    for (int lp = 3; lp <= 31; lp += 2) {
      EXPECT(pdmp3_amd_hpss_plan(lh, lp, &v[0], &v[1], &v[2], &v[3], &v[4], &lds) == 0);
      EXPECT(v[0] == lh / 2 && v[1] == lh / 2 && v[2] == 64 && v[3] == 64 && v[4] == 94 && lds == 35344u && lds <= PDMP3_MEL_LDS_MAX);
      s = spec_of(2048, 512); s.kernel_harm = lh; s.kernel_perc = lp; EXPECT(pdmp3_amd_hpss_check(&s, 44100) == 0);
    }
  if (fails) return 1;
  printf("hpss_plan: ok\n");
  return 0;
}
