/* Sanitizer run of the spectral call's planning (pdmp3_amd/host/clip_spectral.c) on the CPU: the check and its refusals one by
 * one, with windows at the edges of what is read, and the plan over every hop of both lengths and over bad arguments.
 * A stand-alone program, no GPU:
 *   gcc -O1 -g -fsanitize=address,undefined -Iinclude -Ipdmp3_amd/csrc -o spectral_plan tools/sanitize/spectral_plan.c \
 *       pdmp3_amd/host/clip_spectral.c pdmp3_amd/host/clip_stft_long.c -lm && ./spectral_plan
 * (tests/test_clip_spectral_host.py builds and runs it.) */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../pdmp3_amd/host/bulk_internal.h"

static int fails;
#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "spectral_plan: line %d: %s\n", __LINE__, #c); fails++; } } while (0)

static pdmp3_amd_spectral_spec spec_of(int n_fft, int hop) {
  pdmp3_amd_spectral_spec s;
  memset(&s, 0, sizeof s);
  s.n_fft = n_fft; s.hop = hop; s.n_frames = 10; s.channels = 1;
  s.roll_percent = 0.85; s.amin = 1e-10; s.zcr_threshold = 1e-10;
  return s;
}

static unsigned lds_of(int n_fft, int hop) {
  const unsigned tile = n_fft == 2048 ? 8u : 4u, n2 = (unsigned)n_fft / 64u;
  const unsigned span = ((tile - 1u) * (unsigned)hop + (unsigned)n_fft + 3u) & ~3u;
  return ((span + tile * n2 * 32u + tile * ((unsigned)n_fft / 2u + 1u) + 8u * tile + 3u) & ~3u) * 4u;
}

int main(void) {
  pdmp3_amd_spectral_spec s = spec_of(2048, 512);
  int tile = -7, pad = -7;
  unsigned lds = 7;
  EXPECT(pdmp3_amd_spectral_check(&s, 22050) == 0);
  EXPECT(pdmp3_amd_spectral_plan(2048, 512, &tile, &pad, &lds) == 0 && tile == 8 && pad == 0 && lds == 88352u);
  EXPECT(pdmp3_amd_spectral_plan(2048, 512, NULL, NULL, NULL) == 0);
  EXPECT(pdmp3_amd_spectral_check(NULL, 22050) == -1);
  EXPECT(pdmp3_amd_spectral_check(&s, 0) == -1 && pdmp3_amd_spectral_check(&s, -1) == -1);
  /* the refusals, one by one */
  static const int bad_n[] = {0, 1, 64, 400, 1024, 2047, 2049, 4095, 4097, 8192, -2048, 1 << 30};
  for (unsigned i = 0; i < sizeof bad_n / sizeof *bad_n; i++) {
    s = spec_of(bad_n[i], 512);
    EXPECT(pdmp3_amd_spectral_check(&s, 22050) == -1);
    EXPECT(pdmp3_amd_spectral_plan(bad_n[i], 512, &tile, &pad, &lds) == -1 && tile == 8 && pad == 0 && lds == 88352u);
  }
  static const int bad_hop[] = {0, -1, 2049, 4096, 1 << 30, -(1 << 30)};
  for (unsigned i = 0; i < sizeof bad_hop / sizeof *bad_hop; i++) {
    s = spec_of(2048, bad_hop[i]);
    EXPECT(pdmp3_amd_spectral_check(&s, 22050) == -1 && pdmp3_amd_spectral_plan(2048, bad_hop[i], &tile, NULL, &lds) == -1 && tile == 8 && lds == 88352u);
  }
  s = spec_of(4096, 4097); EXPECT(pdmp3_amd_spectral_check(&s, 48000) == -1 && pdmp3_amd_spectral_plan(4096, 4097, NULL, NULL, NULL) == -1);
  static const double bad_roll[] = {0.0, 1.0, -0.5, 1.5, NAN, INFINITY, -INFINITY};
  for (unsigned i = 0; i < sizeof bad_roll / sizeof *bad_roll; i++) { s = spec_of(2048, 512); s.roll_percent = bad_roll[i]; EXPECT(pdmp3_amd_spectral_check(&s, 22050) == -1); }
  static const double bad_amin[] = {0.0, -1e-10, NAN, INFINITY, -INFINITY, 1e-46, 1e39};
  for (unsigned i = 0; i < sizeof bad_amin / sizeof *bad_amin; i++) { s = spec_of(2048, 512); s.amin = bad_amin[i]; EXPECT(pdmp3_amd_spectral_check(&s, 22050) == -1); }
  static const double bad_zt[] = {-1e-10, -1.0, NAN, INFINITY, -INFINITY, 1e39};
  for (unsigned i = 0; i < sizeof bad_zt / sizeof *bad_zt; i++) { s = spec_of(2048, 512); s.zcr_threshold = bad_zt[i]; EXPECT(pdmp3_amd_spectral_check(&s, 22050) == -1); }
  s = spec_of(2048, 512); s.n_frames = -1; EXPECT(pdmp3_amd_spectral_check(&s, 22050) == -1);
  s = spec_of(2048, 512); s.win_length = 2049; EXPECT(pdmp3_amd_spectral_check(&s, 22050) == -1);
  s = spec_of(2048, 512); s.win_length = -1; EXPECT(pdmp3_amd_spectral_check(&s, 22050) == -1);
  /* the edge values that are accepted */
  s = spec_of(2048, 1); s.roll_percent = 1e-300; s.amin = 1.17549435e-38; s.zcr_threshold = 0.0; EXPECT(pdmp3_amd_spectral_check(&s, 1) == 0);
  s = spec_of(4096, 4096); s.roll_percent = 0.9999999999; s.amin = 3e38; s.zcr_threshold = 3e38; s.n_frames = 0; EXPECT(pdmp3_amd_spectral_check(&s, 0x7fffffffL) == 0);
  /* a caller's window: exactly win_length values are read (the allocation ends behind them), a value that is not finite is refused */
  static const int wins[] = {1, 1764, 1920, 2048};
  for (unsigned i = 0; i < sizeof wins / sizeof *wins; i++) {
    float* w = (float*)malloc((size_t)wins[i] * sizeof *w);
    if (!w) return 2;
    for (int n = 0; n < wins[i]; n++) w[n] = 0.25f + (float)(n % 7);
    s = spec_of(2048, 441); s.win_length = wins[i]; s.window = w;
    EXPECT(pdmp3_amd_spectral_check(&s, 22050) == 0);
    w[wins[i] - 1] = NAN;
    EXPECT(pdmp3_amd_spectral_check(&s, 22050) == -1);
    w[wins[i] - 1] = INFINITY;
    EXPECT(pdmp3_amd_spectral_check(&s, 22050) == -1);
    free(w);
  }
  {
    float* w = (float*)malloc(4096 * sizeof *w);
    if (!w) return 2;
    for (int n = 0; n < 4096; n++) w[n] = 1.0f;
    s = spec_of(4096, 1024); s.win_length = 0; s.window = w;             /* (0 = n_fft: all 4096 are read) */
    EXPECT(pdmp3_amd_spectral_check(&s, 48000) == 0);
    w[4095] = NAN;
    EXPECT(pdmp3_amd_spectral_check(&s, 48000) == -1);
    free(w);
  }
  /* the plan over every hop of both lengths */
  for (int n_fft = 2048; n_fft <= 4096; n_fft *= 2) {
    unsigned most = 0;
    for (int hop = 1; hop <= n_fft; hop++) {
      EXPECT(pdmp3_amd_spectral_plan(n_fft, hop, &tile, &pad, &lds) == 0);
      EXPECT(tile == (n_fft == 2048 ? 8 : 4) && pad == 0 && lds == lds_of(n_fft, hop) && lds > 64u * 1024u && lds <= PDMP3_MEL_LDS_MAX && lds % 16u == 0);
      if (lds > most) most = lds;
    }
    EXPECT(most == lds_of(n_fft, n_fft) && most == (n_fft == 2048 ? 131360u : 131216u));
  }
  if (fails) return 1;
  printf("spectral_plan: ok\n");
  return 0;
}
