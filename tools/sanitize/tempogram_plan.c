/* Sanitizer run of the tempogram call's planning (pdmp3_amd/host/clip_tempogram.c) on the CPU: the check and its refusals one
 * by one, the window and the prior at the edge values and with buffers that are too small, the plan over every window length.
 * A stand-alone program, no GPU:
 *   gcc -O1 -g -fsanitize=address,undefined -Iinclude -Ipdmp3_amd/csrc -o tempogram_plan tools/sanitize/tempogram_plan.c \
 *       pdmp3_amd/host/clip_tempogram.c pdmp3_amd/host/clip_mel_long.c pdmp3_amd/host/clip_mel.c pdmp3_amd/host/clip_stft_long.c \
 *       pdmp3_amd/host/clip_stft.c -lm && ./tempogram_plan
 * (tests/test_clip_tempogram_host.py builds and runs it.) */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../pdmp3_amd/host/bulk_internal.h"

static int fails;
#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "tempogram_plan: line %d: %s\n", __LINE__, #c); fails++; } } while (0)

static pdmp3_amd_tempogram_spec spec_of(int lag, int max_size, int wt, int mode) {
  pdmp3_amd_tempogram_spec s;
  memset(&s, 0, sizeof s);
  s.mel.mel.n_fft = 2048; s.mel.mel.hop = 512; s.mel.mel.n_mels = 128; s.mel.mel.norm = 1; s.mel.mel.floor = 1e-10; s.mel.mel.n_frames = 10;
  s.mel.mel.channels = 1;
  s.lag = lag; s.max_size = max_size; s.win_length = wt; s.out_mode = mode;
  s.start_bpm = 120.0; s.std_bpm = 1.0; s.max_tempo = 320.0;
  return s;
}

static unsigned lds_of(int wt, int frames) {
  const unsigned tiles = (unsigned)(wt + 255) / 256u, ksteps = (unsigned)(wt + 18) / 4u;
  const unsigned reach = 4u * (ksteps + 1u) + 240u + 256u * (tiles - 1u);
  const unsigned ext = 16u + (reach > (unsigned)wt ? reach : (unsigned)wt);
  const unsigned span = (ext + 2u * (ext >> 4) + 3u) & ~3u;
  return ((unsigned)frames * (span + 256u * tiles + 8u) * 4u + 15u) & ~15u;
}

int main(void) {
  pdmp3_amd_tempogram_spec s = spec_of(1, 1, 384, 1);
  int front = -7, back = -7, tiles = -7, ksteps = -7, frames = -7, first = -7;
  unsigned lds = 7;
  EXPECT(pdmp3_amd_tempogram_check(&s, 22050) == 0);
  EXPECT(pdmp3_amd_tempogram_plan(&s, 22050, &front, &back, &tiles, &ksteps, &frames, &lds) == 0);
  EXPECT(front == 193 && back == 191 && tiles == 2 && ksteps == 100 && frames == 8 && lds == lds_of(384, 8));
  EXPECT(pdmp3_amd_tempogram_plan(&s, 22050, NULL, NULL, NULL, NULL, NULL, NULL) == 0);
  EXPECT(pdmp3_amd_tempogram_check(NULL, 22050) == -1 && pdmp3_amd_tempogram_plan(NULL, 22050, NULL, NULL, NULL, NULL, NULL, NULL) == -1);
  EXPECT(pdmp3_amd_tempogram_prior(NULL, 22050, NULL, 0, NULL) == -1);
  EXPECT(pdmp3_amd_tempogram_check(&s, 0) == -1 && pdmp3_amd_tempogram_check(&s, -1) == -1);
  /* the refusals, one by one */
  static const int bad_lag[] = {0, -1, 17, 1 << 30};
  for (unsigned i = 0; i < sizeof bad_lag / sizeof *bad_lag; i++) { s = spec_of(bad_lag[i], 1, 384, 1); EXPECT(pdmp3_amd_tempogram_check(&s, 22050) == -1); }
  static const int bad_ms[] = {0, 2, 8, 10, 11, -1, -3};
  for (unsigned i = 0; i < sizeof bad_ms / sizeof *bad_ms; i++) { s = spec_of(1, bad_ms[i], 384, 1); EXPECT(pdmp3_amd_tempogram_check(&s, 22050) == -1); }
  static const int bad_wt[] = {0, 14, 15, 17, 383, 1025, 1026, 2048, -16, 1 << 30};
  for (unsigned i = 0; i < sizeof bad_wt / sizeof *bad_wt; i++) {
    s = spec_of(1, 1, bad_wt[i], 1);
    EXPECT(pdmp3_amd_tempogram_check(&s, 22050) == -1 && pdmp3_amd_tempogram_window(bad_wt[i], NULL, 0) == -1);
    EXPECT(pdmp3_amd_tempogram_plan(&s, 22050, &front, NULL, NULL, NULL, NULL, NULL) == -1 && front == 193);
  }
  static const double bad_v[] = {0.0, -1.0, NAN, INFINITY, -INFINITY};
  for (unsigned i = 0; i < sizeof bad_v / sizeof *bad_v; i++) {
    s = spec_of(1, 1, 384, 1); s.start_bpm = bad_v[i]; EXPECT(pdmp3_amd_tempogram_check(&s, 22050) == -1);
    s = spec_of(1, 1, 384, 1); s.std_bpm = bad_v[i]; EXPECT(pdmp3_amd_tempogram_check(&s, 22050) == -1);
    s = spec_of(1, 1, 384, 1); s.max_tempo = bad_v[i]; EXPECT(pdmp3_amd_tempogram_check(&s, 22050) == -1);
  }
  s = spec_of(1, 1, 384, 3); EXPECT(pdmp3_amd_tempogram_check(&s, 22050) == -1);
  s = spec_of(1, 1, 384, -1); EXPECT(pdmp3_amd_tempogram_check(&s, 22050) == -1);
  s = spec_of(1, 1, 384, 1); s.mel.mel.n_frames = -1; EXPECT(pdmp3_amd_tempogram_check(&s, 22050) == -1);
  s = spec_of(1, 1, 384, 1); s.mel.mel.n_fft = 1024; EXPECT(pdmp3_amd_tempogram_check(&s, 22050) == -1);
  s = spec_of(1, 1, 384, 1); s.mel.mel.n_mels = 0; EXPECT(pdmp3_amd_tempogram_check(&s, 22050) == -1);
  s = spec_of(1, 1, 384, 1); s.mel.mel.out_mode = 7; EXPECT(pdmp3_amd_tempogram_check(&s, 22050) == 0);      /* (not read) */
  /* rows beyond 31 bits */
  s = spec_of(1, 1, 384, 1); s.mel.mel.n_frames = 0x7fffffffLL / 384 + 1; EXPECT(pdmp3_amd_tempogram_check(&s, 22050) == -1);
  s = spec_of(1, 1, 384, 0); s.mel.mel.n_frames = 0x7fffffffLL / 128; EXPECT(pdmp3_amd_tempogram_check(&s, 22050) == -1);
  s = spec_of(1, 1, 384, 2); s.mel.mel.n_frames = 0x7fffffffffffffffLL; EXPECT(pdmp3_amd_tempogram_check(&s, 22050) == -1);
  /* a prior without an admissible lag, and the narrowest one that has one */
  s = spec_of(1, 1, 16, 2); s.max_tempo = 60.0 * 22050.0 / (512.0 * 16.0); EXPECT(pdmp3_amd_tempogram_check(&s, 22050) == -1);
  s.max_tempo = 60.0 * 22050.0 / (512.0 * 14.5);
  {
    double p[16];
    EXPECT(pdmp3_amd_tempogram_prior(&s, 22050, p, 16, &first) == 0 && first == 15 && isinf(p[14]) && p[15] <= 0.0 && isfinite(p[15]));
    EXPECT(pdmp3_amd_tempogram_prior(&s, 22050, p, 15, &first) == -1);
    EXPECT(pdmp3_amd_tempogram_prior(&s, 22050, NULL, 0, &first) == 0 && first == 15);
  }
  /* the window: the count, a buffer that is too small, the values at the edges */
  {
    float w[1024];
    EXPECT(pdmp3_amd_tempogram_window(384, NULL, 0) == 384 && pdmp3_amd_tempogram_window(384, w, 383) == -1 && pdmp3_amd_tempogram_window(384, NULL, 384) == -1);
    EXPECT(pdmp3_amd_tempogram_window(1024, w, 1024) == 1024 && w[0] == 0.0f && w[512] == 1.0f && w[1] == w[1023]);
    EXPECT(pdmp3_amd_tempogram_window(16, w, 16) == 16 && w[8] == 1.0f && w[4] == 0.5f);
  }
  /* the plan over every window length, lag and mode */
  for (int wt = 16; wt <= 1024; wt += 2) {
    for (int mode = 0; mode <= 2; mode++) {
      s = spec_of(1 + wt % 16, 1 + 2 * (wt % 5), wt, mode);
      s.max_tempo = 1e6;
      EXPECT(pdmp3_amd_tempogram_plan(&s, 22050, &front, &back, &tiles, &ksteps, &frames, &lds) == 0);
      EXPECT(front == s.lag + (mode ? wt / 2 : 0) && back == (mode ? wt / 2 - 1 : 0) && tiles == (wt + 255) / 256 && ksteps == (wt + 18) / 4);
      EXPECT(frames == 8 && lds == lds_of(wt, 8) && lds <= PDMP3_MEL_LDS_MAX);
      double p[1024];
      EXPECT(pdmp3_amd_tempogram_prior(&s, 22050, p, (size_t)wt, &first) == 0 && first == 1 && isinf(p[0]) && isfinite(p[wt - 1]));
    }
  }
  if (fails) return 1;
  printf("tempogram_plan: ok\n");
  return 0;
}
