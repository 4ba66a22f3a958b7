/* Sanitizer run of the pitch call's planning (pdmp3_amd/host/clip_pitch.c) on the CPU: the check and its refusals one by one,
 * the lag range at the edges of the quotient rule, the plan over every hop of the shortest, a middle and the longest frame --
 * the LDS inside the limit, the frames a workgroup 8, 4, 2 or 1 and the largest that fits.  A stand-alone program, no GPU:
 *   gcc -O1 -g -fsanitize=address,undefined -Iinclude -Ipdmp3_amd/csrc -o pitch_plan tools/sanitize/pitch_plan.c \
 *       pdmp3_amd/host/clip_pitch.c -lm && ./pitch_plan
 * (tests/test_clip_pitch_host.py builds and runs it.) */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../pdmp3_amd/host/bulk_internal.h"

static int fails;
#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "pitch_plan: line %d: %s\n", __LINE__, #c); fails++; } } while (0)

static pdmp3_amd_pitch_spec spec_of(int N, int W, int H, double fmin, double fmax) {
  pdmp3_amd_pitch_spec s;
  memset(&s, 0, sizeof s);
  s.frame_length = N; s.win_length = W; s.hop = H; s.fmin = fmin; s.fmax = fmax; s.threshold = 0.1; s.n_frames = 10;
  return s;
}

static unsigned lds_of(int N, int W, int H, int tmax, int frames) {
  const unsigned tiles = (unsigned)(tmax + 256) / 256u, ksteps = (unsigned)(W + 18) / 4u;
  const unsigned reach = 4u * (ksteps + 1u) + 240u + 256u * (tiles - 1u), first = (unsigned)(frames - 1) * (unsigned)H;
  const unsigned ext = 16u + first + (reach > (unsigned)N ? reach : (unsigned)N);
  const unsigned span = (ext + 2u * (ext >> 4) + 3u) & ~3u;
  const unsigned doubles = span / 2u + first + (unsigned)N + 1u + 64u * (unsigned)frames + 64u;
  return ((2u * doubles + (unsigned)frames * (256u * tiles + 8u) + 4u * (unsigned)frames) * 4u + 15u) & ~15u;
}

int main(void) {
  pdmp3_amd_pitch_spec s = spec_of(2048, 0, 0, 65.406, 2093.0);
  int tmin = -7, tmax = -7, tiles = -7, frames = -7, ksteps = -7;
  unsigned span = 7, lds = 7;
  EXPECT(pdmp3_amd_pitch_check(&s, 22050) == 0 && pdmp3_amd_pitch_lags(&s, 22050, &tmin, &tmax, &tiles) == 0);
  EXPECT(tmin == 10 && tmax == 338 && tiles == 2);
  EXPECT(pdmp3_amd_pitch_plan(&s, 22050, &frames, &span, &lds, &ksteps) == 0 && frames == 8 && ksteps == 260 && lds == lds_of(2048, 1024, 512, 338, 8));
  EXPECT(pdmp3_amd_pitch_plan(&s, 22050, NULL, NULL, NULL, NULL) == 0 && pdmp3_amd_pitch_lags(&s, 22050, NULL, NULL, NULL) == 0);
  EXPECT(pdmp3_amd_pitch_check(NULL, 22050) == -1 && pdmp3_amd_pitch_lags(NULL, 22050, NULL, NULL, NULL) == -1);
  EXPECT(pdmp3_amd_pitch_plan(NULL, 22050, NULL, NULL, NULL, NULL) == -1);
  EXPECT(pdmp3_amd_pitch_check(&s, 0) == -1 && pdmp3_amd_pitch_check(&s, -1) == -1);
  /* the refusals, one by one; nothing is written */
  static const int bad_n[] = {62, 63, 65, 2047, 2049, 2050, 4096, 0, -64};
  for (unsigned i = 0; i < sizeof bad_n / sizeof *bad_n; i++) { s = spec_of(bad_n[i], 0, 0, 65.406, 2093.0); EXPECT(pdmp3_amd_pitch_check(&s, 22050) == -1); }
  static const int bad_w[] = {-1, 1, 3, 2047, 2048, 4000};
  for (unsigned i = 0; i < sizeof bad_w / sizeof *bad_w; i++) { s = spec_of(2048, bad_w[i], 0, 65.406, 2093.0); EXPECT(pdmp3_amd_pitch_check(&s, 22050) == -1); }
  static const int bad_h[] = {-1, 2049, 1 << 30};
  for (unsigned i = 0; i < sizeof bad_h / sizeof *bad_h; i++) { s = spec_of(2048, 0, bad_h[i], 65.406, 2093.0); EXPECT(pdmp3_amd_pitch_check(&s, 22050) == -1); }
  s = spec_of(2048, 0, 0, 0.0, 2093.0); EXPECT(pdmp3_amd_pitch_check(&s, 22050) == -1);
  s = spec_of(2048, 0, 0, -1.0, 2093.0); EXPECT(pdmp3_amd_pitch_check(&s, 22050) == -1);
  s = spec_of(2048, 0, 0, NAN, 2093.0); EXPECT(pdmp3_amd_pitch_check(&s, 22050) == -1);
  s = spec_of(2048, 0, 0, 65.406, 65.406); EXPECT(pdmp3_amd_pitch_check(&s, 22050) == -1);
  s = spec_of(2048, 0, 0, 65.406, NAN); EXPECT(pdmp3_amd_pitch_check(&s, 22050) == -1);
  s = spec_of(2048, 0, 0, 65.406, 11025.5); EXPECT(pdmp3_amd_pitch_check(&s, 22050) == -1);
  s = spec_of(2048, 0, 0, 65.406, 11025.0); EXPECT(pdmp3_amd_pitch_check(&s, 22050) == 0);
  s = spec_of(64, 60, 0, 100.0, 4000.0); EXPECT(pdmp3_amd_pitch_check(&s, 8000) == 0);           /* tmin 2 < tmax 3 = N - W - 1 */
  s = spec_of(64, 61, 0, 100.0, 4000.0);
  tmin = tmax = -7;
  EXPECT(pdmp3_amd_pitch_lags(&s, 8000, &tmin, &tmax, NULL) == -1 && tmin == -7 && tmax == -7);    /* tmin 2 >= tmax 2 */
  s = spec_of(2048, 0, 0, 65.406, 2093.0);
  s.threshold = 0.0; EXPECT(pdmp3_amd_pitch_check(&s, 22050) == -1);
  s.threshold = 1.0; EXPECT(pdmp3_amd_pitch_check(&s, 22050) == 0);
  s.threshold = 1.0000001; EXPECT(pdmp3_amd_pitch_check(&s, 22050) == -1);
  s.threshold = NAN; EXPECT(pdmp3_amd_pitch_check(&s, 22050) == -1);
  s.threshold = 0.1; s.out_mode = 2; EXPECT(pdmp3_amd_pitch_check(&s, 22050) == -1);
  s.out_mode = -1; EXPECT(pdmp3_amd_pitch_check(&s, 22050) == -1);
  s.out_mode = 1; EXPECT(pdmp3_amd_pitch_check(&s, 22050) == 0);
  s.n_frames = -1; EXPECT(pdmp3_amd_pitch_check(&s, 22050) == -1);
  /* the quotient rule: exact integer ratios pass, a quotient within 1e-9 of an integer that is not one is refused */
  s = spec_of(1024, 0, 0, 100.0, 4000.0);
  EXPECT(pdmp3_amd_pitch_lags(&s, 16000, &tmin, &tmax, &tiles) == 0 && tmin == 4 && tmax == 160 && tiles == 1);
  s = spec_of(1024, 0, 0, 31.25, 2000.0);
  EXPECT(pdmp3_amd_pitch_lags(&s, 8000, &tmin, &tmax, &tiles) == 0 && tmin == 4 && tmax == 256 && tiles == 2);
  s = spec_of(1024, 0, 0, 100.0 * (1.0 + 1e-13), 4000.0);
  EXPECT(pdmp3_amd_pitch_lags(&s, 16000, NULL, NULL, NULL) == -1);
  s = spec_of(1024, 0, 0, 100.0, 4000.0 * (1.0 - 1e-13));
  EXPECT(pdmp3_amd_pitch_lags(&s, 16000, NULL, NULL, NULL) == -1);
  s = spec_of(1024, 0, 0, 100.0 * (1.0 + 1e-8), 4000.0);
  EXPECT(pdmp3_amd_pitch_lags(&s, 16000, &tmin, &tmax, NULL) == 0 && tmax == 160);
  s = spec_of(1024, 0, 0, 100.0 * (1.0 - 1e-8), 4000.0);
  EXPECT(pdmp3_amd_pitch_lags(&s, 16000, &tmin, &tmax, NULL) == 0 && tmax == 161);
  s = spec_of(1024, 0, 0, 1e-300, 4000.0);
  EXPECT(pdmp3_amd_pitch_lags(&s, 16000, NULL, NULL, NULL) == -1);
  /* the plan over every hop */
  static const int Ns[] = {64, 256, 2048};
  for (unsigned i = 0; i < sizeof Ns / sizeof *Ns; i++) {
    const int N = Ns[i];
    for (int H = 1; H <= N; H++) {
      s = spec_of(N, 0, H, 30.0, 4000.0);
      EXPECT(pdmp3_amd_pitch_lags(&s, 8000, &tmin, &tmax, &tiles) == 0 && tmax == (N - N / 2 - 1 < 267 ? N - N / 2 - 1 : 267));
      EXPECT(pdmp3_amd_pitch_plan(&s, 8000, &frames, &span, &lds, &ksteps) == 0);
      EXPECT((frames == 8 || frames == 4 || frames == 2 || frames == 1) && lds <= PDMP3_MEL_LDS_MAX && lds == lds_of(N, N / 2, H, tmax, frames));
      EXPECT(frames == 8 || lds_of(N, N / 2, H, tmax, 2 * frames) > PDMP3_MEL_LDS_MAX);
      EXPECT(ksteps == (N / 2 + 18) / 4 && !(span & 3u));
    }
  }
  if (fails) return 1;
  printf("pitch_plan: ok\n");
  return 0;
}
