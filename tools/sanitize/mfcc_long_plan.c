/* Sanitizer run of the long MFCC call's planning (pdmp3_amd/host/clip_mfcc_long.c) on the CPU: the check and its refusals one by
 * one, the DCT table and the delta taps with buffers that are too small, and the plan over every (n_mels, n_mfcc, width, deltas)
 * edge.  A stand-alone program, no GPU:
 *   gcc -O1 -g -fsanitize=address,undefined -Iinclude -Ipdmp3_amd/csrc -o mfcc_long_plan tools/sanitize/mfcc_long_plan.c \
 *       pdmp3_amd/host/clip_mfcc_long.c pdmp3_amd/host/clip_mel_long.c pdmp3_amd/host/clip_mel.c pdmp3_amd/host/clip_stft_long.c \
 *       pdmp3_amd/host/clip_stft.c -lm && ./mfcc_long_plan
 * (tests/test_clip_mfcc_long_host.py builds and runs it.) */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../pdmp3_amd/host/bulk_internal.h"

static int fails;
#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "mfcc_long_plan: line %d: %s\n", __LINE__, #c); fails++; } } while (0)

static pdmp3_amd_mfcc_long_spec spec_of(int n_mels, int n_mfcc, int deltas, int width) {
  pdmp3_amd_mfcc_long_spec s;
  memset(&s, 0, sizeof s);
  s.mel.mel.n_fft = 2048; s.mel.mel.hop = 512; s.mel.mel.n_mels = n_mels; s.mel.mel.n_frames = 10; s.mel.mel.channels = 1;
  s.mel.mel.floor = 1e-10;
  s.top_db = 80.0; s.n_mfcc = n_mfcc; s.deltas = deltas; s.delta_width = width;
  return s;
}
#define REFUSED(change) do { s = spec_of(128, 20, 2, 9); change; EXPECT(pdmp3_amd_mfcc_long_check(&s, 22050) == -1); } while (0)
#define ACCEPTED(change) do { s = spec_of(128, 20, 2, 9); change; EXPECT(pdmp3_amd_mfcc_long_check(&s, 22050) == 0); } while (0)

int main(void) {
  pdmp3_amd_mfcc_long_spec s = spec_of(128, 20, 2, 9);
  EXPECT(pdmp3_amd_mfcc_long_check(&s, 22050) == 0);
  EXPECT(pdmp3_amd_mfcc_long_check(NULL, 22050) == -1);
  EXPECT(pdmp3_amd_mfcc_long_check(&s, 0) == -1 && pdmp3_amd_mfcc_long_check(&s, -1) == -1);
  /* the refusals, one by one: the log-mel's */
  REFUSED(s.mel.mel.n_fft = 1024); REFUSED(s.mel.mel.n_fft = 8192); REFUSED(s.mel.mel.hop = 0); REFUSED(s.mel.mel.hop = 2049);
  REFUSED(s.mel.mel.n_mels = 0); REFUSED(s.mel.mel.n_mels = 257); REFUSED(s.mel.mel.floor = 0.0); REFUSED(s.mel.mel.floor = NAN);
  REFUSED(s.mel.mel.f_max = 12000.0); REFUSED(s.mel.mel.f_min = -1.0); REFUSED(s.mel.mel.n_frames = -1);
  REFUSED(s.mel.win_length = 2049); REFUSED(s.mel.win_length = -1);
  ACCEPTED(s.mel.mel.out_mode = 7);                      /* (not read) */
  /* top_db */
  REFUSED(s.top_db = NAN); REFUSED(s.top_db = INFINITY);
  ACCEPTED(s.top_db = 0.0); ACCEPTED(s.top_db = -1.0); ACCEPTED(s.top_db = -INFINITY); ACCEPTED(s.top_db = 1e300);
  /* n_mfcc, lifter, deltas, delta_width, out_mode */
  REFUSED(s.n_mfcc = 0); REFUSED(s.n_mfcc = -1); REFUSED(s.n_mfcc = 129); REFUSED(s.n_mfcc = 1 << 30);
  REFUSED(s.mel.mel.n_mels = 19);                        /* (n_mfcc 20 above the bands) */
  ACCEPTED(s.n_mfcc = 128); ACCEPTED(s.n_mfcc = 1); ACCEPTED(s.mel.mel.n_mels = 20);
  REFUSED((s.mel.mel.n_mels = 256, s.n_mfcc = 129)); ACCEPTED((s.mel.mel.n_mels = 256, s.n_mfcc = 128));
  REFUSED(s.lifter = -1.0); REFUSED(s.lifter = NAN); REFUSED(s.lifter = INFINITY); ACCEPTED(s.lifter = 22.0); ACCEPTED(s.lifter = 0.5);
  REFUSED(s.deltas = -1); REFUSED(s.deltas = 3); REFUSED(s.deltas = 1 << 30);
  static const int bad_w[] = {0, 1, 2, 4, 8, 16, 18, 19, -3, -9, 1 << 30, -(1 << 30) - 1};
  for (unsigned i = 0; i < sizeof bad_w / sizeof *bad_w; i++) {
    REFUSED(s.delta_width = bad_w[i]);
    REFUSED((s.deltas = 1, s.delta_width = bad_w[i]));
    ACCEPTED((s.deltas = 0, s.delta_width = bad_w[i]));    /* (read with deltas > 0 only) */
  }
  REFUSED(s.out_mode = 2); REFUSED(s.out_mode = -1); REFUSED(s.out_mode = 1 << 30);
  /* the dB mode reads none of the cepstral fields */
  ACCEPTED((s.out_mode = 1, s.n_mfcc = 0, s.lifter = NAN, s.deltas = 9, s.delta_width = 4));
  REFUSED((s.out_mode = 1, s.top_db = NAN));
  /* a row beyond 2^31 - 1 floats: the output's (1 + deltas) n_mfcc F, n_mels F; the stage's n_mels (F + 2 h) */
  ACCEPTED((s.deltas = 0, s.n_mfcc = 1, s.mel.mel.n_frames = 0x7fffffffLL / 128));
  REFUSED((s.deltas = 0, s.n_mfcc = 1, s.mel.mel.n_frames = 0x7fffffffLL / 128 + 1));
  ACCEPTED((s.n_mfcc = 1, s.mel.mel.n_frames = 0x7fffffffLL / 128 - 8));
  REFUSED((s.n_mfcc = 1, s.mel.mel.n_frames = 0x7fffffffLL / 128 - 7));
  ACCEPTED((s.mel.mel.n_mels = 256, s.n_mfcc = 128, s.mel.mel.n_frames = 0x7fffffffLL / 384));
  REFUSED((s.mel.mel.n_mels = 256, s.n_mfcc = 128, s.mel.mel.n_frames = 0x7fffffffLL / 384 + 1));
  ACCEPTED((s.out_mode = 1, s.mel.mel.n_frames = 0x7fffffffLL / 128));
  REFUSED((s.out_mode = 1, s.mel.mel.n_frames = 0x7fffffffLL / 128 + 1));
  REFUSED(s.mel.mel.n_frames = 0x7fffffffffffffffLL);
  /* a caller's window: exactly win_length values are read */
  {
    float* w = (float*)malloc(1764 * sizeof *w);
    if (!w) return 2;
    for (int n = 0; n < 1764; n++) w[n] = 0.5f;
    ACCEPTED((s.mel.win_length = 1764, s.mel.window = w));
    w[1763] = NAN;
    REFUSED((s.mel.win_length = 1764, s.mel.window = w));
    free(w);
  }
  /* the table: every shape's count, a buffer that is too small receives exactly cap floats */
  static const int mels[] = {1, 15, 16, 17, 20, 40, 128, 255, 256};
  for (unsigned i = 0; i < sizeof mels / sizeof *mels; i++) {
    const int nm = mels[i];
    const int ceps[] = {1, nm < 13 ? nm : 13, nm < 128 ? nm : 128};
    for (int c = 0; c < 3; c++) {
      int rows = -7, cols = -7;
      const long long count = pdmp3_amd_mfcc_long_dct_table(nm, ceps[c], c ? 22.0 : 0.0, NULL, 0, &rows, &cols);
      EXPECT(count == (long long)rows * cols && rows == ((ceps[c] + 15) & ~15) && cols == ((nm + 15) & ~15));
      float* t = (float*)malloc((size_t)count * sizeof *t);
      float* part = (float*)malloc(5 * sizeof *part);
      if (!t || !part) return 2;
      EXPECT(pdmp3_amd_mfcc_long_dct_table(nm, ceps[c], c ? 22.0 : 0.0, t, (size_t)count, NULL, NULL) == count);
      EXPECT(pdmp3_amd_mfcc_long_dct_table(nm, ceps[c], c ? 22.0 : 0.0, part, 5, NULL, NULL) == count);
      EXPECT(memcmp(t, part, 5 * sizeof *t) == 0);
      EXPECT(t[0] > 0.0f && t[count - 1] == (((nm & 15) || (ceps[c] & 15)) ? 0.0f : t[count - 1]));
      free(t); free(part);
    }
  }
  EXPECT(pdmp3_amd_mfcc_long_dct_table(0, 1, 0.0, NULL, 0, NULL, NULL) == -1);
  EXPECT(pdmp3_amd_mfcc_long_dct_table(257, 1, 0.0, NULL, 0, NULL, NULL) == -1);
  EXPECT(pdmp3_amd_mfcc_long_dct_table(20, 21, 0.0, NULL, 0, NULL, NULL) == -1);
  EXPECT(pdmp3_amd_mfcc_long_dct_table(256, 129, 0.0, NULL, 0, NULL, NULL) == -1);
  EXPECT(pdmp3_amd_mfcc_long_dct_table(128, 20, -1.0, NULL, 0, NULL, NULL) == -1);
  EXPECT(pdmp3_amd_mfcc_long_dct_table(128, 20, NAN, NULL, 0, NULL, NULL) == -1);
  /* the taps: 2 w doubles or nothing */
  for (int w = -1; w <= 19; w++) {
    const int ok = w >= 3 && w <= 17 && (w & 1);
    EXPECT(pdmp3_amd_mfcc_long_delta_taps(w, NULL, 0) == (ok ? w : -1));
    if (!ok) { double one = 7.0; EXPECT(pdmp3_amd_mfcc_long_delta_taps(w, &one, 1) == -1 && one == 7.0); continue; }
    double* t = (double*)malloc(2 * (size_t)w * sizeof *t);
    double* small = (double*)malloc((2 * (size_t)w - 1) * sizeof *small);
    if (!t || !small) return 2;
    small[0] = 7.0;
    EXPECT(pdmp3_amd_mfcc_long_delta_taps(w, small, 2 * (size_t)w - 1) == -1 && small[0] == 7.0);
    EXPECT(pdmp3_amd_mfcc_long_delta_taps(w, t, 2 * (size_t)w) == w);
    double s1 = 0.0, s2 = 0.0;
    for (int j = 0; j < w; j++) { s1 += t[j] * (double)(j - w / 2); s2 += t[w + j] * (double)((j - w / 2) * (j - w / 2)); }
    EXPECT(fabs(s1 - 1.0) < 1e-14 && fabs(s2 - 2.0) < 1e-13 && t[w / 2] == 0.0);
    free(t); free(small);
  }
  /* the plan over the edges */
  static const int dl[] = {0, 1, 2};
  for (unsigned i = 0; i < sizeof mels / sizeof *mels; i++)
    for (int nc = 1; nc <= mels[i] && nc <= 128; nc += (nc < 16 ? 1 : 37))
      for (int w = 3; w <= 17; w += 2)
        for (int di = 0; di < 3; di++) {
          int v[5] = {-7, -7, -7, -7, -7};
          unsigned lds = 7;
          EXPECT(pdmp3_amd_mfcc_long_plan(mels[i], nc, dl[di], w, 0, &v[0], &v[1], &v[2], &v[3], &v[4], &lds) == 0);
          const int h = dl[di] ? w / 2 : 0;
          EXPECT(v[0] == h && v[1] == h && v[2] == 64 && v[3] == 80 && v[4] == 84);
          EXPECT(lds == (unsigned)(((mels[i] + 15) & ~15) * 80 + ((nc + 15) & ~15) * 84) * 4u && lds <= PDMP3_MEL_LDS_MAX);
        }
  {
    int v[5] = {-7, -7, -7, -7, -7};
    unsigned lds = 7;
    EXPECT(pdmp3_amd_mfcc_long_plan(128, 20, 2, 9, 0, NULL, NULL, NULL, NULL, NULL, NULL) == 0);
    EXPECT(pdmp3_amd_mfcc_long_plan(128, 0, 9, 4, 1, &v[0], &v[1], &v[2], &v[3], &v[4], &lds) == 0 && v[0] == 0 && v[1] == 0 && v[2] == 1024 && lds == 0);
    EXPECT(pdmp3_amd_mfcc_long_plan(0, 1, 0, 9, 0, &v[0], &v[1], &v[2], &v[3], &v[4], &lds) == -1);
    EXPECT(pdmp3_amd_mfcc_long_plan(257, 1, 0, 9, 0, &v[0], &v[1], &v[2], &v[3], &v[4], &lds) == -1);
    EXPECT(pdmp3_amd_mfcc_long_plan(128, 129, 0, 9, 0, &v[0], &v[1], &v[2], &v[3], &v[4], &lds) == -1);
    EXPECT(pdmp3_amd_mfcc_long_plan(20, 21, 0, 9, 0, &v[0], &v[1], &v[2], &v[3], &v[4], &lds) == -1);
    EXPECT(pdmp3_amd_mfcc_long_plan(128, 20, 3, 9, 0, &v[0], &v[1], &v[2], &v[3], &v[4], &lds) == -1);
    EXPECT(pdmp3_amd_mfcc_long_plan(128, 20, 1, 8, 0, &v[0], &v[1], &v[2], &v[3], &v[4], &lds) == -1);
    EXPECT(pdmp3_amd_mfcc_long_plan(128, 20, 1, 19, 0, &v[0], &v[1], &v[2], &v[3], &v[4], &lds) == -1);
    EXPECT(pdmp3_amd_mfcc_long_plan(128, 20, 0, 9, 2, &v[0], &v[1], &v[2], &v[3], &v[4], &lds) == -1);
    EXPECT(v[0] == 0 && v[2] == 1024 && lds == 0);          /* (a refusal writes nothing) */
  }
  if (fails) return 1;
  printf("mfcc_long_plan: ok\n");
  return 0;
}
