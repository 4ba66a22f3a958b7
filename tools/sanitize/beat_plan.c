/* Sanitizer run of the beat call's planning (pdmp3_amd/host/clip_beat.c) on the CPU: the check and its refusals one by one, the
 * period and h at the rounding boundaries, the two tables into buffers of exactly their sizes at the smallest and the largest
 * period, the block of every admissible period at bpm 0 -- every entry written, nothing behind it --, the plan over every
 * period.  A stand-alone program, no GPU:
 *   gcc -O1 -g -fsanitize=address,undefined -Iinclude -Ipdmp3_amd/csrc -o beat_plan tools/sanitize/beat_plan.c \
 *       pdmp3_amd/host/clip_beat.c pdmp3_amd/host/clip_tempogram.c pdmp3_amd/host/clip_mel_long.c pdmp3_amd/host/clip_mel.c \
 *       pdmp3_amd/host/clip_stft_long.c pdmp3_amd/host/clip_stft.c -lm && ./beat_plan
 * (tests/test_clip_beat_host.py builds and runs it.) */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../pdmp3_amd/host/bulk_internal.h"

static int fails;
#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "beat_plan: line %d: %s\n", __LINE__, #c); fails++; } } while (0)

static pdmp3_amd_beat_spec spec_of(double bpm, int wt, long long frames) {
  pdmp3_amd_beat_spec s;
  memset(&s, 0, sizeof s);
  s.tg.mel.mel.n_fft = 2048; s.tg.mel.mel.hop = 512; s.tg.mel.mel.n_mels = 128; s.tg.mel.mel.norm = 1; s.tg.mel.mel.floor = 1e-10;
  s.tg.mel.mel.n_frames = frames; s.tg.mel.mel.channels = 1;
  s.tg.lag = 1; s.tg.max_size = 1; s.tg.win_length = wt; s.tg.start_bpm = 120.0; s.tg.std_bpm = 1.0; s.tg.max_tempo = 320.0;
  s.bpm = bpm; s.tightness = 100.0; s.trim = 1; s.out_mode = 2;
  return s;
}

static int half_of(int P) { const int h = (int)nearbyint((double)P / 2.0); return h < 1 ? 1 : h; }

/* the period of a bpm at 22 050 Hz and hop 512, or -1 */
static int period_of(double bpm) {
  pdmp3_amd_beat_spec s = spec_of(bpm, 384, 10);
  int numbers[8];
  if (pdmp3_amd_beat_plan(&s, 22050, numbers, NULL, NULL) != 0) return -1;
  EXPECT(numbers[2] == numbers[0] && numbers[3] == numbers[0] && numbers[1] == half_of(numbers[0]) && numbers[4] == 256);
  EXPECT(numbers[6] * numbers[7] == 256 && numbers[6] >= 1 && numbers[6] <= 64 && (numbers[6] == 64 || numbers[6] * 2 * numbers[1] > 256));
  EXPECT(numbers[5] == (10 + numbers[1] - 1) / numbers[1]);
  return numbers[0];
}

int main(void) {
  pdmp3_amd_beat_spec s = spec_of(120.0, 384, 10);
  EXPECT(pdmp3_amd_beat_check(&s, 22050) == 0 && pdmp3_amd_beat_check(NULL, 22050) == -1 && pdmp3_amd_beat_check(&s, 0) == -1);
  EXPECT(pdmp3_amd_beat_plan(NULL, 22050, NULL, NULL, NULL) == -1 && pdmp3_amd_beat_tables(NULL, 22050, 22, NULL, NULL) == -1);
  EXPECT(pdmp3_amd_beat_plan(&s, 22050, NULL, NULL, NULL) == 0);
  /* 60 * 22050 / 512 = 2583.984375 frames a minute */
  EXPECT(period_of(120.0) == 22 && period_of(2583.984375 / 21.6) == 22 && period_of(2583.984375 / 22.4) == 22 && period_of(2583.984375 / 20.4) == 20);
  EXPECT(period_of(2583.984375) == 1 && period_of(2583.984375 / 1023.0) == 1023 && period_of(2583.984375 / 1023.6) == -1);
  EXPECT(period_of(2583.984375 * 2.0) == -1 && period_of(2583.984375 / 0.5) == -1 && period_of(1e300) == -1 && period_of(1e-300) == -1);
  /* the refusals, one by one */
#define REFUSED(change) do { s = spec_of(120.0, 384, 10); change; EXPECT(pdmp3_amd_beat_check(&s, 22050) == -1); } while (0)
  REFUSED(s.bpm = -1.0);
  REFUSED(s.bpm = NAN);
  REFUSED(s.bpm = INFINITY);
  REFUSED(s.tightness = 0.0);
  REFUSED(s.tightness = -100.0);
  REFUSED(s.tightness = NAN);
  REFUSED(s.tightness = INFINITY);
  REFUSED(s.out_mode = 3);
  REFUSED(s.out_mode = -1);
  REFUSED(s.trim = 2);
  REFUSED(s.tg.mel.mel.n_frames = 32769);
  REFUSED(s.tg.mel.mel.n_frames = -1);
  REFUSED(s.tg.win_length = 383);
  REFUSED(s.tg.lag = 0);
  REFUSED(s.tg.mel.mel.n_fft = 1024);
  REFUSED(s.bpm = 0.0; s.tg.max_tempo = 1.0);                          /* no admissible lag */
  s = spec_of(120.0, 384, 32768); EXPECT(pdmp3_amd_beat_check(&s, 22050) == 0);
  s = spec_of(0.0, 1024, 32768); EXPECT(pdmp3_amd_beat_check(&s, 22050) == 0);
  s = spec_of(120.0, 384, 0); EXPECT(pdmp3_amd_beat_check(&s, 22050) == 0);
  /* the tables of a period into buffers of exactly their sizes */
  s = spec_of(120.0, 384, 10);
  EXPECT(pdmp3_amd_beat_tables(&s, 22050, 0, NULL, NULL) == -1 && pdmp3_amd_beat_tables(&s, 22050, 1024, NULL, NULL) == -1);
  for (int P = 1; P <= 1023; P += P < 48 ? 1 : 65) {
    double* g = (double*)malloc((size_t)(P + 1) * sizeof *g);
    double* tx = (double*)malloc((size_t)(2 * P + 1) * sizeof *tx);
    EXPECT(g && tx && pdmp3_amd_beat_tables(&s, 22050, P, g, tx) == 0);
    const int h = half_of(P);
    EXPECT(g[0] == 1.0 && g[P] == exp(-512.0) && tx[P] == 0.0);
    for (int k = 1; k <= P; k++) EXPECT(g[k] < g[k - 1] && g[k] > 0.0);
    for (int d = 0; d <= 2 * P; d++) EXPECT(d < h ? tx[d] == 0.0 : (isfinite(tx[d]) && tx[d] <= 0.0));
    EXPECT(pdmp3_amd_beat_tables(&s, 22050, P, g, NULL) == 0 && pdmp3_amd_beat_tables(&s, 22050, P, NULL, tx) == 0);
    free(g); free(tx);
  }
  /* bpm 0: the block of every admissible period, as the call fills it */
  for (int wt = 16; wt <= 1024; wt += 56) {
    s = spec_of(0.0, wt, 1000);
    int numbers[8], first = -7;
    unsigned lds[2];
    unsigned long long stage[2];
    const int rc = pdmp3_amd_beat_plan(&s, 22050, numbers, lds, stage);
    pdmp3_amd_tempogram_spec tg = s.tg;
    tg.out_mode = 2;
    EXPECT((rc == 0) == (pdmp3_amd_tempogram_prior(&tg, 22050, NULL, 0, &first) == 0));
    if (rc != 0) continue;
    EXPECT(numbers[0] == 0 && numbers[2] == first && numbers[3] == wt - 1 && numbers[1] == half_of(wt - 1));
    EXPECT(lds[0] <= PDMP3_MEL_LDS_SOFT && lds[1] <= PDMP3_MEL_LDS_SOFT);
    EXPECT(stage[0] == (8u + 2000u + 1500u) * 8ull);
    size_t doubles = 0;
    for (int P = first; P < wt; P++) doubles += 3u * (size_t)P + 2u;
    EXPECT(stage[1] == doubles * 8u);
    pdmp3_beat_params p;
    EXPECT(beat_plan(&s, 22050, &p) == 0 && beat_table_bytes(&p) == doubles * 8u);
    double* t = (double*)malloc(doubles * sizeof *t);
    for (size_t i = 0; i < doubles; i++) t[i] = NAN;
    EXPECT(t && beat_tables_fill(&s, &p, t) == 0);
    for (size_t i = 0; i < doubles; i++) EXPECT(isfinite(t[i]));
    const double a = log(2.0 * (wt - 1)) - log((double)(wt - 1));
    EXPECT(t[0] == 1.0 && t[doubles - 1] == -100.0 * (a * a));
    free(t);
  }
  /* the plan over every period: the LDS fits */
  for (int P = 1; P <= 1023; P++) {
    s = spec_of(2583.984375 / (double)P, 384, 32768);
    int numbers[8];
    unsigned lds[2];
    EXPECT(pdmp3_amd_beat_plan(&s, 22050, numbers, lds, NULL) == 0 && numbers[0] == P && numbers[1] == half_of(P));
    EXPECT(lds[0] == (3u * (unsigned)P + 1u + 256u + 513u) * 8u && lds[1] == (4u * (unsigned)P + (unsigned)half_of(P) + 1u + 256u) * 8u);
    EXPECT(lds[0] <= PDMP3_MEL_LDS_SOFT && lds[1] <= PDMP3_MEL_LDS_SOFT);
  }
  if (fails) return 1;
  printf("beat_plan: ok\n");
  return 0;
}
