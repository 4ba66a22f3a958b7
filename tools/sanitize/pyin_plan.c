/* Sanitizer run of the pYIN call's planning (pdmp3_amd/host/clip_pyin.c) on the CPU: the check and its refusals one by one, the
 * rounding boundaries of n_s, n_b and msf, the tables -- every entry written, nothing behind the block, the sizes the plan
 * states -- over the defaults, the widest lag range, an even band on even and odd bin counts, two bins and 2048 bins, and the
 * plan over every hop of the longest frame.  A stand-alone program, no GPU:
 *   gcc -O1 -g -fsanitize=address,undefined -Iinclude -Ipdmp3_amd/csrc -o pyin_plan tools/sanitize/pyin_plan.c \
 *       pdmp3_amd/host/clip_pyin.c pdmp3_amd/host/clip_pitch.c -lm && ./pyin_plan
 * (tests/test_clip_pyin_host.py builds and runs it.) */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../pdmp3_amd/host/bulk_internal.h"

static int fails;
#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "pyin_plan: line %d: %s\n", __LINE__, #c); fails++; } } while (0)

static pdmp3_amd_pyin_spec spec_of(int N, int W, int H, double fmin, double fmax, double resolution) {
  pdmp3_amd_pyin_spec s;
  memset(&s, 0, sizeof s);
  s.pitch.frame_length = N; s.pitch.win_length = W; s.pitch.hop = H; s.pitch.fmin = fmin; s.pitch.fmax = fmax; s.pitch.n_frames = 10;
  s.n_thresholds = 100; s.beta_a = 2.0; s.beta_b = 18.0; s.boltzmann = 2.0; s.resolution = resolution; s.max_transition_rate = 35.92;
  s.switch_prob = 0.01; s.no_trough_prob = 0.01; s.fill = NAN;
  return s;
}

/* the tables of a spec into a block of exactly the size the call states (the sanitizer sees a write behind it), every entry
 * finite but ltri's zeros, the weights non-negative and summing to 1, T falling */
static void tables_of(const pdmp3_amd_pyin_spec* s, long sr, int want_bins, int want_band) {
  int counts[4] = {-7, -7, -7, -7}, numbers[8];
  unsigned lds[2];
  unsigned long long stage[3];
  const int need = pdmp3_amd_pyin_tables(s, sr, NULL, 0, counts);
  EXPECT(need > 0 && counts[2] == want_bins);
  EXPECT(pdmp3_amd_pyin_plan(s, sr, numbers, lds, stage) == 0 && numbers[1] == want_bins && numbers[0] == 2 * want_bins && numbers[4] == want_band);
  EXPECT(numbers[5] == want_band / 2 && counts[3] == numbers[5] && lds[0] <= PDMP3_MEL_LDS_SOFT && lds[1] <= PDMP3_MEL_LDS_MAX);
  EXPECT(numbers[6] == 8 || numbers[6] == 4 || numbers[6] == 2 || numbers[6] == 1);
  EXPECT(numbers[7] >= 64 && numbers[7] <= 1024 && !(numbers[7] & 63) && (numbers[7] >= want_bins || numbers[7] == 1024));
  EXPECT(stage[1] == (s->out_mode ? 0u : 10ull * (unsigned)(want_bins + 1) * 4u) && stage[2] == (s->out_mode ? 0u : 10ull * (unsigned)want_bins * 4u));
  if (need <= 0) return;
  double* t = (double*)malloc((size_t)need * sizeof *t);
  EXPECT(t && pdmp3_amd_pyin_tables(s, sr, t, (size_t)need - 1, NULL) == -1);
  EXPECT(pdmp3_amd_pyin_tables(s, sr, t, (size_t)need, NULL) == need);
  const int nt = counts[0], mt = counts[1], nb = counts[2], hb = counts[3];
  const double* theta = t, *w = theta + nt, *wsum = w + nt, *G = wsum + nt + 1, *cN = G + mt, *T = cN + mt + 1, *ltri = T + nb, *lZ = ltri + 2 * hb + 1;
  for (int i = 0; i < nt; i++) EXPECT(w[i] >= 0.0 && theta[i] == (double)(i + 1) / nt);
  EXPECT(fabs(wsum[nt] - 1.0) < 1e-12 && wsum[0] == 0.0 && G[0] == 1.0 && cN[1] == 1.0);
  for (int q = 1; q < nb; q++) EXPECT(T[q] < T[q - 1]);
  int zeros = 0;
  for (int d = 0; d <= 2 * hb; d++) { EXPECT(ltri[d] <= 0.0); zeros += isinf(ltri[d]) ? 1 : 0; }
  EXPECT(zeros == ((want_band & 1) ? 0 : 1));
  for (int i = 0; i < nb; i++) EXPECT(isfinite(lZ[i]) && lZ[i] >= 0.0 - 1e-12);
  const float* f0 = (const float*)(lZ + nb);
  EXPECT(f0[0] == (float)s->pitch.fmin && f0[nb - 1] <= (float)s->pitch.fmax);
  EXPECT(t[need - 2] == log(2.2250738585072014e-308) && t[need - 1] == -log((double)nb) && t[need - 3] == log(s->switch_prob));
  free(t);
}

int main(void) {
  pdmp3_amd_pyin_spec s = spec_of(2048, 0, 0, 65.406, 2093.0, 0.1);
  EXPECT(pdmp3_amd_pyin_check(&s, 22050) == 0 && pdmp3_amd_pyin_check(NULL, 22050) == -1 && pdmp3_amd_pyin_check(&s, 0) == -1);
  EXPECT(pdmp3_amd_pyin_tables(NULL, 22050, NULL, 0, NULL) == -1 && pdmp3_amd_pyin_plan(NULL, 22050, NULL, NULL, NULL) == -1);
  EXPECT(pdmp3_amd_pyin_plan(&s, 22050, NULL, NULL, NULL) == 0);
  tables_of(&s, 22050, 601, 101);
  s.out_mode = 1; tables_of(&s, 22050, 601, 101);
  /* the refusals, one by one */
#define REFUSED(change) do { s = spec_of(2048, 0, 0, 65.406, 2093.0, 0.1); change; EXPECT(pdmp3_amd_pyin_check(&s, 22050) == -1); } while (0)
  REFUSED(s.pitch.frame_length = 2047);
  REFUSED(s.pitch.fmax = 11025.5);
  REFUSED(s.n_thresholds = 0);
  REFUSED(s.n_thresholds = 257);
  REFUSED(s.boltzmann = 0.0);
  REFUSED(s.boltzmann = NAN);
  REFUSED(s.boltzmann = INFINITY);
  REFUSED(s.switch_prob = 0.0);
  REFUSED(s.switch_prob = 1.0);
  REFUSED(s.switch_prob = NAN);
  REFUSED(s.no_trough_prob = 0.0);
  REFUSED(s.no_trough_prob = 1.0);
  REFUSED(s.resolution = 0.0);
  REFUSED(s.resolution = NAN);
  REFUSED(s.resolution = 0.049);
  REFUSED(s.resolution = 1e-300);
  REFUSED(s.resolution = 1.0 / (3.0 + 1e-12));
  REFUSED(s.pitch.fmax = 65.5);                                        /* n_b 1 */
  REFUSED(s.pitch.fmin = 20.0; s.pitch.fmax = 11000.0; s.resolution = 0.05);   /* n_b 2185 */
  REFUSED(s.pitch.fmin = 100.0; s.pitch.fmax = 200.0 * (1.0 + 1e-13));
  REFUSED(s.max_transition_rate = 300.0);                              /* Wd 841 > n_b */
  REFUSED(s.max_transition_rate = -1.0);
  REFUSED(s.max_transition_rate = NAN);
  REFUSED(s.max_transition_rate = 1e300);
  REFUSED(s.beta_a = 2.5);
  REFUSED(s.beta_b = 65.0);
  REFUSED(s.beta_a = 0.0);
  REFUSED(s.beta_a = NAN);
  REFUSED(s.out_mode = 2);
  REFUSED(s.out_mode = -1);
  REFUSED(s.use_bin_frequency = 2);
  REFUSED(s.pitch.n_frames = -1);
  REFUSED(s.pitch.n_frames = 0x7fffffffLL / 339 + 1);
  static double weights[256];
  for (int i = 0; i < 256; i++) weights[i] = 1.0 / 256.0;
  s = spec_of(2048, 0, 0, 65.406, 2093.0, 0.1);
  s.beta_a = 2.5; s.threshold_weights = weights; s.n_thresholds = 256;
  EXPECT(pdmp3_amd_pyin_check(&s, 22050) == 0);
  tables_of(&s, 22050, 601, 101);
  weights[255] = -1e-9; EXPECT(pdmp3_amd_pyin_check(&s, 22050) == -1);
  weights[255] = NAN; EXPECT(pdmp3_amd_pyin_check(&s, 22050) == -1);
  weights[255] = 0.0;
  /* boundaries that are the value itself pass */
  s = spec_of(2048, 0, 0, 100.0, 200.0, 0.1); tables_of(&s, 22050, 121, 101);
  s = spec_of(2048, 0, 0, 65.406, 2093.0, 0.05); tables_of(&s, 22050, 1201, 201);
  s = spec_of(2048, 512, 256, 10.5, 21.0, 0.5); tables_of(&s, 16000, 25, 15);                 /* the widest lag range: 761 .. 1524 */
  s.max_transition_rate = 62.5; tables_of(&s, 16000, 25, 25);                                  /* Wd = n_b */
  s.pitch.hop = 512; EXPECT(pdmp3_amd_pyin_check(&s, 16000) == -1);                            /* Wd 49 > n_b */
  s = spec_of(2048, 0, 256, 65.406, 2093.0, 1.0); tables_of(&s, 22050, 61, 6);                 /* an even band, odd bins */
  s = spec_of(2048, 0, 256, 65.406, 2000.0, 1.0); tables_of(&s, 22050, 60, 6);                 /* an even band, even bins */
  s = spec_of(2048, 0, 0, 100.0, 108.0, 1.0); s.max_transition_rate = 0.0; tables_of(&s, 16000, 2, 1);
  s = spec_of(2048, 0, 0, 30.0, 10000.0, 0.05); s.max_transition_rate = 0.0; tables_of(&s, 22050, 2012, 1);
  /* the plan over every hop of the longest frame: the band grows with the hop */
  for (int H = 1; H <= 2048; H++) {
    s = spec_of(2048, 0, H, 65.406, 2093.0, 0.1);
    int numbers[8];
    unsigned lds[2];
    const int rc = pdmp3_amd_pyin_plan(&s, 22050, numbers, lds, NULL);
    const double q = 35.92 * 12.0 * (double)H / 22050.0;
    if (fabs(q - floor(q) - 0.5) < 1e-9) continue;
    const int band = (int)nearbyint(q) * 10 + 1;
    EXPECT((rc == 0) == (band <= 601));
    if (rc == 0) EXPECT(numbers[4] == band && numbers[1] == 601 && lds[0] <= PDMP3_MEL_LDS_SOFT);
  }
  if (fails) return 1;
  printf("pyin_plan: ok\n");
  return 0;
}
