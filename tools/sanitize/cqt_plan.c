/* Sanitizer run of the constant-Q transform's planning (pdmp3_amd/host/clip_cqt.c) on the CPU: the check, the lengths, the
 * ragged table into buffers of exactly the size asked for (AddressSanitizer sees one float too many), the plan over every hop,
 * the refusals, and the decoder's cache of tables through more specs than it keeps.  A stand-alone program, no GPU:
 *   gcc -O1 -g -fsanitize=address,undefined -Iinclude -Ipdmp3_amd/csrc -o cqt_plan tools/sanitize/cqt_plan.c \
 *       pdmp3_amd/host/clip_cqt.c -lm && ./cqt_plan
 * (tests/test_clip_cqt_host.py builds and runs it.) */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../pdmp3_amd/host/bulk_internal.h"

static int fails;
#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "cqt_plan: line %d: %s\n", __LINE__, #c); fails++; } } while (0)

static pdmp3_amd_cqt_spec spec_of(int hop, double fmin, int n_bins, int bpo, double fs, int norm, int scale) {
  pdmp3_amd_cqt_spec s;
  memset(&s, 0, sizeof s);
  s.channels = 1; s.hop = hop; s.fmin = fmin; s.n_bins = n_bins; s.bins_per_octave = bpo; s.filter_scale = fs; s.norm = norm; s.scale = scale;
  s.n_frames = 10; s.out_mode = 1; s.floor = 1e-10;
  return s;
}

static void one(long sr, const pdmp3_amd_cqt_spec* s) {
  EXPECT(pdmp3_amd_cqt_check(s, sr) == 0);
  const int nt = (s->n_bins + 15) / 16;
  double* f = (double*)malloc((size_t)s->n_bins * sizeof *f);
  int* h = (int*)malloc((size_t)s->n_bins * sizeof *h);
  int* rows = (int*)malloc((size_t)nt * sizeof *rows);
  int* at = (int*)malloc((size_t)nt * sizeof *at);
  EXPECT(pdmp3_amd_cqt_lengths(s, sr, f, h, (size_t)s->n_bins) == s->n_bins);
  EXPECT(pdmp3_amd_cqt_lengths(s, sr, f, h, (size_t)s->n_bins - 1) == -1);
  const long long count = pdmp3_amd_cqt_table(s, sr, NULL, 0, rows, at);
  EXPECT(count > 0 && count <= (1LL << 22));
  float* t = (float*)malloc((size_t)count * sizeof *t);
  EXPECT(pdmp3_amd_cqt_table(s, sr, t, (size_t)count, NULL, NULL) == count);
  EXPECT(pdmp3_amd_cqt_table(s, sr, t, (size_t)count - 1, NULL, NULL) == -1);
  long long total = 0;
  for (int i = 0; i < nt; i++) { EXPECT(at[i] == total && rows[i] == ((2 * h[16 * i] + 1 + 3) & ~3)); total += rows[i]; }
  EXPECT(total * 32 == count);
  double sum = 0.0;
  for (long long i = 0; i < count; i++) sum += t[i] < 0 ? -t[i] : t[i];
  EXPECT(sum > 0.0);
  int tile = 0, pad = 0, split = 0, seg = 0, ns = 0;
  unsigned lds = 0;
  EXPECT(pdmp3_amd_cqt_plan(s, sr, &tile, &pad, &lds, &split, &seg, &ns) == 0);
  EXPECT((tile == 16 || tile == 8 || tile == 4) && lds <= PDMP3_MEL_LDS_MAX && split == PDMP3_CQT_SPLIT_ROWS && seg == PDMP3_CQT_SEGMENTS && ns <= nt);
  free(f); free(h); free(rows); free(at); free(t);
}

int main(void) {
  const double c1 = 32.70319566257483;
  for (int norm = 0; norm < 3; norm++)
    for (int scale = 0; scale < 3; scale++) {
      pdmp3_amd_cqt_spec s = spec_of(512, c1, 84, 12, 1.0, norm, scale);
      one(22050, &s);
    }
  { pdmp3_amd_cqt_spec s = spec_of(256, 55.0, 96, 24, 1.0, 1, 1); one(48000, &s); }
  { pdmp3_amd_cqt_spec s = spec_of(160, 1000.0, 17, 12, 1.0, 1, 1); one(16000, &s); }
  { pdmp3_amd_cqt_spec s = spec_of(1, 500.0, 3, 1, 0.875, 1, 1); one(8000, &s); }
  { pdmp3_amd_cqt_spec s = spec_of(64, 220.0, 512, 96, 1.0, 2, 2); one(22050, &s); }
  { pdmp3_amd_cqt_spec s = spec_of(64, 100.0, 1, 36, 1.0, 1, 0); one(44100, &s); }
  /* the plan over every hop: accepted or refused, never out of range */
  for (int hop = -2; hop <= 8194; hop++) {
    pdmp3_amd_cqt_spec s = spec_of(hop, c1, 24, 12, 1.0, 1, 1);
    pdmp3_cqt_params p;
    const int rc = cqt_plan(&s, 44100, &p);
    if (hop < 1 || hop > 8192) { EXPECT(rc == -1); continue; }
    if (rc == 0) EXPECT(p.lds_bytes <= PDMP3_MEL_LDS_MAX && p.span_floats % 4 == 0 && p.tile_base[1] + p.tile_rows[1] <= p.rows0 + 3);
  }
  /* refusals: numbers at which a careless check would overflow or divide by zero */
  {
    const double bad_f[] = {0.0, -1.0, 1e-320, 1e308, 0.0 / 0.0, 1.0 / 0.0};
    for (size_t i = 0; i < sizeof bad_f / sizeof *bad_f; i++) {
      pdmp3_amd_cqt_spec s = spec_of(512, bad_f[i], 84, 12, 1.0, 1, 1);
      EXPECT(pdmp3_amd_cqt_check(&s, 22050) == -1);
      s = spec_of(512, c1, 84, 12, bad_f[i], 1, 1);
      EXPECT(pdmp3_amd_cqt_check(&s, 22050) == -1);
    }
    pdmp3_amd_cqt_spec s = spec_of(512, c1, 84, 12, 1.0, 1, 1);
    EXPECT(pdmp3_amd_cqt_check(&s, 0) == -1 && pdmp3_amd_cqt_check(&s, -5) == -1 && pdmp3_amd_cqt_check(NULL, 22050) == -1);
    s.n_bins = 0x7fffffff; EXPECT(pdmp3_amd_cqt_check(&s, 22050) == -1);
    s.n_bins = 84; s.bins_per_octave = 0; EXPECT(pdmp3_amd_cqt_check(&s, 22050) == -1);
  }
  /* the decoder's cache: more specs than it keeps, the first again, then freed as the decoder frees it */
  {
    struct bulk* b = (struct bulk*)calloc(1, sizeof *b);
    const float* first = NULL;
    for (int round = 0; round < 2; round++)
      for (int i = 0; i < PDMP3_CQT_TABLES + 2; i++) {
        pdmp3_amd_cqt_spec s = spec_of(512, 100.0 + i, 40, 12, 1.0, 1, 1);
        pdmp3_cqt_params p;
        EXPECT(cqt_plan(&s, 22050, &p) == 0);
        const float* t = cqt_table(b, &s, 22050, &p);
        EXPECT(t != NULL && t[(size_t)p.half0 * 32] != 0.0f);
        EXPECT(cqt_table(b, &s, 22050, &p) == t);  /* (kept: the same table again) */
        if (!round && !i) first = t;
      }
    (void)first;
    int n = 0;
    while (b->cqt_tabs) { cqt_tab* t = b->cqt_tabs; b->cqt_tabs = t->next; free(t->t); free(t); n++; }
    EXPECT(n == PDMP3_CQT_TABLES);
    free(b);
  }
  if (fails) return 1;
  printf("cqt_plan: ok\n");
  return 0;
}
