/* Sanitizer run of the chroma features' planning (pdmp3_amd/host/clip_chroma.c over clip_cqt.c) on the CPU: the check, the map
 * into buffers of exactly the size asked for (AddressSanitizer sees one int too many), the plan over every hop, and the
 * refusals.  A stand-alone program, no GPU:
 *   gcc -O1 -g -fsanitize=address,undefined -Iinclude -Ipdmp3_amd/csrc -o chroma_plan tools/sanitize/chroma_plan.c \
 *       pdmp3_amd/host/clip_chroma.c pdmp3_amd/host/clip_cqt.c -lm && ./chroma_plan
 * (tests/test_clip_chroma_host.py builds and runs it.) */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../pdmp3_amd/host/bulk_internal.h"

static int fails;
#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "chroma_plan: line %d: %s\n", __LINE__, #c); fails++; } } while (0)

static pdmp3_amd_chroma_spec spec_of(int hop, double fmin, int n_bins, int bpo, int n_chroma, int base, int norm) {
  pdmp3_amd_chroma_spec s;
  memset(&s, 0, sizeof s);
  s.cqt.channels = 1; s.cqt.hop = hop; s.cqt.fmin = fmin; s.cqt.n_bins = n_bins; s.cqt.bins_per_octave = bpo; s.cqt.filter_scale = 1.0;
  s.cqt.norm = 1; s.cqt.scale = 1; s.cqt.n_frames = 10; s.cqt.out_mode = 1;
  s.n_chroma = n_chroma; s.base_class = base; s.chroma_norm = norm; s.norm_floor = 1e-10;
  return s;
}

static void one(long sr, const pdmp3_amd_chroma_spec* s) {
  EXPECT(pdmp3_amd_chroma_check(s, sr) == 0);
  const int nb = s->cqt.n_bins, r = s->cqt.bins_per_octave / s->n_chroma;
  int* cls = (int*)malloc((size_t)nb * sizeof *cls);
  int* count = (int*)malloc((size_t)s->n_chroma * sizeof *count);
  EXPECT(pdmp3_amd_chroma_map(s, sr, cls, (size_t)nb, count) == nb);
  EXPECT(pdmp3_amd_chroma_map(s, sr, cls, (size_t)nb - 1, count) == -1);
  EXPECT(pdmp3_amd_chroma_map(s, sr, NULL, 0, NULL) == nb);
  int total = 0;
  for (int p = 0; p < s->n_chroma; p++) { EXPECT(count[p] >= 0); total += count[p]; }
  EXPECT(total == nb);
  for (int k = 0; k < nb; k++) EXPECT(cls[k] == ((k + r / 2) / r + s->base_class) % s->n_chroma);
  int tile = 0, pad = 0, split = 0, seg = 0, ns = 0;
  unsigned lds = 0, q_at = 0, class_at = 0;
  EXPECT(pdmp3_amd_chroma_plan(s, sr, &tile, &pad, &lds, &split, &seg, &ns, &q_at, &class_at) == 0);
  EXPECT((tile == 16 || tile == 8 || tile == 4) && lds <= PDMP3_MEL_LDS_MAX && split == PDMP3_CQT_SPLIT_ROWS && seg == PDMP3_CQT_SEGMENTS);
  EXPECT(q_at == class_at + PDMP3_CQT_PART_FLOATS && (q_at + (unsigned)((nb + 15) / 16) * 16u * 17u) * 4u == lds);
  EXPECT((unsigned)s->n_chroma * 17u <= PDMP3_CQT_PART_FLOATS);
  free(cls); free(count);
}

int main(void) {
  const double c1 = 32.70319566257483;
  for (int norm = 0; norm < 4; norm++)
    for (int base = 0; base < 12; base += 5) {
      pdmp3_amd_chroma_spec s = spec_of(512, c1, 84, 12, 12, base, norm);
      one(22050, &s);
    }
  { pdmp3_amd_chroma_spec s = spec_of(512, 4.0 * c1, 108, 36, 12, 5, 3); one(22050, &s); }
  { pdmp3_amd_chroma_spec s = spec_of(512, 2.0 * c1, 108, 36, 36, 35, 2); one(22050, &s); }
  { pdmp3_amd_chroma_spec s = spec_of(512, c1, 84, 24, 12, 0, 1); one(22050, &s); }
  { pdmp3_amd_chroma_spec s = spec_of(160, 1000.0, 17, 12, 12, 0, 3); one(16000, &s); }
  { pdmp3_amd_chroma_spec s = spec_of(160, 1000.0, 1, 12, 1, 0, 3); one(16000, &s); }
  { pdmp3_amd_chroma_spec s = spec_of(64, 220.0, 512, 96, 96, 95, 3); one(22050, &s); }
  /* 36 an octave from C1 at 22 050 Hz: the constant-Q transform's own check refuses it */
  { pdmp3_amd_chroma_spec s = spec_of(512, c1, 108, 36, 12, 0, 3); EXPECT(pdmp3_amd_chroma_check(&s, 22050) == -1 && pdmp3_amd_cqt_check(&s.cqt, 22050) == -1); }
  /* the plan over every hop: accepted or refused, never out of range, never a larger tile than the constant-Q call's */
  for (int hop = -2; hop <= 8194; hop++) {
    pdmp3_amd_chroma_spec s = spec_of(hop, c1, 24, 12, 12, 0, 3);
    pdmp3_chroma_params p;
    pdmp3_cqt_params cp;
    const int rc = chroma_plan(&s, 44100, &p);
    if (hop < 1 || hop > 8192) { EXPECT(rc == -1); continue; }
    if (rc == 0) {
      EXPECT(cqt_plan(&s.cqt, 44100, &cp) == 0 && p.cqt.tile <= cp.tile);
      EXPECT(p.cqt.lds_bytes <= PDMP3_MEL_LDS_MAX && p.cqt.span_floats % 4 == 0 && (p.q_at + 2u * 16u * 17u) * 4u == p.cqt.lds_bytes);
    }
  }
  /* refusals */
  {
    pdmp3_amd_chroma_spec s = spec_of(512, c1, 84, 12, 12, 0, 3);
    EXPECT(pdmp3_amd_chroma_check(NULL, 22050) == -1 && pdmp3_amd_chroma_check(&s, 0) == -1);
    const int bad_n[] = {0, -1, 5, 24, 97, 0x7fffffff, -0x7fffffff - 1};
    for (size_t i = 0; i < sizeof bad_n / sizeof *bad_n; i++) { s.n_chroma = bad_n[i]; EXPECT(pdmp3_amd_chroma_check(&s, 22050) == -1); }
    s.n_chroma = 12;
    s.cqt.bins_per_octave = 0; EXPECT(pdmp3_amd_chroma_check(&s, 22050) == -1);
    s.cqt.bins_per_octave = 12;
    const int bad_b[] = {-1, 12, 0x7fffffff};
    for (size_t i = 0; i < sizeof bad_b / sizeof *bad_b; i++) { s.base_class = bad_b[i]; EXPECT(pdmp3_amd_chroma_check(&s, 22050) == -1); }
    s.base_class = 0;
    const double bad_f[] = {0.0, -1.0, 1e-46, 1e39, 0.0 / 0.0, 1.0 / 0.0};
    for (size_t i = 0; i < sizeof bad_f / sizeof *bad_f; i++) {
      s.norm_floor = bad_f[i];
      s.chroma_norm = 3; EXPECT(pdmp3_amd_chroma_check(&s, 22050) == -1);
      s.chroma_norm = 0; EXPECT(pdmp3_amd_chroma_check(&s, 22050) == 0);      /* (not used there) */
    }
    s.norm_floor = 1e-10; s.chroma_norm = 4; EXPECT(pdmp3_amd_chroma_check(&s, 22050) == -1);
    s.chroma_norm = 3;
    for (int m = -1; m <= 5; m++) { s.cqt.out_mode = m; s.cqt.floor = 1e-10; EXPECT((pdmp3_amd_chroma_check(&s, 22050) == 0) == (m == 1 || m == 2)); }
  }
  if (fails) return 1;
  printf("chroma_plan: ok\n");
  return 0;
}
