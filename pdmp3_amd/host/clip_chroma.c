/* clip_chroma.c -- libpdmp3.so: the planning of the chroma features of clips (include/pdmp3_bulk.h pdmp3_amd_chroma_*;
 * DESIGN.md section 17): the check, the class of every bin and the kernel's plan.  The transform under the fold is the
 * constant-Q transform's: its check, table, tile rows, split threshold, segments and cache of tables are clip_cqt.c's, called
 * and not restated.  Plain arithmetic, no GPU; the call itself (pdmp3_amd_bulk_decode_clips_chroma) is clip_features.c's. */
#include "bulk_internal.h"

#include <float.h>

/* the fold's own numbers: 1 when they are acceptable (the constant-Q transform's are cqt_plan's to judge) */
static int chroma_numbers_ok(const pdmp3_amd_chroma_spec* s) {
  if (!s || (s->cqt.out_mode != 1 && s->cqt.out_mode != 2)) return 0;
  if (s->n_chroma < 1 || s->n_chroma > 96 || s->cqt.bins_per_octave < 1 || s->cqt.bins_per_octave % s->n_chroma) return 0;
  if (s->base_class < 0 || s->base_class >= s->n_chroma || s->chroma_norm < 0 || s->chroma_norm > 3) return 0;
  if (s->chroma_norm && (!(s->norm_floor > 0.0) || !(s->norm_floor <= (double)FLT_MAX) || !((float)s->norm_floor >= FLT_MIN))) return 0;
  return 1;
}

static int chroma_class_of(const pdmp3_amd_chroma_spec* s, int k) {
  const int r = s->cqt.bins_per_octave / s->n_chroma;
  return ((k + r / 2) / r + s->base_class) % s->n_chroma;
}

/* cqt_plan's plan with more LDS behind the partial sums: the q plane, [n_bins rounded up to 16][17] floats.  The class plane,
 * [n_chroma][17] floats, lies over the partial sums (96 x 17 <= PDMP3_CQT_PART_FLOATS). */
HOST_LOCAL int chroma_plan(const pdmp3_amd_chroma_spec* s, long sr, pdmp3_chroma_params* p) {
  if (!chroma_numbers_ok(s)) return -1;
  memset(p, 0, sizeof *p);
  if (cqt_plan(&s->cqt, sr, &p->cqt) != 0) return -1;
  p->n_chroma = s->n_chroma; p->r = s->cqt.bins_per_octave / s->n_chroma;
  p->base_class = s->base_class; p->chroma_norm = s->chroma_norm;
  p->norm_floor = s->chroma_norm ? (float)s->norm_floor : 0.0f;
  const unsigned q_bytes = (unsigned)p->cqt.n_tiles * 16u * 17u * 4u;
  static const int tiles[3] = {16, 8, 4};
  for (int i = 0; i < 3; i++) {
    unsigned bytes;
    p->cqt.tile = tiles[i];
    cqt_lds(p->cqt.rows0, s->cqt.hop, p->cqt.tile, p->cqt.row_pad, &p->cqt.span_floats, &bytes);
    p->cqt.lds_bytes = bytes + q_bytes;
    if (p->cqt.lds_bytes > PDMP3_MEL_LDS_MAX) continue;
    p->class_at = p->cqt.span_floats;
    p->q_at = p->cqt.span_floats + (unsigned)PDMP3_CQT_PART_FLOATS;
    return 0;
  }
  return -1;
}

int pdmp3_amd_chroma_check(const pdmp3_amd_chroma_spec* s, long sr) {
  pdmp3_chroma_params p;
  return chroma_plan(s, sr, &p);
}

int pdmp3_amd_chroma_map(const pdmp3_amd_chroma_spec* s, long sr, int* cls, size_t cap, int* count) {
  if (pdmp3_amd_chroma_check(s, sr) != 0 || (cls && cap < (size_t)s->cqt.n_bins)) return -1;
  if (count) memset(count, 0, (size_t)s->n_chroma * sizeof *count);
  for (int k = 0; k < s->cqt.n_bins; k++) {
    const int c = chroma_class_of(s, k);
    if (cls) cls[k] = c;
    if (count) count[c]++;
  }
  return s->cqt.n_bins;
}

int pdmp3_amd_chroma_plan(const pdmp3_amd_chroma_spec* s, long sr, int* tile, int* row_pad, unsigned* lds_bytes, int* split_rows, int* segments,
                          int* n_split, unsigned* q_at, unsigned* class_at) {
  pdmp3_chroma_params p;
  if (chroma_plan(s, sr, &p) != 0) return -1;
  if (tile) *tile = p.cqt.tile;
  if (row_pad) *row_pad = p.cqt.row_pad;
  if (lds_bytes) *lds_bytes = p.cqt.lds_bytes;
  if (split_rows) *split_rows = PDMP3_CQT_SPLIT_ROWS;
  if (segments) *segments = PDMP3_CQT_SEGMENTS;
  if (n_split) *n_split = p.cqt.n_split;
  if (q_at) *q_at = p.q_at;
  if (class_at) *class_at = p.class_at;
  return 0;
}
