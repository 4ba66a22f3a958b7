/* clip_cqt.c -- libpdmp3.so: the planning of the constant-Q transform of clips (include/pdmp3_bulk.h pdmp3_amd_cqt_*;
 * DESIGN.md section 16): the check, the bins' frequencies and lengths, the ragged folded table (window, normalisation and
 * scale in the coefficients), the kernel's plan and the decoder's small cache of tables.  Plain arithmetic in binary64, no
 * GPU; the call itself (pdmp3_amd_bulk_decode_clips_cqt) is clip_features.c's. */
#include "bulk_internal.h"

#include <float.h>
#include <math.h>

#define CQT_TABLE_MAX AUDIO_TABLE_MAX

/* f_k and h_k of bin k (the spec's numbers are in range) */
static double cqt_q(const pdmp3_amd_cqt_spec* s) { return s->filter_scale / (pow(2.0, 1.0 / (double)s->bins_per_octave) - 1.0); }
static double cqt_freq(const pdmp3_amd_cqt_spec* s, int k) { return s->fmin * pow(2.0, (double)k / (double)s->bins_per_octave); }
static double cqt_len(const pdmp3_amd_cqt_spec* s, long sr, int k) { return cqt_q(s) * (double)sr / cqt_freq(s, k); }

/* everything but the plan's verdict: 1 when the numbers are acceptable */
static int cqt_numbers_ok(const pdmp3_amd_cqt_spec* s, long sr) {
  if (!s || sr <= 0 || sr > 0x7fffffffL) return 0;
  if (s->n_bins < 1 || s->n_bins > 16 * PDMP3_CQT_MAX_TILES || s->bins_per_octave < 1 || s->bins_per_octave > 96) return 0;
  if (!isfinite(s->fmin) || !(s->fmin > 0.0) || !isfinite(s->filter_scale) || !(s->filter_scale > 0.0)) return 0;
  if (s->hop < 1 || s->hop > 8192 || s->norm < 0 || s->norm > 2 || s->scale < 0 || s->scale > 2) return 0;
  if (s->n_frames < 0 || s->out_mode < 0 || s->out_mode > 4) return 0;
  if (s->out_mode >= 3 && (!(s->floor > 0.0) || !((float)s->floor >= FLT_MIN) || !(s->floor <= (double)FLT_MAX))) return 0;
  const double top = cqt_freq(s, s->n_bins - 1);
  if (!isfinite(top) || !(top < 0.5 * (double)sr)) return 0;
  const double l0 = cqt_len(s, sr, 0), l1 = cqt_len(s, sr, s->n_bins - 1);
  if (!isfinite(l0) || !(2.0 * floor(0.5 * l0) + 1.0 <= (double)PDMP3_CQT_MAX_LEN)) return 0;
  if (!(floor(0.5 * l1) >= 1.0)) return 0;         /* (N = 1: the Hann window of one tap is 0) */
  return 1;
}
static int cqt_half(const pdmp3_amd_cqt_spec* s, long sr, int k) { return (int)floor(0.5 * cqt_len(s, sr, k)); }
static long long cqt_table_rows(const pdmp3_amd_cqt_spec* s, long sr) {
  long long rows = 0;
  for (int k = 0; k < s->n_bins; k += 16) rows += (2 * cqt_half(s, sr, k) + 1 + 3) & ~3;
  return rows;
}

/* the LDS of a workgroup with `tile` frames: the tile's span in chunks of hop + row_pad floats, then the partial sums */
HOST_LOCAL void cqt_lds(int rows0, int hop, int tile, int row_pad, unsigned* span_floats, unsigned* bytes) {
  const unsigned span = (unsigned)(tile - 1) * (unsigned)hop + (unsigned)rows0;
  const unsigned a = (((span + (unsigned)hop - 1u) / (unsigned)hop) * (unsigned)(hop + row_pad) + 3u) & ~3u;
  *span_floats = a;
  *bytes = (a + (unsigned)PDMP3_CQT_PART_FLOATS) * 4u;
}
HOST_LOCAL int cqt_plan(const pdmp3_amd_cqt_spec* s, long sr, pdmp3_cqt_params* p) {
  if (!cqt_numbers_ok(s, sr) || cqt_table_rows(s, sr) * 32 > CQT_TABLE_MAX) return -1;
  memset(p, 0, sizeof *p);
  const int h0 = cqt_half(s, sr, 0);
  p->n_bins = s->n_bins; p->n_tiles = (s->n_bins + 15) / 16;
  p->hop = s->hop; p->row_pad = (int)((2u - (unsigned)s->hop) & 31u);
  p->out_mode = s->out_mode;
  uint32_t at = 0;
  for (int t = 0; t < p->n_tiles; t++) {
    const int h = cqt_half(s, sr, 16 * t);
    p->tile_rows[t] = (2 * h + 1 + 3) & ~3;
    p->tile_base[t] = h0 - h;
    p->tile_at[t] = at;
    at += (uint32_t)p->tile_rows[t];
    if (p->tile_rows[t] >= PDMP3_CQT_SPLIT_ROWS) p->n_split = t + 1;     /* (the rows descend: the split tiles are the first ones) */
  }
  p->rows0 = p->tile_rows[0]; p->half0 = h0;
  static const int tiles[3] = {16, 8, 4};
  for (int i = 0; i < 3; i++) {
    p->tile = tiles[i];
    cqt_lds(p->rows0, s->hop, p->tile, p->row_pad, &p->span_floats, &p->lds_bytes);
    if (p->lds_bytes <= PDMP3_MEL_LDS_MAX) return 0;
  }
  return -1;
}

int pdmp3_amd_cqt_check(const pdmp3_amd_cqt_spec* s, long sr) {
  pdmp3_cqt_params p;
  return cqt_plan(s, sr, &p);
}

int pdmp3_amd_cqt_plan(const pdmp3_amd_cqt_spec* s, long sr, int* tile, int* row_pad, unsigned* lds_bytes, int* split_rows, int* segments,
                       int* n_split) {
  pdmp3_cqt_params p;
  if (cqt_plan(s, sr, &p) != 0) return -1;
  if (tile) *tile = p.tile;
  if (row_pad) *row_pad = p.row_pad;
  if (lds_bytes) *lds_bytes = p.lds_bytes;
  if (split_rows) *split_rows = PDMP3_CQT_SPLIT_ROWS;
  if (segments) *segments = PDMP3_CQT_SEGMENTS;
  if (n_split) *n_split = p.n_split;
  return 0;
}

int pdmp3_amd_cqt_lengths(const pdmp3_amd_cqt_spec* s, long sr, double* f, int* half, size_t cap) {
  if (pdmp3_amd_cqt_check(s, sr) != 0 || cap < (size_t)s->n_bins) return -1;
  for (int k = 0; k < s->n_bins; k++) {
    if (f) f[k] = cqt_freq(s, k);
    if (half) half[k] = cqt_half(s, sr, k);
  }
  return s->n_bins;
}

/* (the caller has checked the spec; t holds the plan's rows x 32 floats) */
HOST_LOCAL void cqt_table_fill(const pdmp3_amd_cqt_spec* s, long sr, const pdmp3_cqt_params* p, float* t) {
  const double pi = 3.14159265358979323846;
  memset(t, 0, ((size_t)p->tile_at[p->n_tiles - 1] + (size_t)p->tile_rows[p->n_tiles - 1]) * 32 * sizeof *t);
  for (int k = 0; k < s->n_bins; k++) {
    const int tile = k >> 4, ht = cqt_half(s, sr, 16 * tile), h = cqt_half(s, sr, k), n = 2 * h + 1;
    const double fk = cqt_freq(s, k), len = cqt_len(s, sr, k);
    double sum = 0.0, sum2 = 0.0;
    for (int m = -h; m <= h; m++) {
      const double g = 0.5 - 0.5 * cos(2.0 * pi * (double)(m + h) / (double)n);
      sum += g; sum2 += g * g;
    }
    const double nk = s->norm == 1 ? 1.0 / sum : s->norm == 2 ? 1.0 / sqrt(sum2) : 1.0;
    const double ak = s->scale == 1 ? sqrt(len) : s->scale == 2 ? len : 1.0;
    const double sk = nk * ak;
    float* col = t + (size_t)p->tile_at[tile] * 32 + (k & 15);
    for (int m = -h; m <= h; m++) {
      const double g = 0.5 - 0.5 * cos(2.0 * pi * (double)(m + h) / (double)n);
      double x = (double)m * fk / (double)sr;      /* the angle in turns, reduced modulo 1 before the multiplication by 2 pi */
      x -= floor(x);
      const double a = 2.0 * pi * x;
      float* row = col + (size_t)(ht + m) * 32;
      row[0] = (float)(sk * g * cos(a));
      row[16] = (float)(-(sk * g) * sin(a));
    }
  }
}

long long pdmp3_amd_cqt_table(const pdmp3_amd_cqt_spec* s, long sr, float* table, size_t cap, int* tile_rows, int* tile_offset) {
  pdmp3_cqt_params p;
  if (cqt_plan(s, sr, &p) != 0) return -1;
  const long long count = ((long long)p.tile_at[p.n_tiles - 1] + p.tile_rows[p.n_tiles - 1]) * 32;
  if (table && (long long)cap < count) return -1;
  for (int t = 0; t < p.n_tiles; t++) {
    if (tile_rows) tile_rows[t] = p.tile_rows[t];
    if (tile_offset) tile_offset[t] = (int)p.tile_at[t];
  }
  if (table) cqt_table_fill(s, sr, &p, table);
  return count;
}

/* The decoder's table of the spec at sr.  At most PDMP3_CQT_TABLES are kept, the most recently used first; a new one takes
 * the place of the least recently used.  The key is every number that enters the table. */
HOST_LOCAL const float* cqt_table(struct bulk* b, const pdmp3_amd_cqt_spec* s, long sr, const pdmp3_cqt_params* p) {
  cqt_tab* prev = NULL;
  cqt_tab* last_prev = NULL;
  int n = 0;
  for (cqt_tab* t = b->cqt_tabs; t; prev = t, t = t->next) {
    n++;
    if (t->sr == sr && t->n_bins == s->n_bins && t->bpo == s->bins_per_octave && t->norm == s->norm && t->scale == s->scale &&
        t->fmin == s->fmin && t->filter_scale == s->filter_scale) {
      if (prev) { prev->next = t->next; t->next = b->cqt_tabs; b->cqt_tabs = t; }
      return t->t;
    }
    if (t->next) last_prev = t;
  }
  cqt_tab* t;
  if (n >= PDMP3_CQT_TABLES) {                       /* the last of the list leaves it and is filled anew */
    t = last_prev ? last_prev->next : b->cqt_tabs;
    if (last_prev) last_prev->next = NULL; else b->cqt_tabs = NULL;
    free(t->t);
    memset(t, 0, sizeof *t);
  } else {
    t = (cqt_tab*)calloc(1, sizeof *t);
    if (!t) return NULL;
  }
  t->sr = sr; t->n_bins = s->n_bins; t->bpo = s->bins_per_octave; t->norm = s->norm; t->scale = s->scale;
  t->fmin = s->fmin; t->filter_scale = s->filter_scale;
  t->t = (float*)malloc(((size_t)p->tile_at[p->n_tiles - 1] + (size_t)p->tile_rows[p->n_tiles - 1]) * 32 * sizeof(float));
  if (!t->t) { free(t); return NULL; }
  cqt_table_fill(s, sr, p, t->t);
  t->next = b->cqt_tabs;
  b->cqt_tabs = t;
  return t->t;
}
