/* clip_stft.c -- libpdmp3.so: the planning of the short-time Fourier transform of clips (include/pdmp3_bulk.h
 * pdmp3_amd_stft_*): the check, the folded table (window and scale in the DFT's coefficients), the
 * kernel's tile and the decoder's small cache of tables.  Plain arithmetic in binary64, no GPU; the call itself
 * (pdmp3_amd_bulk_decode_clips_stft) is clip_features.c's. */
#include "bulk_internal.h"

#include <float.h>
#include <math.h>

static int stft_fft_ok(int n_fft) { return n_fft >= 16 && n_fft <= 1024 && !(n_fft & 1); }
static int stft_frame_ok(const pdmp3_amd_stft_spec* s) {
  if (!s || !stft_fft_ok(s->n_fft) || s->win_length < 0 || s->win_length > s->n_fft) return 0;
  if (s->normalized != 0 && s->normalized != 1) return 0;
  if (s->window) {
    const int nw = s->win_length ? s->win_length : s->n_fft;
    for (int i = 0; i < nw; i++) if (!isfinite(s->window[i])) return 0;
  }
  return 1;
}

int pdmp3_amd_stft_check(const pdmp3_amd_stft_spec* s, long sr) {
  if (!s || sr <= 0 || sr > 0x7fffffffL) return -1;
  if (!stft_frame_ok(s) || s->hop < 1 || s->hop > s->n_fft || s->n_frames < 0 || s->out_mode < 0 || s->out_mode > 4) return -1;
  if (s->out_mode >= 3 && (!(s->floor > 0.0) || !((float)s->floor >= FLT_MIN) || !(s->floor <= (double)FLT_MAX))) return -1;
  return 0;
}

/* (the caller has checked the frame) */
HOST_LOCAL void stft_table_fill(const pdmp3_amd_stft_spec* s, float* t) {
  const double pi = 3.14159265358979323846;
  const int N = s->n_fft, Nw = s->win_length ? s->win_length : N, K = N / 2 + 1, Kp = (K + 15) & ~15, rows = (N + 3) & ~3;
  const int left = (N - Nw) / 2;
  const double scale = s->normalized ? 1.0 / sqrt((double)N) : 1.0;
  memset(t, 0, (size_t)rows * (size_t)(2 * Kp) * sizeof *t);
  for (int i = 0; i < Nw; i++) {
    const int n = left + i;
    const double w = scale * (s->window ? (double)s->window[i] : 0.5 - 0.5 * cos(2.0 * pi * (double)i / (double)Nw));
    float* row = t + (size_t)n * (size_t)(2 * Kp);
    for (int k = 0; k < K; k++) {
      const double a = 2.0 * pi * (double)(((long)k * n) % N) / (double)N;
      row[k] = (float)(w * cos(a));
      row[Kp + k] = (float)(-w * sin(a));
    }
  }
}

long long pdmp3_amd_stft_table(const pdmp3_amd_stft_spec* s, float* table, size_t cap, int* rows, int* cols) {
  if (!stft_frame_ok(s)) return -1;
  const int K = s->n_fft / 2 + 1, Kp = (K + 15) & ~15, r = (s->n_fft + 3) & ~3;
  const long long count = (long long)r * (2 * Kp);
  if (rows) *rows = r;
  if (cols) *cols = 2 * Kp;
  if (table && cap) {
    if ((size_t)count <= cap) stft_table_fill(s, table);
    else {
      float* t = (float*)malloc((size_t)count * sizeof *t);
      if (!t) return -1;
      stft_table_fill(s, t);
      memcpy(table, t, cap * sizeof *t);
      free(t);
    }
  }
  return count;
}

/* the LDS of a workgroup with `tile` frames: the tile's span in chunks of hop + row_pad floats, then a staging tile a wave:
 * one plane (mode 0: two, Re and Im) of 16 bins by tile + 4 floats */
static void stft_lds(int n_fft, int hop, int out_mode, int tile, int row_pad, unsigned* span_floats, unsigned* bytes) {
  const unsigned rows = ((unsigned)n_fft + 3u) & ~3u;
  const unsigned span = (unsigned)(tile - 1) * (unsigned)hop + rows;
  const unsigned a = (((span + (unsigned)hop - 1u) / (unsigned)hop) * (unsigned)(hop + row_pad) + 3u) & ~3u;
  *span_floats = a;
  *bytes = (a + 4u * (out_mode == 0 ? 2u : 1u) * 16u * (unsigned)(tile + 4)) * 4u;
}
HOST_LOCAL int stft_plan(int n_fft, int hop, int out_mode, pdmp3_stft_params* p) {
  if (!stft_fft_ok(n_fft) || hop < 1 || hop > n_fft || out_mode < 0 || out_mode > 4) return -1;
  p->n_fft = n_fft; p->rows = (n_fft + 3) & ~3;
  p->hop = hop; p->row_pad = (int)((2u - (unsigned)hop) & 31u);
  p->bins = n_fft / 2 + 1; p->bins16 = (p->bins + 15) & ~15;
  p->out_mode = out_mode;
  p->tile = 32;
  stft_lds(n_fft, hop, out_mode, 32, p->row_pad, &p->span_floats, &p->lds_bytes);
  if (p->lds_bytes > PDMP3_MEL_LDS_SOFT) {
    p->tile = 16;
    stft_lds(n_fft, hop, out_mode, 16, p->row_pad, &p->span_floats, &p->lds_bytes);
  }
  return p->lds_bytes <= PDMP3_MEL_LDS_MAX ? 0 : -1;
}
int pdmp3_amd_stft_tile(int n_fft, int hop, int out_mode, int* tile, int* row_pad, unsigned* lds_bytes) {
  pdmp3_stft_params p;
  memset(&p, 0, sizeof p);
  if (stft_plan(n_fft, hop, out_mode, &p) != 0) return -1;
  if (tile) *tile = p.tile;
  if (row_pad) *row_pad = p.row_pad;
  if (lds_bytes) *lds_bytes = p.lds_bytes;
  return 0;
}

/* The decoder's folded table of the spec's frame.  At most PDMP3_STFT_TABLES are kept, the most recently used first; a new
 * one takes the place of the least recently used.  The key is (N, Nw, normalized, the window's values): the stored copy of
 * the window is compared, never the caller's pointer. */
HOST_LOCAL const float* stft_table(struct bulk* b, const pdmp3_amd_stft_spec* s) {
  const int N = s->n_fft, Nw = s->win_length ? s->win_length : N, K = N / 2 + 1, Kp = (K + 15) & ~15;
  stft_tab* prev = NULL;
  stft_tab* last_prev = NULL;
  int n = 0;
  for (stft_tab* t = b->stft_tabs; t; prev = t, t = t->next) {
    n++;
    if (t->n_fft == N && t->win == Nw && t->normalized == s->normalized && !t->window == !s->window &&
        (!s->window || memcmp(t->window, s->window, (size_t)Nw * sizeof(float)) == 0)) {
      if (prev) { prev->next = t->next; t->next = b->stft_tabs; b->stft_tabs = t; }
      return t->t;
    }
    if (t->next) last_prev = t;
  }
  stft_tab* t;
  if (n >= PDMP3_STFT_TABLES) {                      /* the last of the list leaves it and is filled anew */
    t = last_prev ? last_prev->next : b->stft_tabs;
    if (last_prev) last_prev->next = NULL; else b->stft_tabs = NULL;
    free(t->t); free(t->window);
    memset(t, 0, sizeof *t);
  } else {
    t = (stft_tab*)calloc(1, sizeof *t);
    if (!t) return NULL;
  }
  t->n_fft = N; t->win = Nw; t->normalized = s->normalized;
  t->t = (float*)malloc((size_t)((N + 3) & ~3) * (size_t)(2 * Kp) * sizeof(float));
  if (s->window) {
    t->window = (float*)malloc((size_t)Nw * sizeof(float));
    if (t->window) memcpy(t->window, s->window, (size_t)Nw * sizeof(float));
  }
  if (!t->t || (s->window && !t->window)) { free(t->t); free(t->window); free(t); return NULL; }
  stft_table_fill(s, t->t);
  t->next = b->stft_tabs;
  b->stft_tabs = t;
  return t->t;
}
