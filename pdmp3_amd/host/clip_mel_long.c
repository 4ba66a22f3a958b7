/* clip_mel_long.c -- libpdmp3.so: the planning of log-mel features of clips at n_fft 2048 and 4096 (include/pdmp3_bulk.h
 * pdmp3_amd_mel_long_*): the check, the filterbank on the wider domain, the operand in the order
 * k_clip_mel_long meets the bins, the kernel's tile.  The filterbank's arithmetic is clip_mel.c's (mel_fb_fill), the four
 * transform tables are clip_stft_long.c's; no GPU.  The call itself (pdmp3_amd_bulk_decode_clips_mel_long) is clip_features.c's. */
#include "bulk_internal.h"

static int mell_fft_ok(int n_fft) { return n_fft == 2048 || n_fft == 4096; }

HOST_LOCAL void mel_long_stft_spec(const pdmp3_amd_mel_long_spec* s, pdmp3_amd_stft_spec* t) {
  memset(t, 0, sizeof *t);
  t->n_fft = s->mel.n_fft; t->hop = s->mel.hop;
  t->win_length = s->win_length; t->window = s->window;
  t->out_mode = 2;
}

int pdmp3_amd_mel_long_check(const pdmp3_amd_mel_long_spec* s, long sr) {
  if (!s || !mell_fft_ok(s->mel.n_fft) || s->mel.hop < 1 || s->mel.hop > s->mel.n_fft || s->mel.out_mode > 2) return -1;
  /* the bands, the frequencies, scale, norm, floor, n_frames and sr: section 10's limits, by section 10's check */
  pdmp3_amd_mel_spec m = s->mel;
  m.n_fft = 1024; m.hop = 1;
  if (pdmp3_amd_mel_check(&m, sr) != 0) return -1;
  /* win_length and the window's values: section 14's */
  pdmp3_amd_stft_spec t;
  mel_long_stft_spec(s, &t);
  return pdmp3_amd_stft_long_check(&t, sr);
}

long long pdmp3_amd_mel_long_filterbank(long sr, int n_fft, int n_mels, double f_min, double f_max, int scale, int norm, float* w, size_t cap) {
  pdmp3_amd_mel_long_spec s;
  memset(&s, 0, sizeof s);
  s.mel.n_fft = n_fft; s.mel.hop = 1; s.mel.n_mels = n_mels; s.mel.f_min = f_min; s.mel.f_max = f_max; s.mel.scale = scale; s.mel.norm = norm;
  s.mel.floor = 1.0;
  if (pdmp3_amd_mel_long_check(&s, sr) != 0) return -1;
  const long long count = (long long)n_mels * (n_fft / 2 + 1);
  if (w && cap) {
    if ((size_t)count <= cap) { if (mel_fb_fill(sr, n_fft, n_mels, f_min, f_max, scale, norm, w) != 0) return -1; }
    else {
      float* t = (float*)malloc((size_t)count * sizeof *t);
      if (!t || mel_fb_fill(sr, n_fft, n_mels, f_min, f_max, scale, norm, t) != 0) { free(t); return -1; }
      memcpy(w, t, cap * sizeof *t);
      free(t);
    }
  }
  return count;
}

/* The order of the bins (csrc/mel_long_core.h has the same numbers for the kernel): bin k = 16 kt + k1l + 64 k2 lies in row
 * 8 N2 kt + slot(k1l, k2). */
static int mell_row(int kt, int k1l, int k2, int n2) {
  return 8 * n2 * kt + 32 * (((k1l & 3) | ((k1l >> 3) << 2)) * (n2 >> 5) + (k2 >> 4)) + 16 * ((k1l >> 2) & 1) + (k2 & 15);
}
/* op [N / 2][mels16] from the dense w [n_mels][N / 2 + 1]: a permutation of the columns 0 .. N / 2 - 1, zeros in the bands'
 * padding; column N / 2 -- exactly 0 for every spec the check accepts -- is left out */
static void mell_operand_fill(int n_fft, int n_mels, const float* w, float* op) {
  const int n2 = n_fft / 64, K = n_fft / 2 + 1, mp = (n_mels + 15) & ~15;
  memset(op, 0, (size_t)(n_fft / 2) * (size_t)mp * sizeof *op);
  for (int kt = 0; kt < 4; kt++)
    for (int k1l = 0; k1l < 16; k1l++)
      for (int k2 = 0; k2 < n2 / 2; k2++) {
        const int k = 16 * kt + k1l + 64 * k2;
        float* row = op + (size_t)mell_row(kt, k1l, k2, n2) * (size_t)mp;
        for (int m = 0; m < n_mels; m++) row[m] = w[(size_t)m * (size_t)K + (size_t)k];
      }
}

long long pdmp3_amd_mel_long_operand(long sr, int n_fft, int n_mels, double f_min, double f_max, int scale, int norm, float* op, size_t cap,
                                     int* rows, int* cols) {
  const long long dense = pdmp3_amd_mel_long_filterbank(sr, n_fft, n_mels, f_min, f_max, scale, norm, NULL, 0);
  if (dense < 0) return -1;
  const int mp = (n_mels + 15) & ~15;
  const long long count = (long long)(n_fft / 2) * mp;
  if (rows) *rows = n_fft / 2;
  if (cols) *cols = mp;
  if (op && cap) {
    float* w = (float*)malloc((size_t)dense * sizeof *w);
    float* t = (float*)malloc((size_t)count * sizeof *t);
    if (!w || !t || mel_fb_fill(sr, n_fft, n_mels, f_min, f_max, scale, norm, w) != 0) { free(w); free(t); return -1; }
    mell_operand_fill(n_fft, n_mels, w, t);
    memcpy(op, t, ((size_t)count < cap ? (size_t)count : cap) * sizeof *t);
    free(w); free(t);
  }
  return count;
}

/* The LDS of a workgroup with `tile` frames: the tile's span, (tile - 1) hop + N floats rounded up to 4, which stays for all
 * four tiles of k1; then Z, tile x N2 x 32 floats; then the powers of one tile of k1, tile x (8 N2 + 2) floats.  The
 * accumulators live in registers and the rows leave from them: nothing else.
 * 16 frames where that fits the LDS of a workgroup, else 8, else 4.  By this arithmetic N 2048 takes 16 frames up to hop
 * 1225 and 8 beyond (104 KB at hop 2048); N 4096 never fits 16, takes 8 up to hop 2336 and 4 beyond (104 KB at hop 4096).
 * n_mels does not enter.  These four (N2, tile) pairs are the kernel's launch paths. */
HOST_LOCAL int mel_long_plan(int n_fft, int hop, int n_mels, pdmp3_mel_long_params* p) {
  if (!mell_fft_ok(n_fft) || hop < 1 || hop > n_fft || n_mels < 1 || n_mels > 256) return -1;
  const unsigned n2 = (unsigned)n_fft / 64u;
  p->n_fft = n_fft; p->n2 = (int32_t)n2;
  p->hop = hop; p->n_mels = n_mels; p->mels16 = (n_mels + 15) & ~15;
  for (int tile = 16; tile >= 4; tile >>= 1) {
    p->tile = tile;
    p->span_floats = ((unsigned)(tile - 1) * (unsigned)hop + (unsigned)n_fft + 3u) & ~3u;
    p->lds_bytes = (p->span_floats + (unsigned)tile * n2 * 32u + (unsigned)tile * (8u * n2 + 2u)) * 4u;
    if (p->lds_bytes <= PDMP3_MEL_LDS_MAX) return 0;
  }
  return -1;
}
int pdmp3_amd_mel_long_plan(int n_fft, int hop, int n_mels, int* tile, int* row_pad, unsigned* lds_bytes) {
  pdmp3_mel_long_params p;
  memset(&p, 0, sizeof p);
  if (mel_long_plan(n_fft, hop, n_mels, &p) != 0) return -1;
  if (tile) *tile = p.tile;
  if (row_pad) *row_pad = 0;                         /* (the span lies plain in LDS, as section 14's) */
  if (lds_bytes) *lds_bytes = p.lds_bytes;
  return 0;
}

/* The decoder's operand of a spec the check accepts at sr: made once per (sr, N, n_mels, f_min, f_max, scale, norm), kept for
 * the decoder's life in the list of section 10's tables (fb == 2 there).  NULL: no memory. */
HOST_LOCAL const float* mel_long_operand(struct bulk* b, long sr, const pdmp3_amd_mel_spec* s) {
  for (mel_tab* t = b->mel_tabs; t; t = t->next)
    if (t->fb == 2 && t->n_fft == s->n_fft && t->sr == sr && t->n_mels == s->n_mels && t->f_min == s->f_min && t->f_max == s->f_max &&
        t->scale == s->scale && t->norm == s->norm)
      return t->t;
  const int K = s->n_fft / 2 + 1, mp = (s->n_mels + 15) & ~15;
  mel_tab* t = (mel_tab*)calloc(1, sizeof *t);
  if (!t) return NULL;
  t->fb = 2; t->n_fft = s->n_fft; t->sr = sr; t->n_mels = s->n_mels; t->f_min = s->f_min; t->f_max = s->f_max; t->scale = s->scale; t->norm = s->norm;
  float* w = (float*)malloc((size_t)s->n_mels * (size_t)K * sizeof(float));
  t->t = (float*)malloc((size_t)(s->n_fft / 2) * (size_t)mp * sizeof(float));
  if (w && t->t && mel_fb_fill(sr, s->n_fft, s->n_mels, s->f_min, s->f_max, s->scale, s->norm, w) == 0) mell_operand_fill(s->n_fft, s->n_mels, w, t->t);
  else { free(t->t); t->t = NULL; }
  free(w);
  if (!t->t) { free(t); return NULL; }
  t->next = b->mel_tabs;
  b->mel_tabs = t;
  return t->t;
}
