/* clip_mfcc.c -- libpdmp3.so: the planning of Kaldi-style MFCC features of clips (include/pdmp3_bulk.h pdmp3_amd_mfcc_*;
 * DESIGN.md section 12): the check, the DCT table with the lifter, htk_compat's sqrt 2 and the column order folded in, and the
 * kernel's tile.  Plain arithmetic in binary64, no GPU; the call itself (pdmp3_amd_bulk_decode_clips_mfcc) is clip_features.c's. */
#include "bulk_internal.h"

#include <math.h>

static int mfcc_dct_ok(const pdmp3_amd_mfcc_spec* s) {
  if (!s || s->fbank.n_mels < 1 || s->fbank.n_mels > 256 || s->num_ceps < 1 || s->num_ceps > s->fbank.n_mels) return 0;
  if ((s->fbank.use_energy & ~1) || (s->fbank.htk_compat & ~1)) return 0;
  return isfinite(s->cepstral_lifter) && s->cepstral_lifter >= 0.0;
}

int pdmp3_amd_mfcc_check(const pdmp3_amd_mfcc_spec* s, long sr) {
  if (!s || pdmp3_amd_fbank_check(&s->fbank, sr) != 0) return -1;
  if (s->fbank.out_mode != 1) return -1;               /* (there is no power mode) */
  return mfcc_dct_ok(s) ? 0 : -1;
}

HOST_LOCAL void mfcc_dct_fill(const pdmp3_amd_mfcc_spec* s, float* t) {
  const double pi = 3.14159265358979323846;
  const int Nm = s->fbank.n_mels, nc = s->num_ceps, Mp = (Nm + 15) & ~15, Cp = (nc + 15) & ~15;
  const double Q = s->cepstral_lifter;
  memset(t, 0, (size_t)Mp * (size_t)Cp * sizeof *t);
  for (int col = 0; col < nc; col++) {
    /* the cepstral index the column holds */
    const int c = !s->fbank.htk_compat ? col : col == nc - 1 ? 0 : col + 1;
    if (c == 0 && s->fbank.use_energy) continue;       /* (the energy's column: zeros) */
    const double lift = Q > 0.0 ? 1.0 + 0.5 * Q * sin(pi * (double)c / Q) : 1.0;
    const double root2 = c == 0 && s->fbank.htk_compat ? sqrt(2.0) : 1.0;
    for (int m = 0; m < Nm; m++) {
      const double v = c == 0 ? sqrt(1.0 / (double)Nm) : sqrt(2.0 / (double)Nm) * cos(pi * ((double)m + 0.5) * (double)c / (double)Nm);
      t[(size_t)m * (size_t)Cp + (size_t)col] = (float)(lift * root2 * v);
    }
  }
}

long long pdmp3_amd_mfcc_dct_table(const pdmp3_amd_mfcc_spec* s, float* table, size_t cap, int* rows, int* cols) {
  if (!mfcc_dct_ok(s)) return -1;
  const int Mp = (s->fbank.n_mels + 15) & ~15, Cp = (s->num_ceps + 15) & ~15;
  const long long count = (long long)Mp * Cp;
  if (rows) *rows = Mp;
  if (cols) *cols = Cp;
  if (table && cap) {
    if ((size_t)count <= cap) mfcc_dct_fill(s, table);
    else {
      float* t = (float*)malloc((size_t)count * sizeof *t);
      if (!t) return -1;
      mfcc_dct_fill(s, t);
      memcpy(table, t, cap * sizeof *t);
      free(t);
    }
  }
  return count;
}

/* fbank_plan's arithmetic (clip_fbank.c) with the second region the powers and the cepstra share: the larger of
 * [tile][bins16 + 2] and [tile][ceps16 + 1] */
static void mfcc_lds(const pdmp3_mfcc_params* q, int tile, unsigned* span_floats, unsigned* bytes) {
  const pdmp3_fbank_params* p = &q->fb;
  const unsigned span = (unsigned)(tile - 1) * (unsigned)p->hop + (unsigned)p->rows;
  unsigned a = ((span + (unsigned)p->hop - 1u) / (unsigned)p->hop) * (unsigned)(p->hop + p->row_pad);
  const unsigned mt = (unsigned)p->mels16 * (unsigned)(tile + 1);
  const unsigned pw = (unsigned)p->bins16 + 2u, ct = (unsigned)q->ceps16 + 1u;
  if (mt > a) a = mt;
  a = (a + 3u) & ~3u;
  *span_floats = a;
  *bytes = (a + (unsigned)tile * (pw > ct ? pw : ct)) * 4u;
}
HOST_LOCAL int mfcc_plan(int win, int n_dft, int hop, int n_mels, int n_ceps, pdmp3_mfcc_params* q) {
  pdmp3_fbank_params* p = &q->fb;
  if (n_ceps < 1 || n_ceps > n_mels) return -1;
  /* the sizes and row_pad are the filterbank kernel's; the tile follows from this kernel's own bytes */
  if (fbank_plan(win, n_dft, hop, n_mels, p) != 0) return -1;
  q->n_ceps = n_ceps; q->ceps16 = (n_ceps + 15) & ~15;
  p->tile = 32;
  mfcc_lds(q, 32, &p->span_floats, &p->lds_bytes);
  if (p->lds_bytes > PDMP3_MEL_LDS_SOFT) {
    p->tile = 16;
    mfcc_lds(q, 16, &p->span_floats, &p->lds_bytes);
  }
  return p->lds_bytes <= PDMP3_MEL_LDS_MAX ? 0 : -1;
}
int pdmp3_amd_mfcc_tile(int win_length, int n_dft, int hop, int n_mels, int num_ceps, int* tile, int* row_pad, unsigned* lds_bytes) {
  pdmp3_mfcc_params q;
  memset(&q, 0, sizeof q);
  if (mfcc_plan(win_length, n_dft, hop, n_mels, num_ceps, &q) != 0) return -1;
  if (tile) *tile = q.fb.tile;
  if (row_pad) *row_pad = q.fb.row_pad;
  if (lds_bytes) *lds_bytes = q.fb.lds_bytes;
  return 0;
}
