/* clip_mfcc_long.c -- libpdmp3.so: the planning of librosa-style MFCC, deltas and dB mel of clips at n_fft 2048 and 4096
 * (include/pdmp3_bulk.h pdmp3_amd_mfcc_long_*): the check, the DCT table with the lifter folded in, the
 * delta taps, the frames a clip is widened by and the kernel's tile.  The log-mel's rules are clip_mel_long.c's.  Plain
 * arithmetic in binary64, no GPU; the call itself (pdmp3_amd_bulk_decode_clips_mfcc_long) is clip_features.c's. */
#include "bulk_internal.h"

#include <math.h>

static int mfl_width_ok(int w) { return w >= 3 && w <= PDMP3_MFCC_LONG_MAX_WIDTH && (w & 1); }
static int mfl_dct_ok(int n_mels, int n_mfcc, double lifter) {
  if (n_mels < 1 || n_mels > 256 || n_mfcc < 1 || n_mfcc > n_mels || n_mfcc > PDMP3_MFCC_LONG_MAX_CEPS) return 0;
  return isfinite(lifter) && lifter >= 0.0;
}
/* the frames in front of frame 0 and behind frame F - 1 */
static int mfl_halo(const pdmp3_amd_mfcc_long_spec* s) { return s->out_mode == 0 && s->deltas > 0 ? (s->delta_width - 1) / 2 : 0; }

int pdmp3_amd_mfcc_long_check(const pdmp3_amd_mfcc_long_spec* s, long sr) {
  if (!s) return -1;
  pdmp3_amd_mel_long_spec m = s->mel;
  m.mel.out_mode = 2;
  if (pdmp3_amd_mel_long_check(&m, sr) != 0) return -1;
  if (isnan(s->top_db) || (s->top_db > 0.0 && isinf(s->top_db))) return -1;
  if (s->out_mode != 0 && s->out_mode != 1) return -1;
  const long long F = m.mel.n_frames, Nm = m.mel.n_mels;
  if (F < 0) return -1;
  long long rows = Nm;
  if (s->out_mode == 0) {
    if (!mfl_dct_ok(m.mel.n_mels, s->n_mfcc, s->lifter) || s->deltas < 0 || s->deltas > 2) return -1;
    if (s->deltas > 0 && !mfl_width_ok(s->delta_width)) return -1;
    rows = (long long)(1 + s->deltas) * s->n_mfcc;
  }
  /* a channel's row of the output and of the stage inside 31 bits */
  if (F > 0x7fffffffLL / rows || F + 2 * mfl_halo(s) > 0x7fffffffLL / Nm) return -1;
  return 0;
}

static void mfl_dct_fill(int n_mels, int n_mfcc, double lifter, float* t) {
  const double pi = 3.14159265358979323846;
  const int Mp = (n_mels + 15) & ~15, Cp = (n_mfcc + 15) & ~15;
  memset(t, 0, (size_t)Mp * (size_t)Cp * sizeof *t);
  for (int q = 0; q < n_mfcc; q++) {
    const double lift = lifter > 0.0 ? 1.0 + 0.5 * lifter * sin(pi * (double)(q + 1) / lifter) : 1.0;
    const double sq = q == 0 ? sqrt(1.0 / (double)n_mels) : sqrt(2.0 / (double)n_mels);
    for (int m = 0; m < n_mels; m++)
      t[(size_t)q * (size_t)Mp + (size_t)m] = (float)(sq * cos(pi * (double)q * (double)(2 * m + 1) / (double)(2 * n_mels)) * lift);
  }
}

long long pdmp3_amd_mfcc_long_dct_table(int n_mels, int n_mfcc, double lifter, float* table, size_t cap, int* rows, int* cols) {
  if (!mfl_dct_ok(n_mels, n_mfcc, lifter)) return -1;
  const int Mp = (n_mels + 15) & ~15, Cp = (n_mfcc + 15) & ~15;
  const long long count = (long long)Mp * Cp;
  if (rows) *rows = Cp;
  if (cols) *cols = Mp;
  if (table && cap) {
    if ((size_t)count <= cap) mfl_dct_fill(n_mels, n_mfcc, lifter, table);
    else {
      float* t = (float*)malloc((size_t)count * sizeof *t);
      if (!t) return -1;
      mfl_dct_fill(n_mels, n_mfcc, lifter, t);
      memcpy(table, t, cap * sizeof *t);
      free(t);
    }
  }
  return count;
}

/* j, S2 and S4 are small integers, exact in binary64; every tap is a few roundings of its rational value */
static void mfl_taps_fill(int w, double* t1, double* t2) {
  const int h = (w - 1) / 2;
  double s2 = 0.0, s4 = 0.0;
  for (int j = -h; j <= h; j++) { s2 += (double)(j * j); s4 += (double)(j * j) * (double)(j * j); }
  const double den = s4 - s2 * s2 / (double)w;
  for (int j = -h; j <= h; j++) {
    t1[j + h] = (double)j / s2;
    t2[j + h] = 2.0 * ((double)(j * j) - s2 / (double)w) / den;
  }
}
int pdmp3_amd_mfcc_long_delta_taps(int delta_width, double* taps, size_t cap) {
  if (!mfl_width_ok(delta_width)) return -1;
  if (!taps && !cap) return delta_width;
  if (!taps || cap < 2 * (size_t)delta_width) return -1;
  mfl_taps_fill(delta_width, taps, taps + delta_width);
  return delta_width;
}

/* One tile and one LDS layout for every shape (csrc/mfcc_long_core.h has the same numbers for the kernel): 64 frames, a lane
 * a frame; the plane of dB values [mels16][80] has room for the widest halo, 8 frames on both sides, and the plane of cepstra
 * [ceps16][84] is 4 floats wider.  At 256 bands and 128 cepstra that is (256 x 80 + 128 x 84) x 4 = 124 928 B, inside
 * PDMP3_MEL_LDS_MAX: no shape needs a smaller tile.  At librosa's 128 / 20 it is 51 712 B, three workgroups a CU. */
static int mfl_tile(int n_mels, int n_mfcc, pdmp3_mfcc_long_params* p) {
  p->n_mels = n_mels; p->mels16 = (n_mels + 15) & ~15;
  p->n_mfcc = n_mfcc; p->ceps16 = (n_mfcc + 15) & ~15;
  p->tile = 64;
  p->d_pitch = p->tile + PDMP3_MFCC_LONG_MAX_WIDTH - 1;
  p->c_pitch = p->d_pitch + 4;
  p->lds_bytes = ((uint32_t)p->mels16 * (uint32_t)p->d_pitch + (uint32_t)p->ceps16 * (uint32_t)p->c_pitch) * 4u;
  return p->lds_bytes <= PDMP3_MEL_LDS_MAX ? 0 : -1;
}
/* the geometry of a spec's numbers (0, or -1): the check's rules on them, the halo, the taps */
static int mfl_geometry(int n_mels, int n_mfcc, int deltas, int delta_width, int out_mode, pdmp3_mfcc_long_params* p) {
  memset(p, 0, sizeof *p);
  if (n_mels < 1 || n_mels > 256 || (out_mode != 0 && out_mode != 1)) return -1;
  p->out_mode = out_mode;
  if (out_mode == 1) {
    p->n_mels = n_mels; p->mels16 = (n_mels + 15) & ~15;
    p->tile = 1024;
    return 0;
  }
  if (!mfl_dct_ok(n_mels, n_mfcc, 0.0) || deltas < 0 || deltas > 2 || (deltas > 0 && !mfl_width_ok(delta_width))) return -1;
  if (mfl_tile(n_mels, n_mfcc, p) != 0) return -1;
  p->deltas = deltas;
  p->halo = deltas > 0 ? (delta_width - 1) / 2 : 0;
  if (deltas > 0) mfl_taps_fill(delta_width, p->taps[0], p->taps[1]);
  return 0;
}
int pdmp3_amd_mfcc_long_plan(int n_mels, int n_mfcc, int deltas, int delta_width, int out_mode, int* front, int* back, int* tile,
                             int* d_pitch, int* c_pitch, unsigned* lds_bytes) {
  pdmp3_mfcc_long_params p;
  if (mfl_geometry(n_mels, n_mfcc, deltas, delta_width, out_mode, &p) != 0) return -1;
  if (front) *front = p.halo;
  if (back) *back = p.halo;
  if (tile) *tile = p.tile;
  if (d_pitch) *d_pitch = p.d_pitch;
  if (c_pitch) *c_pitch = p.c_pitch;
  if (lds_bytes) *lds_bytes = p.lds_bytes;
  return 0;
}

HOST_LOCAL int mfcc_long_plan(const pdmp3_amd_mfcc_long_spec* s, long sr, pdmp3_mfcc_long_params* p, int* front, int* back) {
  if (pdmp3_amd_mfcc_long_check(s, sr) != 0) return -1;
  if (mfl_geometry(s->mel.mel.n_mels, s->n_mfcc, s->deltas, s->delta_width, s->out_mode, p) != 0) return -1;
  p->use_top = s->top_db >= 0.0;
  p->top_db = p->use_top ? (float)s->top_db : 0.0f;
  *front = *back = p->halo;
  return 0;
}

/* The decoder's table of (n_mels, n_mfcc, lifter): made once, kept for the decoder's life in a list of its own.  NULL: no
 * memory. */
HOST_LOCAL const float* mfcc_long_table(struct bulk* b, int n_mels, int n_mfcc, double lifter) {
  for (mfcc_long_tab* t = b->mfcc_long_tabs; t; t = t->next)
    if (t->n_mels == n_mels && t->n_mfcc == n_mfcc && t->lifter == lifter) return t->t;
  if (!mfl_dct_ok(n_mels, n_mfcc, lifter)) return NULL;
  mfcc_long_tab* t = (mfcc_long_tab*)calloc(1, sizeof *t);
  if (!t) return NULL;
  t->n_mels = n_mels; t->n_mfcc = n_mfcc; t->lifter = lifter;
  t->t = (float*)malloc((size_t)((n_mels + 15) & ~15) * (size_t)((n_mfcc + 15) & ~15) * sizeof(float));
  if (!t->t) { free(t); return NULL; }
  mfl_dct_fill(n_mels, n_mfcc, lifter, t->t);
  t->next = b->mfcc_long_tabs;
  b->mfcc_long_tabs = t;
  return t->t;
}
