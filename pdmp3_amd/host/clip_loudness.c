/* clip_loudness.c -- libpdmp3.so: the planning of the loudness of clips (include/pdmp3_bulk.h pdmp3_amd_loudness_*; DESIGN.md
 * section 18): the check, the K-weighting's coefficients at a rate, the tables of the device's blocked filter and the launch's
 * geometry.  Plain binary64 arithmetic, no GPU; the call itself (pdmp3_amd_bulk_decode_clips_loudness) is clip_features.c's. */
#include "bulk_internal.h"

#include <math.h>

#define LOUD_B PDMP3_LOUD_B

static int loud_rate_ok(long fs) { return fs >= 8000 && fs <= 192000; }

int pdmp3_amd_loudness_check(const pdmp3_amd_loudness_spec* s, long fs, int channels) {
  if (!s || !loud_rate_ok(fs) || (channels != 1 && channels != 2)) return -1;
  if (!isnan(s->target) && !(s->target >= -70.0 && s->target <= 0.0)) return -1;
  if (!(s->peak_limit >= 0.0) || !isfinite(s->peak_limit)) return -1;
  if ((s->dual_mono != 0 && s->dual_mono != 1) || (s->dual_mono && channels == 2)) return -1;
  return 0;
}

/* libebur128's parametrisation of the two biquads: coef = b1[3] a1[3] b2[3] a2[3] */
static void loud_coefficients(long fs, double* c) {
  const double pi = 3.14159265358979323846;
  {
    const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
    const double K = tan(pi * f0 / (double)fs), Vh = pow(10.0, G / 20.0), Vb = pow(Vh, 0.4996667741545416);
    const double a0 = 1.0 + K / Q + K * K;
    c[0] = (Vh + Vb * K / Q + K * K) / a0; c[1] = 2.0 * (K * K - Vh) / a0; c[2] = (Vh - Vb * K / Q + K * K) / a0;
    c[3] = 1.0; c[4] = 2.0 * (K * K - 1.0) / a0; c[5] = (1.0 - K / Q + K * K) / a0;
  }
  {
    const double f0 = 38.13547087602444, Q = 0.5003270373238773;
    const double K = tan(pi * f0 / (double)fs), a0 = 1.0 + K / Q + K * K;
    c[6] = 1.0; c[7] = -2.0; c[8] = 1.0;
    c[9] = 1.0; c[10] = 2.0 * (K * K - 1.0) / a0; c[11] = (1.0 - K / Q + K * K) / a0;
  }
}
int pdmp3_amd_loudness_coefficients(long fs, double* coef) {
  if (!loud_rate_ok(fs) || !coef) return -1;
  loud_coefficients(fs, coef);
  return 0;
}

/* one sample through the two biquads in transposed direct form II; s = (z1, z2 of H1, z1, z2 of H2) */
static double loud_step(const double* c, double* s, double x) {
  const double v = c[0] * x + s[0];
  s[0] = c[1] * x - c[4] * v + s[1];
  s[1] = c[2] * x - c[5] * v;
  const double y = c[6] * v + s[2];
  s[2] = c[7] * v - c[10] * y + s[3];
  s[3] = c[8] * v - c[11] * y;
  return y;
}

/* The tables, each by running the recurrence itself: the impulse response from rest (Hm), blocks without input from each unit
 * state (O, and the powers of Phi behind 64 k samples: products of the matrices would lose digits, Phi's entries being far
 * larger than its eigenvalues), a block with a unit sample at j from rest (R's column j). */
HOST_LOCAL void loud_tables_fill(long fs, pdmp3_loud_tables* t) {
  double c[12], s[4];
  loud_coefficients(fs, c);
  memset(t, 0, sizeof *t);
  memset(s, 0, sizeof s);
  for (int n = 0; n < LOUD_B; n++) {
    const float h = (float)loud_step(c, s, n == 0 ? 1.0 : 0.0);
    for (int i = n; i < LOUD_B; i++) t->Hm[i][i - n] = h;
  }
  for (int m = 0; m < 4; m++) {
    memset(s, 0, sizeof s);
    s[m] = 1.0;
    t->pow[0][m * 4 + m] = 1.0;
    for (int i = 0; i < LOUD_B; i++) t->O[i][m] = (float)loud_step(c, s, 0.0);
    for (int k = 1, at = 1; k < PDMP3_LOUD_POWS; k++) {            /* pow[k] = Phi^at: at = k to 64, then doubled */
      for (int r = 0; r < 4; r++) t->pow[k][r * 4 + m] = s[r];
      const int next = k < PDMP3_LOUD_CHUNK ? at + 1 : 2 * at;
      if (k + 1 < PDMP3_LOUD_POWS)
        for (long i = (long)at * LOUD_B; i < (long)next * LOUD_B; i++) (void)loud_step(c, s, 0.0);
      at = next;
    }
  }
  for (int j = 0; j < LOUD_B; j++) {
    memset(s, 0, sizeof s);
    for (int i = 0; i < LOUD_B; i++) (void)loud_step(c, s, i == j ? 1.0 : 0.0);
    for (int r = 0; r < 4; r++) t->R[r][j] = s[r];
  }
}

int pdmp3_amd_loudness_tables(long fs, float* Hm, float* O, double* Phi, double* R, double* pows) {
  if (!loud_rate_ok(fs)) return -1;
  pdmp3_loud_tables* t = (pdmp3_loud_tables*)malloc(sizeof *t);
  if (!t) return -1;
  loud_tables_fill(fs, t);
  if (Hm) memcpy(Hm, t->Hm, sizeof t->Hm);
  if (O) memcpy(O, t->O, sizeof t->O);
  if (Phi) memcpy(Phi, t->pow[1], sizeof t->pow[1]);
  if (R) memcpy(R, t->R, sizeof t->R);
  if (pows) memcpy(pows, t->pow, sizeof t->pow);
  free(t);
  return 0;
}

/* the decoder's tables of the rate: made once, kept */
HOST_LOCAL const pdmp3_loud_tables* loud_tables(struct bulk* b, long fs) {
  for (loud_tab* t = b->loud_tabs; t; t = t->next)
    if (t->fs == fs) return &t->t;
  loud_tab* t = (loud_tab*)calloc(1, sizeof *t);
  if (!t) return NULL;
  t->fs = fs;
  loud_tables_fill(fs, &t->t);
  t->next = b->loud_tabs;
  b->loud_tabs = t;
  return &t->t;
}

HOST_LOCAL int loud_plan(long fs, long long n_samples, pdmp3_loud_params* p) {
  if (!loud_rate_ok(fs) || n_samples < 0 || n_samples > 0x7fffffffLL - 3) return -1;
  memset(p, 0, sizeof *p);
  const long long span = (long long)LOUD_B * PDMP3_LOUD_CHUNK;
  p->n_in = n_samples;
  p->q = (int32_t)((fs + 5) / 10);
  p->n_chunks = (int32_t)((n_samples + span - 1) / span);
  p->n_sub = (int32_t)(n_samples / p->q);
  p->n_mom = p->n_sub > 3 ? p->n_sub - 3 : 0;
  return 0;
}

int pdmp3_amd_loudness_plan(long fs, long long n_samples, int* B, int* chunk, unsigned* lds_bytes, int* q, long long* n_chunks, long long* I,
                            long long* J) {
  pdmp3_loud_params p;
  if (loud_plan(fs, n_samples, &p) != 0) return -1;
  if (B) *B = LOUD_B;
  if (chunk) *chunk = PDMP3_LOUD_CHUNK;
  if (lds_bytes) *lds_bytes = PDMP3_LOUD_LDS_BYTES;
  if (q) *q = p.q;
  if (n_chunks) *n_chunks = p.n_chunks;
  if (I) *I = p.n_sub;
  if (J) *J = p.n_mom;
  return 0;
}
