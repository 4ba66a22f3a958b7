/* clip_r128.c -- libpdmp3.so: the planning of the true peak, the short-term loudness and the loudness range of clips
 * (include/pdmp3_bulk.h pdmp3_amd_r128_*): the check, the interpolator's taps and the launch's geometry on
 * top of clip_loudness.c's.  Plain binary64 arithmetic, no GPU; the call itself (pdmp3_amd_bulk_decode_clips_r128) is
 * clip_features.c's. */
#include "bulk_internal.h"

#include <math.h>

#define R128_H 49                      /* taps of the interpolator */
#define R128_WINDOW 30                 /* sub-blocks of a short-term window */
#define R128_EVERY 10                  /* sub-blocks between two windows of the range */

/* h[j] = sinc4(j - 24) * Hann(j / 48); what is smaller than 1e-6 is exactly 0 (libebur128's interpolator at factor 4) */
static void r128_h(double* h) {
  const double pi = 3.14159265358979323846;
  for (int j = 0; j < R128_H; j++) {
    const int m = j - (R128_H - 1) / 2;
    const double x = (double)m * pi / 4.0;
    const double c = (m == 0 ? 1.0 : sin(x) / x) * 0.5 * (1.0 - cos(2.0 * pi * (double)j / (double)(R128_H - 1)));
    h[j] = fabs(c) < 1e-6 ? 0.0 : c;
  }
}

int pdmp3_amd_r128_taps(double* h, float* phases) {
  double t[R128_H];
  r128_h(t);
  if (h) memcpy(h, t, sizeof t);
  if (phases)
    for (int p = 1; p < 4; p++)
      for (int d = 0; d < PDMP3_R128_TAPS; d++) phases[(p - 1) * PDMP3_R128_TAPS + d] = (float)t[4 * d + p];
  return 0;
}

HOST_LOCAL int r128_plan(long fs, long long n_samples, pdmp3_r128_params* p) {
  memset(p, 0, sizeof *p);
  if (loud_plan(fs, n_samples, &p->loud) != 0) return -1;
  p->n_st = p->loud.n_sub > R128_WINDOW - 1 ? p->loud.n_sub - (R128_WINDOW - 1) : 0;
  const long long n_rng = ((long long)p->n_st + R128_EVERY - 1) / R128_EVERY;
  if (n_rng > PDMP3_R128_MAX_RANGE) return -1;
  p->n_rng = (int32_t)n_rng;
  return 0;
}

int pdmp3_amd_r128_check(const pdmp3_amd_r128_spec* s, long fs, int channels) {
  pdmp3_r128_params p;
  if (!s || pdmp3_amd_loudness_check(&s->loudness, fs, channels) != 0) return -1;
  if (s->limit_true_peak != 0 && s->limit_true_peak != 1) return -1;
  return r128_plan(fs, s->loudness.n_samples, &p);
}

int pdmp3_amd_r128_plan(long fs, long long n_samples, int* B, int* chunk, unsigned* lds_bytes, int* q, long long* n_chunks, long long* I,
                        long long* J, long long* Js, long long* Jr, long long* Jsmax) {
  pdmp3_r128_params p;
  if (r128_plan(fs, n_samples, &p) != 0) return -1;
  if (pdmp3_amd_loudness_plan(fs, n_samples, B, chunk, lds_bytes, q, n_chunks, I, J) != 0) return -1;
  if (Js) *Js = p.n_st;
  if (Jr) *Jr = p.n_rng;
  if (Jsmax) *Jsmax = p.n_st;
  return 0;
}
