/* clip_audio.c -- libpdmp3.so: the planning of clips as float batches (include/pdmp3_bulk.h pdmp3_amd_audio_span,
 * pdmp3_amd_audio_table): which input samples a clip reads, and the filter table of a pair of sampling
 * frequencies.  Plain arithmetic, no GPU; the call itself (pdmp3_amd_bulk_decode_clips_audio) is clip_features.c's. */
#include "bulk_internal.h"

#include <math.h>

HOST_LOCAL int audio_plan_init(audio_plan* p, long in, long out, int width, double rolloff) {
  if (width == 0) width = 6;
  if (rolloff == 0.0) rolloff = 0.99;
  if (in <= 0 || out <= 0 || in > 0x7fffffffL || out > 0x7fffffffL || width < 1 || width > 64 || !(rolloff > 0.0 && rolloff <= 1.0)) return -1;
  long a = in, b = out;
  while (b) { const long t = a % b; a = b; b = t; }
  memset(p, 0, sizeof *p);
  p->in = in; p->out = out; p->width = width; p->rolloff = rolloff;
  p->M = in / a; p->L = out / a;
  if (p->M == p->L) { p->taps = 1; return 0; }      /* (the stream's own rate: input sample j, no table) */
  /* |n L - j M| < B = Z max(L, M) / rolloff, j M = q L + r with 0 <= r < L, n = q + d:  (r - B) / L < d < (r + B) / L;
   * over all r:  floor(-B / L) + 1 <= d <= ceil((L - 1 + B) / L) - 1 */
  const double B = (double)width * (double)(p->L > p->M ? p->L : p->M) / rolloff;
  const double d0 = floor(-B / (double)p->L) + 1.0, d1 = ceil(((double)(p->L - 1) + B) / (double)p->L) - 1.0;
  if (d1 - d0 + 1.0 > (double)AUDIO_TABLE_MAX) return -1;
  p->d0 = (int)d0;
  p->taps = (int)(d1 - d0) + 1;
  return 0;
}

int pdmp3_amd_audio_span(long in, long out, int width, double rolloff, long long start, long long n, long long* first_in, long long* n_in) {
  audio_plan p;
  if (audio_plan_init(&p, in, out, width, rolloff) != 0 || start < 0 || n < 0 || !first_in || !n_in) return -1;
  if (start > (long long)(0x7fffffffffffffffLL / 2) / p.M - n) return -1;         /* (j M stays inside 63 bits) */
  if (p.M == p.L || n == 0) { *first_in = start; *n_in = n; return 0; }
  const long long q0 = start * p.M / p.L, q1 = (start + n - 1) * p.M / p.L;
  *first_in = q0 + p.d0;
  *n_in = q1 - q0 + p.taps;
  return 0;
}

/* row r, tap k: n L - j M = (d0 + k) L - r, an integer; everything from there on in binary64, rounded once */
HOST_LOCAL void audio_plan_table(const audio_plan* p, float* table) {
  const double pi = 3.14159265358979323846;
  const double s = (double)(p->L > p->M ? p->L : p->M);
  const double scale = p->rolloff * (double)(p->L < p->M ? p->L : p->M) / (double)p->M;
  for (long r = 0; r < p->L; r++)
    for (int k = 0; k < p->taps; k++) {
      const double u = p->rolloff * (double)((long long)(p->d0 + k) * p->L - r) / s;
      double h = 0.0;
      if (fabs(u) < (double)p->width) {
        const double c = cos(pi * u / (2.0 * (double)p->width));
        h = scale * (u == 0.0 ? 1.0 : sin(pi * u) / (pi * u)) * c * c;
      }
      table[(size_t)r * (size_t)p->taps + (size_t)k] = (float)h;
    }
}

long long pdmp3_amd_audio_table(long in, long out, int width, double rolloff, float* table, size_t cap, long* rows, int* taps, int* first_tap) {
  audio_plan p;
  if (audio_plan_init(&p, in, out, width, rolloff) != 0 || p.M == p.L) return -1;
  const long long count = (long long)p.L * p.taps;
  if (count > AUDIO_TABLE_MAX) return -1;
  if (rows) *rows = p.L;
  if (taps) *taps = p.taps;
  if (first_tap) *first_tap = p.d0;
  if (table && cap) {
    if ((size_t)count <= cap) audio_plan_table(&p, table);
    else {
      float* t = (float*)malloc((size_t)count * sizeof *t);
      if (!t) return -1;
      audio_plan_table(&p, t);
      memcpy(table, t, cap * sizeof *t);
      free(t);
    }
  }
  return count;
}
