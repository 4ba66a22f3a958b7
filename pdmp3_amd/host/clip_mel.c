/* clip_mel.c -- libpdmp3.so: the planning of log-mel features of clips (include/pdmp3_bulk.h pdmp3_amd_mel_*; DESIGN.md
 * section 10): the DFT table with the window folded in, the mel filterbank, the samples a clip's frames read and the
 * kernel's tile.  Plain arithmetic in binary64, no GPU; the call itself (pdmp3_amd_bulk_decode_clips_mel) is clip_features.c's. */
#include "bulk_internal.h"

#include <float.h>
#include <math.h>

static int mel_fft_ok(int n_fft) { return n_fft >= 16 && n_fft <= 1024 && !(n_fft & 1); }

int pdmp3_amd_mel_check(const pdmp3_amd_mel_spec* s, long sr) {
  if (!s || sr <= 0 || sr > 0x7fffffffL) return -1;
  if (!mel_fft_ok(s->n_fft) || s->hop < 1 || s->hop > s->n_fft || s->n_mels < 1 || s->n_mels > 256) return -1;
  const double top = s->f_max == 0.0 ? (double)sr / 2.0 : s->f_max;
  if (!(s->f_min >= 0.0) || !(top <= (double)sr / 2.0) || !(s->f_min < top)) return -1;
  if (s->scale < 0 || s->scale > 1 || s->norm < 0 || s->norm > 1 || s->out_mode < 0 || s->out_mode > 3 || s->n_frames < 0) return -1;
  if (!(s->floor > 0.0) || !((float)s->floor >= FLT_MIN) || !(s->floor <= (double)FLT_MAX)) return -1;
  return 0;
}

int pdmp3_amd_mel_span(int n_fft, int hop, long long start, long long n_frames, long long* first, long long* count) {
  if (!mel_fft_ok(n_fft) || hop < 1 || hop > n_fft || start < 0 || n_frames < 0 || !first || !count) return -1;
  if (n_frames > (1LL << 40) || start > (1LL << 62)) return -1;           /* (the products below stay inside 63 bits) */
  *first = start - n_fft / 2;
  *count = n_frames ? (n_frames - 1) * hop + n_fft : 0;
  return 0;
}

HOST_LOCAL void mel_dft_fill(int n_fft, float* t) {
  const double pi = 3.14159265358979323846;
  const int N = n_fft, K = N / 2 + 1, Kp = (K + 15) & ~15, rows = (N + 3) & ~3;
  memset(t, 0, (size_t)rows * (size_t)(2 * Kp) * sizeof *t);
  for (int n = 0; n < N; n++) {
    const double w = 0.5 - 0.5 * cos(2.0 * pi * (double)n / (double)N);
    float* row = t + (size_t)n * (size_t)(2 * Kp);
    for (int k = 0; k < K; k++) {
      const double a = 2.0 * pi * (double)(((long)k * n) % N) / (double)N;
      row[k] = (float)(w * cos(a));
      row[Kp + k] = (float)(-w * sin(a));
    }
  }
}

long long pdmp3_amd_mel_dft_table(int n_fft, float* table, size_t cap, int* rows, int* cols) {
  if (!mel_fft_ok(n_fft)) return -1;
  const int K = n_fft / 2 + 1, Kp = (K + 15) & ~15, r = (n_fft + 3) & ~3;
  const long long count = (long long)r * (2 * Kp);
  if (rows) *rows = r;
  if (cols) *cols = 2 * Kp;
  if (table && cap) {
    if ((size_t)count <= cap) mel_dft_fill(n_fft, table);
    else {
      float* t = (float*)malloc((size_t)count * sizeof *t);
      if (!t) return -1;
      mel_dft_fill(n_fft, t);
      memcpy(table, t, cap * sizeof *t);
      free(t);
    }
  }
  return count;
}

static double hz_to_mel(double f, int htk) {
  if (htk) return 2595.0 * log10(1.0 + f / 700.0);
  return f < 1000.0 ? 3.0 * f / 200.0 : 15.0 + 27.0 * log(f / 1000.0) / log(6.4);
}
static double mel_to_hz(double m, int htk) {
  if (htk) return 700.0 * (pow(10.0, m / 2595.0) - 1.0);
  return m < 15.0 ? 200.0 * m / 3.0 : 1000.0 * exp(log(6.4) * (m - 15.0) / 27.0);
}

HOST_LOCAL int mel_fb_fill(long sr, int n_fft, int n_mels, double f_min, double f_max, int scale, int norm, float* w) {
  const int K = n_fft / 2 + 1;
  if (f_max == 0.0) f_max = (double)sr / 2.0;
  double* f = (double*)malloc((size_t)(n_mels + 2) * sizeof *f);
  if (!f) return -1;
  const double m0 = hz_to_mel(f_min, scale), m1 = hz_to_mel(f_max, scale);
  for (int i = 0; i < n_mels + 2; i++) f[i] = mel_to_hz(m0 + (m1 - m0) * (double)i / (double)(n_mels + 1), scale);
  f[0] = f_min; f[n_mels + 1] = f_max;              /* (the ends are what was asked for, not a round trip through mel) */
  for (int m = 0; m < n_mels; m++) {
    const double enorm = norm ? 2.0 / (f[m + 2] - f[m]) : 1.0;
    for (int k = 0; k < K; k++) {
      const double fk = (double)k * (double)sr / (double)n_fft;
      const double up = (fk - f[m]) / (f[m + 1] - f[m]), down = (f[m + 2] - fk) / (f[m + 2] - f[m + 1]);
      const double v = up < down ? up : down;
      w[(size_t)m * (size_t)K + (size_t)k] = (float)(v > 0.0 ? v * enorm : 0.0);
    }
  }
  free(f);
  return 0;
}

long long pdmp3_amd_mel_filterbank(long sr, int n_fft, int n_mels, double f_min, double f_max, int scale, int norm, float* w, size_t cap) {
  pdmp3_amd_mel_spec s;
  memset(&s, 0, sizeof s);
  s.n_fft = n_fft; s.hop = 1; s.n_mels = n_mels; s.f_min = f_min; s.f_max = f_max; s.scale = scale; s.norm = norm; s.floor = 1.0;
  if (pdmp3_amd_mel_check(&s, sr) != 0) return -1;
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

/* the LDS of a workgroup with `tile` frames: the tile's span in chunks of hop + row_pad floats, or the mel tile
 * [mels16][tile + 1] where that is larger; then the powers [tile][bins16 + 2] */
static void mel_lds(int n_fft, int hop, int n_mels, int tile, int row_pad, unsigned* span_floats, unsigned* bytes) {
  const unsigned rows = ((unsigned)n_fft + 3u) & ~3u, Kp = ((unsigned)n_fft / 2u + 1u + 15u) & ~15u, Mp = ((unsigned)n_mels + 15u) & ~15u;
  const unsigned span = (unsigned)(tile - 1) * (unsigned)hop + rows;
  unsigned a = ((span + (unsigned)hop - 1u) / (unsigned)hop) * (unsigned)(hop + row_pad);
  const unsigned mt = Mp * (unsigned)(tile + 1);
  if (mt > a) a = mt;
  a = (a + 3u) & ~3u;
  *span_floats = a;
  *bytes = (a + (unsigned)tile * (Kp + 2u)) * 4u;
}
HOST_LOCAL int mel_plan(int n_fft, int hop, int n_mels, pdmp3_mel_params* p) {
  if (!mel_fft_ok(n_fft) || hop < 1 || hop > n_fft || n_mels < 1 || n_mels > 256) return -1;
  p->n_fft = n_fft; p->rows = (n_fft + 3) & ~3;
  p->hop = hop; p->row_pad = (int)((2u - (unsigned)hop) & 31u);
  p->bins16 = (n_fft / 2 + 1 + 15) & ~15; p->n_mels = n_mels; p->mels16 = (n_mels + 15) & ~15;
  p->tile = 32;
  mel_lds(n_fft, hop, n_mels, 32, p->row_pad, &p->span_floats, &p->lds_bytes);
  if (p->lds_bytes > PDMP3_MEL_LDS_SOFT) {
    p->tile = 16;
    mel_lds(n_fft, hop, n_mels, 16, p->row_pad, &p->span_floats, &p->lds_bytes);
  }
  return p->lds_bytes <= PDMP3_MEL_LDS_MAX ? 0 : -1;
}
int pdmp3_amd_mel_tile(int n_fft, int hop, int n_mels, int* tile, int* row_pad, unsigned* lds_bytes) {
  pdmp3_mel_params p;
  memset(&p, 0, sizeof p);
  if (mel_plan(n_fft, hop, n_mels, &p) != 0) return -1;
  if (tile) *tile = p.tile;
  if (row_pad) *row_pad = p.row_pad;
  if (lds_bytes) *lds_bytes = p.lds_bytes;
  return 0;
}
