/* clip_stft_long.c -- libpdmp3.so: the planning of the short-time Fourier transform of clips at n_fft 2048 and 4096
 * (include/pdmp3_bulk.h pdmp3_amd_stft_long_*): the check, the four tables of the two-stage transform
 * N = 64 N2, the kernel's tile and the decoder's two blocks of tables.  Plain arithmetic in binary64, every angle reduced as
 * an integer modulo its period, rounded once; no GPU.  The call itself (pdmp3_amd_bulk_decode_clips_stft_long) is clip_features.c's. */
#include "bulk_internal.h"

#include <float.h>
#include <math.h>

static const double kPi = 3.14159265358979323846;

static int stftl_fft_ok(int n_fft) { return n_fft == 2048 || n_fft == 4096; }
static int stftl_frame_ok(const pdmp3_amd_stft_spec* s) {
  if (!s || !stftl_fft_ok(s->n_fft) || s->win_length < 0 || s->win_length > s->n_fft) return 0;
  if (s->normalized != 0 && s->normalized != 1) return 0;
  if (s->window) {
    const int nw = s->win_length ? s->win_length : s->n_fft;
    for (int i = 0; i < nw; i++) if (!isfinite(s->window[i])) return 0;
  }
  return 1;
}

int pdmp3_amd_stft_long_check(const pdmp3_amd_stft_spec* s, long sr) {
  if (!s || sr <= 0 || sr > 0x7fffffffL) return -1;
  if (!stftl_frame_ok(s) || s->hop < 1 || s->hop > s->n_fft || s->n_frames < 0 || s->out_mode < 0 || s->out_mode > 4) return -1;
  if (s->out_mode >= 3 && (!(s->floor > 0.0) || !((float)s->floor >= FLT_MIN) || !(s->floor <= (double)FLT_MAX))) return -1;
  return 0;
}

/* the places of the four tables in their block (csrc/stft_long_core.h has the same numbers for the kernel) */
static size_t stftl_at_d64(int N) { return (size_t)N; }
static size_t stftl_at_h2(int N) { return (size_t)N + 64 * 128; }
static size_t stftl_at_tw(int N) { return stftl_at_h2(N) + 2 * (size_t)(N / 64) * (size_t)(N / 64); }
static size_t stftl_floats(int N) { return stftl_at_tw(N) + (size_t)(N / 64) * 128; }

/* wt[n] = fl32(s w[n]), 0 outside the window's support (the caller has checked the frame) */
static void stftl_fill_wt(const pdmp3_amd_stft_spec* s, float* wt) {
  const int N = s->n_fft, Nw = s->win_length ? s->win_length : N, left = (N - Nw) / 2;
  const double scale = s->normalized ? 1.0 / sqrt((double)N) : 1.0;
  memset(wt, 0, (size_t)N * sizeof *wt);
  for (int i = 0; i < Nw; i++)
    wt[left + i] = (float)(scale * (s->window ? (double)s->window[i] : 0.5 - 0.5 * cos(2.0 * kPi * (double)i / (double)Nw)));
}
/* the three tables that depend on N alone */
static void stftl_fill_const(int N, float* t) {
  const int N2 = N / 64, K2 = N2 / 2;
  float* d64 = t + stftl_at_d64(N);
  for (int n1 = 0; n1 < 64; n1++)
    for (int k1 = 0; k1 < 64; k1++) {
      const double a = 2.0 * kPi * (double)((n1 * k1) % 64) / 64.0;
      d64[n1 * 128 + k1] = (float)cos(a);
      d64[n1 * 128 + 64 + k1] = (float)(-sin(a));
    }
  float* h2 = t + stftl_at_h2(N);
  for (int n2 = 0; n2 < N2; n2++)
    for (int k2 = 0; k2 < K2; k2++) {
      const double a = 2.0 * kPi * (double)((n2 * k2) % N2) / (double)N2;
      h2[(2 * n2) * N2 + k2] = (float)cos(a);
      h2[(2 * n2 + 1) * N2 + k2] = (float)sin(a);
      h2[(2 * n2) * N2 + K2 + k2] = (float)(-sin(a));
      h2[(2 * n2 + 1) * N2 + K2 + k2] = (float)cos(a);
    }
  float* tw = t + stftl_at_tw(N);
  for (int n2 = 0; n2 < N2; n2++)
    for (int k1 = 0; k1 < 64; k1++) {
      const double a = 2.0 * kPi * (double)(n2 * k1) / (double)N;            /* (n2 k1 < N: reduced as it is) */
      tw[n2 * 128 + k1] = (float)cos(a);
      tw[n2 * 128 + 64 + k1] = (float)(-sin(a));
    }
}

long long pdmp3_amd_stft_long_tables(const pdmp3_amd_stft_spec* s, float* tables, size_t cap, int* shapes) {
  if (!stftl_frame_ok(s)) return -1;
  const int N = s->n_fft, N2 = N / 64;
  const size_t count = stftl_floats(N);
  if (shapes) {
    shapes[0] = 1; shapes[1] = N;
    shapes[2] = 64; shapes[3] = 128;
    shapes[4] = 2 * N2; shapes[5] = N2;
    shapes[6] = N2; shapes[7] = 128;
  }
  if (tables && cap) {
    float* t = (float*)malloc(count * sizeof *t);
    if (!t) return -1;
    stftl_fill_wt(s, t);
    stftl_fill_const(N, t);
    memcpy(tables, t, (cap < count ? cap : count) * sizeof *t);
    free(t);
  }
  return (long long)count;
}

/* The LDS of a workgroup with `tile` frames: the first region holds the tile's span, (tile - 1) hop + N floats, and after
 * stage 1 the staging tile, (out_mode 0 ? 2 : 1) x 16 x N2 / 2 rows of tile + 1 floats -- the larger of the two, rounded up
 * to 4 floats; then Z, tile x N2 x 32 floats. */
static void stftl_lds(int n_fft, int hop, int out_mode, int tile, unsigned* span_floats, unsigned* bytes) {
  const unsigned n2 = (unsigned)n_fft / 64u;
  const unsigned span = (unsigned)(tile - 1) * (unsigned)hop + (unsigned)n_fft;
  const unsigned stage = (out_mode == 0 ? 2u : 1u) * 16u * (n2 / 2u) * (unsigned)(tile + 1);
  const unsigned a = ((span > stage ? span : stage) + 3u) & ~3u;
  *span_floats = a;
  *bytes = (a + (unsigned)tile * n2 * 32u) * 4u;
}
/* 16 frames where that fits the LDS of a workgroup, else 8, else 4.  By the arithmetic above: N 2048 takes 16 frames up to
 * hop 1500 and 8 beyond (96 KB at hop 2048); N 4096 never fits 16 (Z alone is 128 KB), takes 8 up to hop 2923 and 4 beyond
 * (96 KB at hop 4096).  These four (N2, tile) pairs are the kernel's launch paths. */
HOST_LOCAL int stft_long_plan(int n_fft, int hop, int out_mode, pdmp3_stft_long_params* p) {
  if (!stftl_fft_ok(n_fft) || hop < 1 || hop > n_fft || out_mode < 0 || out_mode > 4) return -1;
  p->n_fft = n_fft; p->n2 = n_fft / 64;
  p->hop = hop; p->bins = n_fft / 2 + 1;
  p->out_mode = out_mode;
  for (int tile = 16; tile >= 4; tile >>= 1) {
    p->tile = tile;
    stftl_lds(n_fft, hop, out_mode, tile, &p->span_floats, &p->lds_bytes);
    if (p->lds_bytes <= PDMP3_MEL_LDS_MAX) return 0;
  }
  return -1;
}
int pdmp3_amd_stft_long_plan(int n_fft, int hop, int out_mode, int* tile, int* row_pad, unsigned* lds_bytes) {
  pdmp3_stft_long_params p;
  memset(&p, 0, sizeof p);
  if (stft_long_plan(n_fft, hop, out_mode, &p) != 0) return -1;
  if (tile) *tile = p.tile;
  if (row_pad) *row_pad = 0;                         /* (the span lies plain in LDS: section 14 has the banks) */
  if (lds_bytes) *lds_bytes = p.lds_bytes;
  return 0;
}

/* The decoder's block of tables of the spec's n_fft: the three constant tables are made once and kept for the decoder's
 * life, wt -- N products -- is filled on every call. */
HOST_LOCAL const float* stft_long_tables(struct bulk* b, const pdmp3_amd_stft_spec* s) {
  float** t = &b->stft_long_tabs[s->n_fft == 4096];
  if (!*t) {
    *t = (float*)malloc(stftl_floats(s->n_fft) * sizeof **t);
    if (!*t) return NULL;
    stftl_fill_const(s->n_fft, *t);
  }
  stftl_fill_wt(s, *t);
  return *t;
}
