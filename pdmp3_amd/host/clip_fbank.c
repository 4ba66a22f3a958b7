/* clip_fbank.c -- libpdmp3.so: the planning of Kaldi-style filterbank features of clips (include/pdmp3_bulk.h
 * pdmp3_amd_fbank_*): the DFT table with DC removal, pre-emphasis, the window and the zero padding
 * folded in, the mel filterbank, the frames wholly inside a stream and the kernel's tile.  Plain arithmetic in binary64, no
 * GPU; the call itself (pdmp3_amd_bulk_decode_clips_fbank) is clip_features.c's. */
#include "bulk_internal.h"

#include <float.h>
#include <math.h>

static int flag_ok(int v) { return v == 0 || v == 1; }

int pdmp3_amd_fbank_dft_length(int win_length, int round_to_power_of_two) {
  if (win_length < 2 || win_length > 1024 || !flag_ok(round_to_power_of_two)) return -1;
  if (!round_to_power_of_two) return (win_length & 1) ? -1 : win_length;
  int n = 2;
  while (n < win_length) n <<= 1;
  return n;
}

HOST_LOCAL int fbank_frame_ok(const pdmp3_amd_fbank_spec* s) {
  if (!s || pdmp3_amd_fbank_dft_length(s->win_length, s->round_to_power_of_two) < 0) return 0;
  if (!flag_ok(s->remove_dc_offset) || !(s->preemphasis >= 0.0) || !(s->preemphasis <= 1.0)) return 0;
  if (s->window < 0 || s->window > 4 || !isfinite(s->blackman_coeff)) return 0;
  /* (|w| <= 1 + 2 |b| and |T| <= 6 max |w| scale: inside binary32, and scale itself not below its normal numbers) */
  if (!isfinite(s->scale) || !(s->scale > 0.0) || !((float)s->scale >= FLT_MIN)) return 0;
  if (!(6.0 * (1.0 + 2.0 * fabs(s->blackman_coeff)) * s->scale <= (double)FLT_MAX)) return 0;
  return 1;
}

static double fbank_mel(double f) { return 1127.0 * log(1.0 + f / 700.0); }
static double fbank_hi(long sr, double high_freq) { return high_freq <= 0.0 ? (double)sr / 2.0 + high_freq : high_freq; }
static int fbank_band_ok(long sr, int n_mels, double lo, double high_freq) {
  if (sr <= 0 || sr > 0x7fffffffL || n_mels < 1 || n_mels > 256 || !isfinite(high_freq)) return 0;
  const double hi = fbank_hi(sr, high_freq);
  return lo >= 0.0 && hi <= (double)sr / 2.0 && lo < hi;
}

int pdmp3_amd_fbank_check(const pdmp3_amd_fbank_spec* s, long sr) {
  if (!fbank_frame_ok(s)) return -1;
  if (s->hop < 1 || s->hop > s->win_length || !fbank_band_ok(sr, s->n_mels, s->low_freq, s->high_freq)) return -1;
  if (s->out_mode < 0 || s->out_mode > 1 || !flag_ok(s->use_energy) || !flag_ok(s->htk_compat) || !flag_ok(s->subtract_mean)) return -1;
  if (!(s->energy_floor >= 0.0) || !isfinite(s->energy_floor) || s->n_frames < 0) return -1;
  /* what is not offered */
  if (s->dither != 0.0 || (s->vtln_warp != 0.0 && s->vtln_warp != 1.0) || s->no_power || s->no_raw_energy || s->no_snip_edges) return -1;
  return 0;
}

static double fbank_window(int window, double b, int n, int Nw) {
  const double pi = 3.14159265358979323846;
  const double t = 2.0 * pi * (double)n / (double)(Nw - 1);
  switch (window) {
    case 0: return pow(0.5 - 0.5 * cos(t), 0.85);
    case 1: return 0.5 - 0.5 * cos(t);
    case 2: return 0.54 - 0.46 * cos(t);
    case 3: return 1.0;
    default: return b - 0.5 * cos(t) + (0.5 - b) * cos(2.0 * t);
  }
}

HOST_LOCAL void fbank_table_fill(const pdmp3_amd_fbank_spec* s, float* t) {
  const double pi = 3.14159265358979323846;
  const int Nw = s->win_length, N = pdmp3_amd_fbank_dft_length(Nw, s->round_to_power_of_two);
  const int K = N / 2, Kp = (K + 15) & ~15, rows = (Nw + 3) & ~3, ld = 2 * Kp;
  const double rho = s->preemphasis;
  double w[1024], c[1025];
  memset(t, 0, (size_t)rows * (size_t)ld * sizeof *t);
  for (int n = 0; n < Nw; n++) w[n] = fbank_window(s->window, s->blackman_coeff, n, Nw);
  for (int part = 0; part < 2; part++)
    for (int k = 0; k < K; k++) {
      for (int n = 0; n < Nw; n++) {
        const double a = 2.0 * pi * (double)(((long)k * n) % N) / (double)N;
        c[n] = part ? -w[n] * sin(a) : w[n] * cos(a);
      }
      c[Nw] = 0.0;
      /* the frame's own steps, transposed: X = sum c[n] p[n] = sum d[n] a[n] = sum (d[n] - mean d) s[n] */
      double sum = 0.0;
      for (int n = 0; n < Nw; n++) {
        c[n] = c[n] - rho * c[n + 1] - (n == 0 ? rho * c[0] : 0.0);      /* (c[n + 1] is still the window's) */
        sum += c[n];
      }
      const double mean = s->remove_dc_offset ? sum / (double)Nw : 0.0;
      for (int n = 0; n < Nw; n++) t[(size_t)n * (size_t)ld + (size_t)(part ? Kp + k : k)] = (float)(s->scale * (c[n] - mean));
    }
}

long long pdmp3_amd_fbank_table(const pdmp3_amd_fbank_spec* s, float* table, size_t cap, int* rows, int* cols) {
  if (!fbank_frame_ok(s)) return -1;
  const int N = pdmp3_amd_fbank_dft_length(s->win_length, s->round_to_power_of_two);
  const int Kp = (N / 2 + 15) & ~15, r = (s->win_length + 3) & ~3;
  const long long count = (long long)r * (2 * Kp);
  if (rows) *rows = r;
  if (cols) *cols = 2 * Kp;
  if (table && cap) {
    if ((size_t)count <= cap) fbank_table_fill(s, table);
    else {
      float* t = (float*)malloc((size_t)count * sizeof *t);
      if (!t) return -1;
      fbank_table_fill(s, t);
      memcpy(table, t, cap * sizeof *t);
      free(t);
    }
  }
  return count;
}

HOST_LOCAL void fbank_fb_fill(long sr, int n_dft, int n_mels, double lo, double high_freq, float* w) {
  const int K = n_dft / 2;
  const double m_lo = fbank_mel(lo), m_hi = fbank_mel(fbank_hi(sr, high_freq));
  const double d = (m_hi - m_lo) / (double)(n_mels + 1);
  for (int m = 0; m < n_mels; m++) {
    const double l = m_lo + (double)m * d, c = l + d, r = l + 2.0 * d;
    for (int k = 0; k < K; k++) {
      const double mk = fbank_mel((double)k * (double)sr / (double)n_dft);
      const double up = (mk - l) / (c - l), down = (r - mk) / (r - c);
      const double v = up < down ? up : down;
      w[(size_t)m * (size_t)K + (size_t)k] = (float)(v > 0.0 ? v : 0.0);
    }
  }
}

long long pdmp3_amd_fbank_filterbank(long sr, int n_dft, int n_mels, double low_freq, double high_freq, float* w, size_t cap) {
  if (n_dft < 2 || n_dft > 1024 || (n_dft & 1) || !fbank_band_ok(sr, n_mels, low_freq, high_freq)) return -1;
  const long long count = (long long)n_mels * (n_dft / 2);
  if (w && cap) {
    if ((size_t)count <= cap) fbank_fb_fill(sr, n_dft, n_mels, low_freq, high_freq, w);
    else {
      float* t = (float*)malloc((size_t)count * sizeof *t);
      if (!t) return -1;
      fbank_fb_fill(sr, n_dft, n_mels, low_freq, high_freq, t);
      memcpy(w, t, cap * sizeof *t);
      free(t);
    }
  }
  return count;
}

long long pdmp3_amd_fbank_valid(long long J, long long start, int win_length, int hop, long long n_frames) {
  if (J < 0 || start < 0 || win_length < 1 || hop < 1 || n_frames < 0) return -1;
  if (J - start < win_length) return 0;               /* (J >= 0 and start >= 0: no overflow) */
  const long long v = (J - start - win_length) / hop + 1;
  return v < n_frames ? v : n_frames;
}

/* mel_lds's arithmetic (clip_mel.c) with this kernel's rows and bins: the tile's span in chunks of hop + row_pad floats, or
 * the mel tile [mels16][tile + 1] where that is larger; then the powers [tile][bins16 + 2] */
static void fbank_lds(int win, int n_dft, int hop, int n_mels, int tile, int row_pad, unsigned* span_floats, unsigned* bytes) {
  const unsigned rows = ((unsigned)win + 3u) & ~3u, Kp = ((unsigned)n_dft / 2u + 15u) & ~15u, Mp = ((unsigned)n_mels + 15u) & ~15u;
  const unsigned span = (unsigned)(tile - 1) * (unsigned)hop + rows;
  unsigned a = ((span + (unsigned)hop - 1u) / (unsigned)hop) * (unsigned)(hop + row_pad);
  const unsigned mt = Mp * (unsigned)(tile + 1);
  if (mt > a) a = mt;
  a = (a + 3u) & ~3u;
  *span_floats = a;
  *bytes = (a + (unsigned)tile * (Kp + 2u)) * 4u;
}
HOST_LOCAL int fbank_plan(int win, int n_dft, int hop, int n_mels, pdmp3_fbank_params* p) {
  if (win < 2 || win > 1024 || n_dft < win || n_dft > 1024 || (n_dft & 1) || hop < 1 || hop > win || n_mels < 1 || n_mels > 256) return -1;
  if (n_dft != win && (n_dft & (n_dft - 1))) return -1;
  p->win = win; p->rows = (win + 3) & ~3; p->n_dft = n_dft;
  p->hop = hop; p->row_pad = (int)((2u - (unsigned)hop) & 31u);
  p->bins16 = (n_dft / 2 + 15) & ~15; p->n_mels = n_mels; p->mels16 = (n_mels + 15) & ~15;
  p->tile = 32;
  fbank_lds(win, n_dft, hop, n_mels, 32, p->row_pad, &p->span_floats, &p->lds_bytes);
  if (p->lds_bytes > PDMP3_MEL_LDS_SOFT) {
    p->tile = 16;
    fbank_lds(win, n_dft, hop, n_mels, 16, p->row_pad, &p->span_floats, &p->lds_bytes);
  }
  return p->lds_bytes <= PDMP3_MEL_LDS_MAX ? 0 : -1;
}
int pdmp3_amd_fbank_tile(int win_length, int n_dft, int hop, int n_mels, int* tile, int* row_pad, unsigned* lds_bytes) {
  pdmp3_fbank_params p;
  memset(&p, 0, sizeof p);
  if (fbank_plan(win_length, n_dft, hop, n_mels, &p) != 0) return -1;
  if (tile) *tile = p.tile;
  if (row_pad) *row_pad = p.row_pad;
  if (lds_bytes) *lds_bytes = p.lds_bytes;
  return 0;
}
