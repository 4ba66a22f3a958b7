/* clip_hpss.c -- libpdmp3.so: the planning of the harmonic-percussive separation of clips (include/pdmp3_bulk.h
 * pdmp3_amd_hpss_*): the check, the frames a clip is widened by and the kernel's tile.  The frame's
 * rules and the transform's tables are clip_stft_long.c's; no table of its own, no GPU.  The call itself
 * (pdmp3_amd_bulk_decode_clips_hpss) is clip_features.c's. */
#include "bulk_internal.h"

#include <float.h>
#include <math.h>

static int hpss_kernel_ok(int l) { return l >= 3 && l <= PDMP3_HPSS_MAX_KERNEL && (l & 1); }
static int hpss_margin_ok(double m) { return m >= 1.0 && m <= DBL_MAX; }      /* (false for a NaN) */
/* 1, 2, or 0 for +inf; -1: refused */
static int hpss_power(double p) { return p == 1.0 ? 1 : p == 2.0 ? 2 : (p > 0.0 && isinf(p)) ? 0 : -1; }

HOST_LOCAL void hpss_stft_spec(const pdmp3_amd_hpss_spec* s, pdmp3_amd_stft_spec* t) {
  memset(t, 0, sizeof *t);
  t->rate = s->rate; t->channels = s->channels; t->width = s->width; t->rolloff = s->rolloff;
  t->n_fft = s->n_fft; t->hop = s->hop;
  t->win_length = s->win_length; t->window = s->window;
  t->n_frames = s->n_frames;
  t->out_mode = s->out_mode == 2 ? 0 : 1;            /* what the stage holds: complex values for mode 2, else magnitudes */
}

int pdmp3_amd_hpss_check(const pdmp3_amd_hpss_spec* s, long sr) {
  if (!s || !hpss_kernel_ok(s->kernel_harm) || !hpss_kernel_ok(s->kernel_perc)) return -1;
  if (!hpss_margin_ok(s->margin_harm) || !hpss_margin_ok(s->margin_perc) || hpss_power(s->power) < 0) return -1;
  if (s->out_mode < 0 || s->out_mode > 3 || s->n_frames < 0) return -1;
  /* n_fft, hop, win_length, the window's values and sr: section 14's */
  pdmp3_amd_stft_spec t;
  hpss_stft_spec(s, &t);
  if (pdmp3_amd_stft_long_check(&t, sr) != 0) return -1;
  /* a channel's row of the output and of the stage inside 31 bits */
  const long long e = s->out_mode == 2 ? 2 : 1, K = s->n_fft / 2 + 1;
  if (s->n_frames > 0x7fffffffLL / (2 * e * K) || s->n_frames + s->kernel_harm - 1 > 0x7fffffffLL / (e * K)) return -1;
  return 0;
}

/* One tile and one LDS layout for every pair of kernel sizes: 64 bins x 64 frames -- a wave's lanes are the 64 frames of one
 * bin -- with room for 15 bins and 15 frames around it, rows 94 floats apart (csrc/hpss_core.h has the same numbers for the
 * kernel): 94 x 94 x 4 = 35 344 B, four workgroups a CU.  The sizes decide what of it is loaded, and the frames in front and
 * behind. */
static int hpss_tile(int kernel_harm, int kernel_perc, pdmp3_hpss_params* p) {
  if (!hpss_kernel_ok(kernel_harm) || !hpss_kernel_ok(kernel_perc)) return -1;
  p->kernel_harm = kernel_harm; p->kernel_perc = kernel_perc;
  p->tile_bins = 64; p->tile_frames = 64;
  p->pitch = p->tile_frames + PDMP3_HPSS_MAX_KERNEL - 1;
  p->lds_bytes = (uint32_t)(p->tile_bins + PDMP3_HPSS_MAX_KERNEL - 1) * (uint32_t)p->pitch * 4u;
  return p->lds_bytes <= PDMP3_MEL_LDS_MAX ? 0 : -1;
}
int pdmp3_amd_hpss_plan(int kernel_harm, int kernel_perc, int* front, int* back, int* tile_bins, int* tile_frames, int* pitch,
                        unsigned* lds_bytes) {
  pdmp3_hpss_params p;
  memset(&p, 0, sizeof p);
  if (hpss_tile(kernel_harm, kernel_perc, &p) != 0) return -1;
  if (front) *front = kernel_harm / 2;
  if (back) *back = kernel_harm / 2;
  if (tile_bins) *tile_bins = p.tile_bins;
  if (tile_frames) *tile_frames = p.tile_frames;
  if (pitch) *pitch = p.pitch;
  if (lds_bytes) *lds_bytes = p.lds_bytes;
  return 0;
}

HOST_LOCAL int hpss_plan(const pdmp3_amd_hpss_spec* s, long sr, pdmp3_hpss_params* p, int* front, int* back) {
  if (pdmp3_amd_hpss_check(s, sr) != 0 || hpss_tile(s->kernel_harm, s->kernel_perc, p) != 0) return -1;
  p->n_fft = s->n_fft; p->bins = s->n_fft / 2 + 1;
  p->out_mode = s->out_mode; p->power = hpss_power(s->power);
  p->margin_harm = s->margin_harm; p->margin_perc = s->margin_perc;
  *front = *back = s->kernel_harm / 2;
  return 0;
}
