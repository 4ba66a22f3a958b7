/* clip_spectral.c -- libpdmp3.so: the planning of the spectral descriptors of clips at n_fft 2048 and 4096 (include/pdmp3_bulk.h
 * pdmp3_amd_spectral_*): the check and the kernel's tile.  The frame's rules and the four transform
 * tables are clip_stft_long.c's; no table of its own, no GPU.  The call itself (pdmp3_amd_bulk_decode_clips_spectral) is
 * clip_features.c's. */
#include "bulk_internal.h"

#include <float.h>
#include <math.h>

static int spec_fft_ok(int n_fft) { return n_fft == 2048 || n_fft == 4096; }

HOST_LOCAL void spectral_stft_spec(const pdmp3_amd_spectral_spec* s, pdmp3_amd_stft_spec* t) {
  memset(t, 0, sizeof *t);
  t->rate = s->rate; t->channels = s->channels; t->width = s->width; t->rolloff = s->rolloff;
  t->n_fft = s->n_fft; t->hop = s->hop;
  t->win_length = s->win_length; t->window = s->window;
  t->n_frames = s->n_frames;
  t->out_mode = 1;
}

int pdmp3_amd_spectral_check(const pdmp3_amd_spectral_spec* s, long sr) {
  if (!s || !spec_fft_ok(s->n_fft)) return -1;
  if (!(s->roll_percent > 0.0) || !(s->roll_percent < 1.0)) return -1;
  if (!(s->amin > 0.0) || !((float)s->amin >= FLT_MIN) || !(s->amin <= (double)FLT_MAX)) return -1;
  if (!(s->zcr_threshold >= 0.0) || !(s->zcr_threshold <= (double)FLT_MAX)) return -1;
  /* hop, win_length, the window's values, n_frames and sr: section 14's */
  pdmp3_amd_stft_spec t;
  spectral_stft_spec(s, &t);
  return pdmp3_amd_stft_long_check(&t, sr);
}

/* The LDS of a workgroup with `tile` frames: the tile's span, (tile - 1) hop + N floats rounded up to 4, which stays for all
 * four tiles of k1; then Z, tile x N2 x 32 floats; then the plane, tile x (N / 2 + 1) floats; then the results, 8 x tile floats
 * (csrc/spectral_core.h has the same numbers for the kernel).  One tile a length: 8 frames at N 2048 -- one a wave; 16 would
 * need 64 KB of Z and 64 KB of plane beside a span of up to 128 KB -- and 4 at N 4096, where 8 would need 128 KB for Z and the
 * plane alone.  By this arithmetic the largest plans are 131 360 B (N 2048, hop 2048) and 131 216 B (N 4096, hop 4096): every
 * hop fits PDMP3_MEL_LDS_MAX.  These two (N2, tile) pairs are the kernel's launch paths. */
static int spec_plan(int n_fft, int hop, pdmp3_spectral_params* p) {
  if (!spec_fft_ok(n_fft) || hop < 1 || hop > n_fft) return -1;
  const unsigned n2 = (unsigned)n_fft / 64u, tile = n_fft == 2048 ? 8u : 4u;
  p->n_fft = n_fft; p->n2 = (int32_t)n2; p->hop = hop; p->tile = (int32_t)tile;
  p->span_floats = ((tile - 1u) * (unsigned)hop + (unsigned)n_fft + 3u) & ~3u;
  p->lds_bytes = ((p->span_floats + tile * n2 * 32u + tile * ((unsigned)n_fft / 2u + 1u) + 8u * tile + 3u) & ~3u) * 4u;
  return p->lds_bytes <= PDMP3_MEL_LDS_MAX ? 0 : -1;
}
int pdmp3_amd_spectral_plan(int n_fft, int hop, int* tile, int* row_pad, unsigned* lds_bytes) {
  pdmp3_spectral_params p;
  memset(&p, 0, sizeof p);
  if (spec_plan(n_fft, hop, &p) != 0) return -1;
  if (tile) *tile = p.tile;
  if (row_pad) *row_pad = 0;                         /* (the span lies plain in LDS, as section 14's) */
  if (lds_bytes) *lds_bytes = p.lds_bytes;
  return 0;
}

HOST_LOCAL int spectral_plan(const pdmp3_amd_spectral_spec* s, long sr, pdmp3_spectral_params* p) {
  if (pdmp3_amd_spectral_check(s, sr) != 0 || spec_plan(s->n_fft, s->hop, p) != 0) return -1;
  p->bin_hz = (double)sr / (double)s->n_fft;
  p->roll_percent = s->roll_percent;
  p->amin = (float)s->amin;
  p->zcr_threshold = (float)s->zcr_threshold;
  return 0;
}
