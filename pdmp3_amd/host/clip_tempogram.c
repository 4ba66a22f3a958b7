/* clip_tempogram.c -- libpdmp3.so: the planning of onset strength, tempogram and tempo of clips (include/pdmp3_bulk.h
 * pdmp3_amd_tempogram_*): the check, the window, the prior and the geometry of the launches.  Plain
 * arithmetic in binary64, no GPU; the call itself (pdmp3_amd_bulk_decode_clips_tempogram) is clip_features.c's. */
#include "bulk_internal.h"

#include <math.h>

static int tg_win_ok(int wt) { return wt >= 16 && wt <= 1024 && !(wt & 1); }
static int tg_positive(double v) { return isfinite(v) && v > 0.0; }

/* item 6's prior at lag tau (H tau and 60 sr are exact in binary64) */
static double tg_prior(const pdmp3_amd_tempogram_spec* s, long sr, int tau) {
  if (tau < 1) return -INFINITY;
  const double bpm = 60.0 * (double)sr / ((double)s->mel.mel.hop * (double)tau);
  if (!(bpm < s->max_tempo)) return -INFINITY;
  const double z = (log2(bpm) - log2(s->start_bpm)) / s->std_bpm;
  return -0.5 * (z * z);
}

/* the smallest admissible lag below Wt, or 0 */
static int tg_first(const pdmp3_amd_tempogram_spec* s, long sr) {
  for (int tau = 1; tau < s->win_length; tau++) if (tg_prior(s, sr, tau) > -INFINITY) return tau;
  return 0;
}

int pdmp3_amd_tempogram_check(const pdmp3_amd_tempogram_spec* s, long sr) {
  if (!s) return -1;
  pdmp3_amd_mel_long_spec m = s->mel;
  m.mel.out_mode = 2;
  if (pdmp3_amd_mel_long_check(&m, sr) != 0) return -1;
  if (s->lag < 1 || s->lag > 16 || s->max_size < 1 || s->max_size > 9 || !(s->max_size & 1) || !tg_win_ok(s->win_length)) return -1;
  if (!tg_positive(s->start_bpm) || !tg_positive(s->std_bpm) || !tg_positive(s->max_tempo)) return -1;
  if (s->out_mode < 0 || s->out_mode > 2 || m.mel.n_frames < 0) return -1;
  if (!tg_first(s, sr)) return -1;
  /* a clip's rows stay inside 31 bits: the log-mel's, the tempogram's */
  const long long F = m.mel.n_frames;
  if (F > 0x7fffffffLL) return -1;
  const long long Fe = s->out_mode == 0 ? F : F + s->win_length - 1;
  if ((Fe + s->lag) * m.mel.n_mels > 0x7fffffffLL || (s->out_mode != 0 && F * s->win_length > 0x7fffffffLL)) return -1;
  return 0;
}

int pdmp3_amd_tempogram_window(int win_length, float* w, size_t cap) {
  if (!tg_win_ok(win_length)) return -1;
  if (!w && !cap) return win_length;
  if (!w || cap < (size_t)win_length) return -1;
  for (int n = 0; n < win_length; n++) w[n] = (float)(0.5 - 0.5 * cos(2.0 * M_PI * (double)n / (double)win_length));
  return win_length;
}

int pdmp3_amd_tempogram_prior(const pdmp3_amd_tempogram_spec* s, long sr, double* prior, size_t cap, int* first) {
  if (pdmp3_amd_tempogram_check(s, sr) != 0 || (prior && cap < (size_t)s->win_length)) return -1;
  if (prior) for (int tau = 0; tau < s->win_length; tau++) prior[tau] = tg_prior(s, sr, tau);
  if (first) *first = tg_first(s, sr);
  return 0;
}

/* the LDS of a workgroup of `frames` waves, as csrc/tempogram_core.h lays it out (tempogram_ext, tempogram_lds) */
static void tg_lds_of(pdmp3_tempogram_params* p, int frames) {
  const unsigned reach = 4u * (unsigned)(p->ksteps + 1) + 240u + 256u * (unsigned)(p->tiles - 1);
  p->frames_wg = frames;
  p->ext = 16u + (reach > (unsigned)p->win ? reach : (unsigned)p->win);
  p->span_floats = (p->ext + 2u * (p->ext >> 4) + 3u) & ~3u;
  const unsigned floats = (unsigned)frames * (p->span_floats + 256u * (unsigned)p->tiles + 8u);
  p->lds_bytes = (floats * 4u + 15u) & ~15u;
}

/* (n_frames, n_env, n_mel_frames, env_stride and channels are the call's to fill) */
HOST_LOCAL int tempogram_plan(const pdmp3_amd_tempogram_spec* s, long sr, pdmp3_tempogram_params* p, int* front, int* back) {
  if (pdmp3_amd_tempogram_check(s, sr) != 0) return -1;
  const int wt = s->win_length;
  p->sr = (double)sr;
  p->n_mels = s->mel.mel.n_mels; p->lag = s->lag; p->half = (s->max_size - 1) / 2;
  p->hop = s->mel.mel.hop; p->win = wt;
  p->tiles = (wt + 255) / 256; p->ksteps = (wt + 18) / 4;
  p->out_mode = s->out_mode;
  *front = s->out_mode == 0 ? s->lag : s->lag + wt / 2;
  *back = s->out_mode == 0 ? 0 : wt / 2 - 1;
  for (int frames = 8; frames >= 1; frames >>= 1) {
    tg_lds_of(p, frames);
    if (p->lds_bytes <= PDMP3_MEL_LDS_MAX) return 0;
  }
  return -1;
}

int pdmp3_amd_tempogram_plan(const pdmp3_amd_tempogram_spec* s, long sr, int* front, int* back, int* tiles, int* ksteps, int* frames,
                             unsigned* lds_bytes) {
  pdmp3_tempogram_params p;
  int fr, bk;
  memset(&p, 0, sizeof p);
  if (tempogram_plan(s, sr, &p, &fr, &bk) != 0) return -1;
  if (front) *front = fr;
  if (back) *back = bk;
  if (tiles) *tiles = p.tiles;
  if (ksteps) *ksteps = p.ksteps;
  if (frames) *frames = p.frames_wg;
  if (lds_bytes) *lds_bytes = p.lds_bytes;
  return 0;
}
