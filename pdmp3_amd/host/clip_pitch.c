/* clip_pitch.c -- libpdmp3.so: the planning of the pitch of clips (include/pdmp3_bulk.h pdmp3_amd_pitch_*; DESIGN.md section
 * 20): the check, the lag range and the geometry of a workgroup of k_clip_pitch.  Plain arithmetic in binary64, no GPU, no
 * table; the call itself (pdmp3_amd_bulk_decode_clips_pitch) is clip_features.c's. */
#include "bulk_internal.h"

#include <math.h>

/* floor (up = 0) or ceiling (up = 1) of num / den from the binary64 quotient: a quotient within 1e-9 of an integer must be
 * that integer exactly -- den times it is num without a rounding error -- or nothing is known about its side (0, or -1) */
static int pitch_quotient(double num, double den, int up, double* out) {
  const double q = num / den;
  if (!(q >= 0.0) || !(q < 1e15)) return -1;
  const double n = nearbyint(q);
  if (fabs(q - n) < 1e-9) {
    if (fma(den, n, -num) != 0.0) return -1;
    *out = n;
  } else {
    *out = up ? ceil(q) : floor(q);
  }
  return 0;
}

static int pitch_frame(const pdmp3_amd_pitch_spec* s, int* N, int* W, int* H) {
  if (!s) return -1;
  const int n = s->frame_length;
  if (n < 64 || n > 2048 || (n & 1)) return -1;
  const int w = s->win_length ? s->win_length : n / 2, h = s->hop ? s->hop : n / 4;
  if (w < 4 || w > n - 2 || h < 1 || h > n) return -1;
  *N = n; *W = w; *H = h;
  return 0;
}

int pdmp3_amd_pitch_lags(const pdmp3_amd_pitch_spec* s, long sr, int* tmin, int* tmax, int* tiles) {
  int N, W, H;
  if (sr <= 0 || sr > 0x7fffffffL || pitch_frame(s, &N, &W, &H) != 0) return -1;
  if (!(s->fmin > 0.0) || !(s->fmax > s->fmin) || !(s->fmax <= (double)sr / 2.0)) return -1;
  double lo, hi;
  if (pitch_quotient((double)sr, s->fmax, 0, &lo) != 0 || pitch_quotient((double)sr, s->fmin, 1, &hi) != 0) return -1;
  const int a = lo < 1.0 ? 1 : (int)lo;                /* (fmax <= sr / 2: lo >= 2 in fact) */
  const int b = hi < (double)(N - W - 1) ? (int)hi : N - W - 1;
  if (a >= b) return -1;
  if (tmin) *tmin = a;
  if (tmax) *tmax = b;
  if (tiles) *tiles = (b + 256) / 256;
  return 0;
}

int pdmp3_amd_pitch_check(const pdmp3_amd_pitch_spec* s, long sr) {
  if (pdmp3_amd_pitch_lags(s, sr, NULL, NULL, NULL) != 0) return -1;
  if (!(s->threshold > 0.0) || !(s->threshold <= 1.0) || s->n_frames < 0 || (s->out_mode != 0 && s->out_mode != 1)) return -1;
  return 0;
}

/* the LDS of a workgroup of `frames` waves, as csrc/pitch_core.h lays it out (pitch_at, pitch_lds) */
static void pitch_lds_of(pdmp3_pitch_params* p, int frames) {
  /* the A operand's last row of the last tile, one k-step behind the last: the kernel reads a k-step ahead */
  const unsigned reach = 4u * (unsigned)(p->ksteps + 1) + 240u + 256u * (unsigned)(p->tiles - 1);
  const unsigned first = (unsigned)(frames - 1) * (unsigned)p->hop;
  p->frames_wg = frames;
  p->ext = 16u + first + (reach > (unsigned)p->n ? reach : (unsigned)p->n);
  p->span_floats = (p->ext + 2u * (p->ext >> 4) + 3u) & ~3u;
  p->q_doubles = first + (unsigned)p->n + 1u;
  const unsigned doubles = p->span_floats / 2u + p->q_doubles + 64u * (unsigned)frames + 64u;
  const unsigned floats = 2u * doubles + (unsigned)frames * (256u * (unsigned)p->tiles + 8u) + 4u * (unsigned)frames;
  p->lds_bytes = (floats * 4u + 15u) & ~15u;
}

/* (n_in, n_frames and channels are the call's to fill) */
HOST_LOCAL int pitch_plan(const pdmp3_amd_pitch_spec* s, long sr, pdmp3_pitch_params* p) {
  int N, W, H, tmin, tmax, tiles;
  if (pdmp3_amd_pitch_check(s, sr) != 0 || pitch_frame(s, &N, &W, &H) != 0 || pdmp3_amd_pitch_lags(s, sr, &tmin, &tmax, &tiles) != 0) return -1;
  p->sr = (double)sr; p->threshold = s->threshold;
  p->n = N; p->win = W; p->hop = H;
  p->tmin = tmin; p->tmax = tmax; p->tiles = tiles; p->ksteps = (W + 18) / 4;
  p->out_mode = s->out_mode;
  for (int frames = 8; frames >= 1; frames >>= 1) {
    pitch_lds_of(p, frames);
    if (p->lds_bytes <= PDMP3_MEL_LDS_MAX) return 0;
  }
  return -1;
}

int pdmp3_amd_pitch_plan(const pdmp3_amd_pitch_spec* s, long sr, int* frames, unsigned* span_floats, unsigned* lds_bytes, int* ksteps) {
  pdmp3_pitch_params p;
  memset(&p, 0, sizeof p);
  if (pitch_plan(s, sr, &p) != 0) return -1;
  if (frames) *frames = p.frames_wg;
  if (span_floats) *span_floats = p.span_floats;
  if (lds_bytes) *lds_bytes = p.lds_bytes;
  if (ksteps) *ksteps = p.ksteps;
  return 0;
}
