/* clip_beat.c -- libpdmp3.so: the planning of beat tracking of clips (include/pdmp3_bulk.h pdmp3_amd_beat_*; DESIGN.md section
 * 26): the check, the period, the two tables and the geometry of the launches of k_clip_beat_score, k_clip_beat_dp and
 * k_clip_beat_pick.  Plain arithmetic in binary64, no GPU; the call itself (pdmp3_amd_bulk_decode_clips_beats) is
 * clip_features.c's. */
#include "bulk_internal.h"

#include <math.h>

#define BEAT_THREADS 256
#define BEAT_BLOCK 64
#define BEAT_TILE 256

/* h = max(1, round-half-even(P / 2)) (csrc/beat_core.h beat_half) */
static int beat_half(int P) {
  int h = P >> 1;
  if (P & 1) h += h & 1;
  return h < 1 ? 1 : h;
}

/* the periods the tables must hold: the one of bpm, or every lag the tempo call can decide on (0, or -1) */
static int beat_periods(const pdmp3_amd_beat_spec* s, long sr, int* P, int* p_min, int* p_max) {
  if (!s) return -1;
  pdmp3_amd_tempogram_spec tg = s->tg;
  tg.out_mode = s->bpm == 0.0 ? 2 : 0;
  if (pdmp3_amd_tempogram_check(&tg, sr) != 0) return -1;
  if (!isfinite(s->bpm) || s->bpm < 0.0 || !isfinite(s->tightness) || !(s->tightness > 0.0)) return -1;
  if (s->out_mode < 0 || s->out_mode > 2 || (s->trim != 0 && s->trim != 1) || tg.mel.mel.n_frames > PDMP3_BEAT_MAX_FRAMES) return -1;
  if (s->bpm > 0.0) {
    const double p = nearbyint(60.0 * (double)sr / ((double)tg.mel.mel.hop * s->bpm));   /* (ties to even, as Python's round) */
    if (!(p >= 1.0) || !(p <= (double)PDMP3_BEAT_MAX_PERIOD)) return -1;
    *P = *p_min = *p_max = (int)p;
    return 0;
  }
  int first;
  if (pdmp3_amd_tempogram_prior(&tg, sr, NULL, 0, &first) != 0 || first < 1) return -1;
  *P = 0; *p_min = first; *p_max = tg.win_length - 1;
  return 0;
}

int pdmp3_amd_beat_check(const pdmp3_amd_beat_spec* s, long sr) {
  int P, a, b;
  return beat_periods(s, sr, &P, &a, &b);
}

/* lg: ln d for d = 0 .. 2 P at least (lg[0] is not read), so that a block of many periods takes every logarithm once */
static void beat_fill(double tightness, int P, const double* lg, double* g, double* tx) {
  const int h = beat_half(P);
  if (g) for (int k = 0; k <= P; k++) { const double a = 32.0 * (double)k / (double)P; g[k] = exp(-0.5 * (a * a)); }
  if (tx) for (int d = 0; d <= 2 * P; d++) { const double a = d >= h ? lg[d] - lg[P] : 0.0; tx[d] = d >= h ? -tightness * (a * a) : 0.0; }
}

static double* beat_logs(int p_max) {
  double* lg = (double*)malloc((size_t)(2 * p_max + 1) * sizeof *lg);
  if (lg) for (int d = 0; d <= 2 * p_max; d++) lg[d] = d ? log((double)d) : 0.0;
  return lg;
}

int pdmp3_amd_beat_tables(const pdmp3_amd_beat_spec* s, long sr, int P, double* g, double* tx) {
  if (pdmp3_amd_beat_check(s, sr) != 0 || P < 1 || P > PDMP3_BEAT_MAX_PERIOD) return -1;
  double* lg = beat_logs(P);
  if (!lg) return -1;
  beat_fill(s->tightness, P, lg, g, tx);
  free(lg);
  return 0;
}

/* doubles of the block in front of P's tables (csrc/beat_core.h beat_table_at) */
static size_t beat_table_at(int p_min, int P) {
  return (size_t)(3 * ((long long)P * (P - 1) - (long long)p_min * (p_min - 1)) / 2 + 2 * (long long)(P - p_min));
}
HOST_LOCAL size_t beat_table_bytes(const pdmp3_beat_params* p) { return beat_table_at(p->p_min, p->p_max + 1) * sizeof(double); }

HOST_LOCAL int beat_tables_fill(const pdmp3_amd_beat_spec* s, const pdmp3_beat_params* p, double* t) {
  double* lg = beat_logs(p->p_max);
  if (!lg) return -1;
  for (int P = p->p_min; P <= p->p_max; P++) {
    double* const g = t + beat_table_at(p->p_min, P);
    beat_fill(s->tightness, P, lg, g, g + P + 1);
  }
  free(lg);
  return 0;
}

/* (env_stride, channels and the frames are the call's to fill; n_frames: F for the scratch and the LDS of the blocks' sums) */
HOST_LOCAL int beat_plan(const pdmp3_amd_beat_spec* s, long sr, pdmp3_beat_params* p) {
  int P, a, b;
  if (beat_periods(s, sr, &P, &a, &b) != 0) return -1;
  memset(p, 0, sizeof *p);
  const unsigned F = (unsigned)s->tg.mel.mel.n_frames;
  p->tightness = s->tightness; p->bpm = (float)s->bpm;
  p->period = P; p->p_min = a; p->p_max = b;
  p->n_frames = (int32_t)F; p->trim = s->trim; p->out_mode = s->out_mode;
  /* csrc/beat_core.h beat_work_of, beat_score_lds, beat_dp_lds */
  p->work_stride = 8u + 2u * F + (3u * F + 1u) / 2u;
  p->score_lds_bytes = (((unsigned)b + 1u) + (BEAT_TILE + 2u * (unsigned)b) + ((F + BEAT_BLOCK - 1u) / BEAT_BLOCK + 1u)) * 8u;
  p->dp_lds_bytes = ((2u * (unsigned)b + (unsigned)beat_half(b)) + (2u * (unsigned)b + 1u) + BEAT_THREADS) * 8u;
  return p->score_lds_bytes <= PDMP3_MEL_LDS_SOFT && p->dp_lds_bytes <= PDMP3_MEL_LDS_SOFT ? 0 : -1;
}

int pdmp3_amd_beat_plan(const pdmp3_amd_beat_spec* s, long sr, int* numbers, unsigned* lds, unsigned long long* stage) {
  pdmp3_beat_params p;
  if (beat_plan(s, sr, &p) != 0) return -1;
  const int h = beat_half(p.p_max);
  int lanes = 64;
  while (lanes > 1 && lanes * h > BEAT_THREADS) lanes >>= 1;
  if (numbers) {
    numbers[0] = p.period; numbers[1] = h; numbers[2] = p.p_min; numbers[3] = p.p_max; numbers[4] = BEAT_THREADS;
    numbers[5] = (p.n_frames + h - 1) / h; numbers[6] = lanes; numbers[7] = BEAT_THREADS / lanes;
  }
  if (lds) { lds[0] = p.score_lds_bytes; lds[1] = p.dp_lds_bytes; }
  if (stage) { stage[0] = (unsigned long long)p.work_stride * 8u; stage[1] = beat_table_bytes(&p); }
  return 0;
}
