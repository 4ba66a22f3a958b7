/* clip_pyin.c -- libpdmp3.so: the planning of pYIN pitch tracking of clips (include/pdmp3_bulk.h pdmp3_amd_pyin_*; DESIGN.md
 * section 25): the check, the numbers derived from the spec, every table the kernels read, and the geometry of the launches of
 * k_clip_pyin_obs and k_clip_pyin_path.  Plain arithmetic in binary64 (the beta weights in long double, rounded once), no GPU;
 * the call itself (pdmp3_amd_bulk_decode_clips_pyin) is clip_features.c's. */
#include "bulk_internal.h"

#include <float.h>
#include <math.h>

/* what the spec comes to at sr */
typedef struct {
  int tmin, tmax, H;
  int n_s, n_b, msf, Wd, hb, max_troughs;
} pyin_numbers;

static int pyin_prob(double p) { return p > 0.0 && p < 1.0; }

/* x, which decides an integer at the boundaries k + at (at: 0 for floor and ceiling, 0.5 for rounding): closer than 1e-9 to one
 * without being it, nothing is known about its side (-1; section 20's rule 2 on the binary64 value of the stated formula) */
static int pyin_clear(double x, double at) {
  if (!isfinite(x) || !(x >= 0.0) || !(x < 1e9)) return -1;
  const double k = nearbyint(x - at) + at;
  return x != k && fabs(x - k) < 1e-9 ? -1 : 0;
}

static int pyin_derive(const pdmp3_amd_pyin_spec* s, long sr, pyin_numbers* n) {
  if (!s) return -1;
  pdmp3_amd_pitch_spec ps = s->pitch;
  ps.threshold = 0.1; ps.out_mode = 1;                 /* (neither is read: the curve has no threshold) */
  int tiles;
  if (pdmp3_amd_pitch_check(&ps, sr) != 0 || pdmp3_amd_pitch_lags(&ps, sr, &n->tmin, &n->tmax, &tiles) != 0) return -1;
  n->H = ps.hop ? ps.hop : ps.frame_length / 4;
  if (s->n_thresholds < 1 || s->n_thresholds > 256 || !(s->boltzmann > 0.0) || !isfinite(s->boltzmann)) return -1;
  if (!pyin_prob(s->switch_prob) || !pyin_prob(s->no_trough_prob) || (s->out_mode != 0 && s->out_mode != 1)) return -1;
  if (s->use_bin_frequency != 0 && s->use_bin_frequency != 1) return -1;
  if (s->threshold_weights) {
    for (int i = 0; i < s->n_thresholds; i++) if (!isfinite(s->threshold_weights[i]) || !(s->threshold_weights[i] >= 0.0)) return -1;
  } else if (!(s->beta_a >= 1.0) || !(s->beta_a <= 64.0) || !(s->beta_b >= 1.0) || !(s->beta_b <= 64.0) || s->beta_a != floor(s->beta_a) ||
             s->beta_b != floor(s->beta_b)) {
    return -1;
  }
  if (!(s->resolution > 0.0) || !(s->max_transition_rate >= 0.0)) return -1;
  const double qs = 1.0 / s->resolution;
  if (pyin_clear(qs, 0.0) != 0 || !(ceil(qs) >= 1.0) || !(ceil(qs) <= 20.0)) return -1;
  n->n_s = (int)ceil(qs);
  const double qb = (double)(12 * n->n_s) * log2(s->pitch.fmax / s->pitch.fmin);
  if (pyin_clear(qb, 0.0) != 0 || !(floor(qb) + 1.0 >= 2.0) || !(floor(qb) + 1.0 <= 2048.0)) return -1;
  n->n_b = (int)floor(qb) + 1;
  const double qm = s->max_transition_rate * 12.0 * (double)n->H / (double)sr;
  if (pyin_clear(qm, 0.5) != 0 || !(nearbyint(qm) <= 4096.0)) return -1;
  n->msf = (int)nearbyint(qm);                         /* (ties to even, as Python's round) */
  n->Wd = n->msf * n->n_s + 1;
  if (n->Wd > n->n_b) return -1;
  n->hb = n->Wd / 2;
  n->max_troughs = (n->tmax - 1 - n->tmin) / 2 + 1;
  /* rows inside 31 bits: the curve's, the observation's, the back-pointers' */
  const long long F = s->pitch.n_frames;
  if (F * (n->tmax + 1) > 0x7fffffffLL || F * (n->n_b + 1) > 0x7fffffffLL || F * 2 * n->n_b > 0x7fffffffLL) return -1;
  return 0;
}

int pdmp3_amd_pyin_check(const pdmp3_amd_pyin_spec* s, long sr) {
  pyin_numbers n;
  return pyin_derive(s, sr, &n);
}

/* I(x; a, b) for integers a, b: the binomial sum over j = a .. n of C(n, j) x^j (1 - x)^(n - j), n = a + b - 1, and its
 * complement, the sum over j < a.  Every term is positive, so long double carries either to far below binary64's rounding; the
 * weights are differences of the one that is small, so that they keep their relative accuracy where the other nears 1. */
static void pyin_beta_cdf(long double x, int a, int b, long double* head, long double* tail) {
  const int n = a + b - 1;
  long double c = 1.0L;                                /* C(n, j) */
  *head = *tail = 0.0L;
  for (int j = 0; j <= n; j++) {
    const long double term = c * powl(x, (long double)j) * powl(1.0L - x, (long double)(n - j));
    if (j >= a) *head += term; else *tail += term;
    c = c * (long double)(n - j) / (long double)(j + 1);
  }
}

/* the transition window at offset d = j - i of a row (item 7): librosa's transition_local places scipy's triangle of Wd samples
 * with pad_center and a roll by n_b / 2 + i + 1.  An odd Wd has its peak of 1 on the diagonal.  An even Wd has two equal peaks
 * (Wd - 1) / Wd, at offsets 0 and +1 where n_b is even, at -1 and 0 where n_b is odd; the offset at the other end holds 0. */
static double pyin_tri(int Wd, int n_b, int d) {
  if (Wd & 1) return 1.0 - (double)abs(d) / ((double)(Wd + 1) / 2.0);
  const int m = d + Wd / 2 - ((n_b & 1) ? 0 : 1);
  if (m < 0 || m >= Wd) return 0.0;
  return (double)(2 * (m < Wd - 1 - m ? m : Wd - 1 - m) + 1) / (double)Wd;
}

static void pyin_params_of(const pdmp3_amd_pyin_spec* s, const pyin_numbers* n, pdmp3_pyin_params* p) {
  memset(p, 0, sizeof *p);
  p->no_trough = s->no_trough_prob;
  p->l_stay = log(1.0 - s->switch_prob); p->l_sw = log(s->switch_prob);
  p->l0 = log(DBL_MIN); p->lp0_u = -log((double)n->n_b);
  p->fill = s->fill; p->use_bin = s->use_bin_frequency;
  p->tmin = n->tmin; p->tmax = n->tmax;
  p->n_thr = s->n_thresholds; p->n_bins = n->n_b; p->hb = n->hb; p->max_troughs = n->max_troughs;
  p->out_mode = s->out_mode;
}

/* doubles of the block without the bins' frequencies behind it (csrc/pyin_core.h pyin_table_layout) */
static size_t pyin_table_doubles(const pdmp3_pyin_params* p) {
  return 3u * (size_t)p->n_thr + 1u + 2u * (size_t)p->max_troughs + 1u + 2u * (size_t)p->n_bins + 2u * (size_t)p->hb + 1u;
}

HOST_LOCAL size_t pyin_table_bytes(const pdmp3_pyin_params* p) { return pyin_table_doubles(p) * sizeof(double) + (size_t)p->n_bins * sizeof(float); }

/* the block: theta | w | wsum | G | cN | T | ltri | lZ in binary64, then the bins' frequencies in binary32 */
HOST_LOCAL int pyin_tables_fill(const pdmp3_amd_pyin_spec* s, long sr, const pdmp3_pyin_params* p, double* t) {
  pyin_numbers n;
  if (pyin_derive(s, sr, &n) != 0) return -1;
  const int nt = p->n_thr, nb = p->n_bins, mt = p->max_troughs, hb = p->hb;
  double* theta = t, *w = theta + nt, *wsum = w + nt, *G = wsum + nt + 1, *cN = G + mt, *T = cN + mt + 1, *ltri = T + nb, *lZ = ltri + 2 * hb + 1;
  float* f0 = (float*)(lZ + nb);
  for (int i = 1; i <= nt; i++) theta[i - 1] = (double)i / (double)nt;
  if (s->threshold_weights) {
    for (int i = 0; i < nt; i++) w[i] = s->threshold_weights[i];
  } else {
    long double h0 = 0.0L, q0 = 1.0L;
    for (int i = 1; i <= nt; i++) {
      long double h1, q1;
      pyin_beta_cdf((long double)i / (long double)nt, (int)s->beta_a, (int)s->beta_b, &h1, &q1);
      const long double d = h1 < q1 ? h1 - h0 : q0 - q1;
      w[i - 1] = d > 0.0L ? (double)d : 0.0;
      h0 = h1; q0 = q1;
    }
  }
  wsum[0] = 0.0;
  for (int i = 1; i <= nt; i++) wsum[i] = wsum[i - 1] + w[i - 1];
  const double lam = s->boltzmann;
  for (int k = 0; k < mt; k++) G[k] = exp(-lam * (double)k);
  cN[0] = 0.0;
  for (int k = 1; k <= mt; k++) cN[k] = (1.0 - exp(-lam)) / (1.0 - exp(-lam * (double)k));
  for (int q = 1; q <= nb; q++) T[q - 1] = (double)sr / (s->pitch.fmin * exp2(((double)q - 0.5) / (double)(12 * n.n_s)));
  for (int q = 1; q < nb; q++) if (!(T[q] < T[q - 1])) return -1;          /* (the search in T_q relies on it) */
  for (int d = -hb; d <= hb; d++) { const double v = pyin_tri(n.Wd, nb, d); ltri[d + hb] = v > 0.0 ? log(v) : -INFINITY; }
  for (int i = 0; i < nb; i++) {
    double z = 0.0;
    for (int j = i - hb < 0 ? 0 : i - hb; j <= i + hb && j < nb; j++) z += pyin_tri(n.Wd, nb, j - i);
    lZ[i] = log(z);
  }
  for (int b = 0; b < nb; b++) f0[b] = (float)(s->pitch.fmin * exp2((double)b / (double)(12 * n.n_s)));
  return 0;
}

/* (n_frames and channels are the call's to fill) */
HOST_LOCAL int pyin_plan(const pdmp3_amd_pyin_spec* s, long sr, pdmp3_pyin_params* p) {
  pyin_numbers n;
  if (pyin_derive(s, sr, &n) != 0) return -1;
  pyin_params_of(s, &n, p);
  /* csrc/pyin_core.h pyin_obs_lds, pyin_path_lds, pyin_path_threads */
  const unsigned stride = (((unsigned)n.tmax + 2u) & ~1u) + (((unsigned)n.n_b + 2u) & ~1u) + 2u * (((unsigned)p->n_thr + 1u) & ~1u) + 64u;
  for (int frames = 8; frames >= 1; frames >>= 1) {
    p->frames_wg = frames;
    p->obs_lds_bytes = (unsigned)frames * stride * 4u;
    if (p->obs_lds_bytes <= PDMP3_MEL_LDS_SOFT) break;
  }
  const unsigned t = ((unsigned)n.n_b + 63u) & ~63u;
  p->path_threads = (int)(t > 1024u ? 1024u : t);
  p->path_lds_bytes = (8u * (unsigned)n.n_b + 96u + 2u * (unsigned)n.hb + 1u) * 8u;
  return p->obs_lds_bytes <= PDMP3_MEL_LDS_SOFT && p->path_lds_bytes <= PDMP3_MEL_LDS_MAX ? 0 : -1;
}

int pdmp3_amd_pyin_tables(const pdmp3_amd_pyin_spec* s, long sr, double* tables, size_t cap, int* counts) {
  pdmp3_pyin_params p;
  if (pyin_plan(s, sr, &p) != 0) return -1;
  const size_t block = (pyin_table_bytes(&p) + 7u) / 8u, need = block + 4u;   /* (the four scalars behind the kernels' block) */
  if (counts) { counts[0] = p.n_thr; counts[1] = p.max_troughs; counts[2] = p.n_bins; counts[3] = p.hb; }
  if (!tables && !cap) return (int)need;
  if (!tables || cap < need) return -1;
  memset(tables, 0, need * 8u);
  if (pyin_tables_fill(s, sr, &p, tables) != 0) return -1;
  tables[block] = p.l_stay; tables[block + 1] = p.l_sw; tables[block + 2] = p.l0; tables[block + 3] = p.lp0_u;
  return (int)need;
}

int pdmp3_amd_pyin_plan(const pdmp3_amd_pyin_spec* s, long sr, int* numbers, unsigned* lds, unsigned long long* stage) {
  pdmp3_pyin_params p;
  pyin_numbers n;
  if (pyin_plan(s, sr, &p) != 0 || pyin_derive(s, sr, &n) != 0) return -1;
  if (numbers) {
    numbers[0] = 2 * n.n_b; numbers[1] = n.n_b; numbers[2] = n.n_s; numbers[3] = n.msf; numbers[4] = n.Wd; numbers[5] = n.hb;
    numbers[6] = p.frames_wg; numbers[7] = p.path_threads;
  }
  if (lds) { lds[0] = p.obs_lds_bytes; lds[1] = p.path_lds_bytes; }
  if (stage) {
    const unsigned long long F = (unsigned long long)s->pitch.n_frames;
    stage[0] = F * (unsigned)(n.tmax + 1) * 4u;
    stage[1] = s->out_mode == 0 ? F * (unsigned)(n.n_b + 1) * 4u : 0u;
    stage[2] = s->out_mode == 0 ? F * 2u * (unsigned)n.n_b * 2u : 0u;
  }
  return 0;
}
