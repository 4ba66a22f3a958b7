/* clip_features.c -- libpdmp3.so: clips by sample position as float batches, and the feature calls on top of them
 * (include/pdmp3_bulk.h: pdmp3_amd_bulk_decode_clips_audio, _mel, _mel_long, _fbank, _mfcc, _stft, _stft_long, _cqt, _chroma,
 * _loudness, _r128, _pitch, _tempogram, _spectral, _hpss, _mfcc_long, _pyin, _beats; DESIGN.md sections 9-26).  The audio call turns clips into rows of resampled samples; a feature call runs its rows through
 * the audio call into audio stage 2 and its own kernel behind them.  That course -- arguments, rows, signal, copies out -- is
 * written once here (clip_course); an entry point has its check and plan, its tables, its parameters and its launch.  The
 * checks, plans and tables' contents are the clip_*.c files'.  See host_internal.h for the map of the library. */
#include "bulk_internal.h"

#include <math.h>
#include <stddef.h>

/* host destinations: rows that lie one behind the other in the caller's memory as they do in the stage leave in one copy.
 * host[i]: descriptor i's clip, if that one's rows went to the stage, else -1; dst: the descriptors' device addresses, `stride`
 * bytes apart; per: floats of a channel's row.  One loop serves both descriptor types (the audio call's and the feature calls'):
 * it is given the first descriptor's dst and the descriptors' size, which holds as long as dst is a uint64_t in both. */
_Static_assert(_Generic(((pdmp3_audio_desc*)0)->dst, uint64_t: 1, default: 0) && _Generic(((pdmp3_mel_desc*)0)->dst, uint64_t: 1, default: 0),
               "copy_rows_out reads dst as a uint64_t");
static int copy_rows_out(const pdmp3_amd_audio_clip* clips, const int* host, int nd, int C, size_t per, const uint64_t* dst, size_t stride) {
  for (int i = 0; i < nd; i++) {
    if (host[i] < 0) continue;
    const pdmp3_amd_audio_clip* c = &clips[host[i]];
    const float* from = (const float*)(uintptr_t)*(const uint64_t*)((const char*)dst + (size_t)i * stride);
    if (C == 2 && c->chan_stride != per) {
      if (pdmp3_hip_copy_from_device(c->dst, from, per * sizeof(float)) != PDMP3_HIP_OK ||
          pdmp3_hip_copy_from_device(c->dst + c->chan_stride, from + per, per * sizeof(float)) != PDMP3_HIP_OK) return -1;
      continue;
    }
    size_t floats = (size_t)C * per;
    int j = i + 1;
    for (; j < nd && host[j] >= 0; j++) {
      const pdmp3_amd_audio_clip* n = &clips[host[j]];
      if (n->dst != c->dst + floats || (C == 2 && n->chan_stride != per)) break;
      floats += (size_t)C * per;
    }
    if (pdmp3_hip_copy_from_device(c->dst, from, floats * sizeof(float)) != PDMP3_HIP_OK) return -1;
    i = j - 1;
  }
  return 0;
}

/* ---- clips as float batches ---- */
/* the decoder's table of the pair (made once, kept) */
static const audio_tab* audio_table(struct bulk* b, const audio_plan* p) {
  for (audio_tab* t = b->audio_tabs; t; t = t->next)
    if (t->p.in == p->in && t->p.out == p->out && t->p.width == p->width && t->p.rolloff == p->rolloff) return t;
  audio_tab* t = (audio_tab*)calloc(1, sizeof *t);
  if (t) t->h = (float*)malloc((size_t)p->L * (size_t)p->taps * sizeof(float));
  if (!t || !t->h) { free(t); return NULL; }
  t->p = *p;
  audio_plan_table(p, t->h);
  t->next = b->audio_tabs;
  b->audio_tabs = t;
  return t;
}
/* what a workgroup of k_clip_audio keeps in LDS (include/pdmp3_hip.h pdmp3_audio_desc): the input span of its
 * PDMP3_AUDIO_TILE output samples if that fits, the table too if it fits behind it */
static void audio_lds(pdmp3_audio_desc* d, int channels) {
  const unsigned long long span = ((unsigned long long)(d->L - 1) + (unsigned long long)(PDMP3_AUDIO_TILE - 1) * d->M) / d->L + (unsigned)d->taps;
  const unsigned long long cap = (span + 3) & ~3ULL, xb = cap * (unsigned)channels * 4;
  d->flags = 0; d->span_cap = 0;
  if (xb > PDMP3_AUDIO_LDS_BYTES) return;
  d->flags = PDMP3_AUDIO_LDS_X;
  d->span_cap = (uint32_t)cap;
  if (xb + ((((unsigned long long)d->L * (unsigned)d->taps) + 3) & ~3ULL) * 4 <= PDMP3_AUDIO_LDS_BYTES) d->flags |= PDMP3_AUDIO_LDS_TABLE;
}
/* ... for the host tests: the plan a clip of this pair gets in a call with `channels` channels */
int pdmp3_amd_audio_lds_plan(long in, long out, int width, double rolloff, int channels, unsigned* flags, unsigned* span_cap) {
  audio_plan p;
  pdmp3_audio_desc d;
  if (audio_plan_init(&p, in, out, width, rolloff) != 0 || (channels != 1 && channels != 2)) return -1;
  memset(&d, 0, sizeof d);
  d.M = (uint32_t)p.M; d.L = (uint32_t)p.L; d.taps = p.taps;
  if (p.M != p.L) audio_lds(&d, channels);
  if (flags) *flags = d.flags;
  if (span_cap) *span_cap = d.span_cap;
  return 0;
}

int pdmp3_amd_bulk_decode_clips_audio(struct bulk* b, const pdmp3_amd_audio_clip* clips, int n_clips, const pdmp3_amd_audio_spec* spec,
                                      long long* valid) {
  if (!b || !b->hs || !b->bits_mode || !spec || n_clips < 0 || (n_clips && (!clips || !valid)) || spec->n_samples < 0) return -1;
  const long long T = spec->n_samples;
  int C = spec->channels, rc = 0;
  if (C < 0 || C > 2) return -1;
  for (int k = 0; k < n_clips; k++) {
    const pdmp3_amd_audio_clip* c = &clips[k];
    if (!c->index || (!c->mp3 && c->n) || c->n != c->index->n || c->start < 0 || (T && !c->dst)) return -1;
    if ((c->index->iso & PDMP3_ISO_LSF) != (b->id->iso & PDMP3_ISO_LSF)) return -1;
    if (c->index->frames < 0 || c->index->mixed) continue;
    const int cs = c->index->stereo ? 2 : 1;
    if (!spec->channels) {
      if (C && C != cs) return -1;                   /* (no channel count asked for, and the clips' differ) */
      C = cs;
    }
  }
  if (!C) C = 1;                                     /* (no clip to decode) */
  for (int k = 0; k < n_clips; k++) if (C == 2 && T && clips[k].chan_stride < (size_t)T) return -1;
  pdmp3_amd_clip* pc = (pdmp3_amd_clip*)calloc((size_t)n_clips + 1, sizeof *pc);
  long long* pb = (long long*)calloc((size_t)n_clips + 1, sizeof *pb);
  pdmp3_audio_desc* ds = (pdmp3_audio_desc*)calloc((size_t)n_clips + 1, sizeof *ds);
  int* host = (int*)calloc((size_t)n_clips + 1, sizeof *host);       /* per descriptor: its clip, if that one's rows go to host memory, else -1 */
  const audio_tab** tabs = (const audio_tab**)calloc((size_t)n_clips + 1, sizeof *tabs);   /* the launch's distinct tables */
  uint32_t* ft = NULL;
  float* coef = NULL;
  int nd = 0, ntab = 0;
  size_t n_ft = 0, n_coef = 0, in_bytes = 0, out_floats = 0;
  if (!pc || !pb || !ds || !host || !tabs) { rc = -1; goto out; }
  /* pass 1: every clip's plan -- its frames [a, e), its table, where its PCM and (host destinations) its rows are staged */
  for (int k = 0; k < n_clips; k++) {
    const pdmp3_amd_audio_clip* c = &clips[k];
    const pdmp3_amd_index* ix = c->index;
    if (ix->frames < 0) { valid[k] = PDMP3_BULK_REPLAY; rc = PDMP3_BULK_REPLAY; continue; }
    if (ix->mixed) { valid[k] = PDMP3_BULK_MIXED_FORMAT; if (rc != PDMP3_BULK_REPLAY) rc = PDMP3_BULK_MIXED_FORMAT; continue; }
    audio_plan p;
    const long in = ix->frames ? ix->rate : (spec->rate ? spec->rate : 44100);      /* (a stream without frames: only zeros come of it) */
    if (audio_plan_init(&p, in, spec->rate ? spec->rate : in, spec->width, spec->rolloff) != 0) { rc = -1; goto out; }
    if (p.M != p.L && (long long)p.L * p.taps > AUDIO_TABLE_MAX) { rc = -1; goto out; }
    const long long N = ix->frames * (ix->frames ? ix->spf : 0);
    const long long J = (long long)(((__int128)N * p.L + p.M - 1) / p.M);
    long long first, cnt;
    if (pdmp3_amd_audio_span(p.in, p.out, p.width, p.rolloff, c->start, T, &first, &cnt) != 0) { rc = -1; goto out; }
    valid[k] = J - c->start < 0 ? 0 : J - c->start < T ? J - c->start : T;
    if (!T) continue;
    long long lo = first < 0 ? 0 : first, hi = first + cnt > N ? N : first + cnt;
    if (!valid[k] || hi <= lo) lo = hi = 0;          /* (wholly behind the stream's end: zeros) */
    const long long a = hi > lo ? lo / ix->spf : 0, e = hi > lo ? (hi - 1) / ix->spf + 1 : 0;
    pdmp3_audio_desc* d = &ds[nd];
    d->start = c->start; d->n_in = N; d->n_out = J;
    d->frame0 = a; d->n_frames = (uint32_t)(e - a); d->frame_tab = (uint32_t)n_ft;
    d->M = (uint32_t)p.M; d->L = (uint32_t)p.L; d->spf = (uint32_t)(ix->frames ? ix->spf : 1152);
    d->taps = p.taps; d->d0 = p.d0;
    d->chan_stride = c->chan_stride;
    if (e - a > 0x7fffffff || n_ft + (size_t)(e - a) > 0xffffffffu) { rc = -1; goto out; }
    if (p.M != p.L) {
      const audio_tab* t = audio_table(b, &p);
      if (!t) { rc = -1; goto out; }
      int i = 0;
      while (i < ntab && tabs[i] != t) i++;
      if (i == ntab) tabs[ntab++] = t;
      d->table = (uint32_t)i;                        /* (its place among the launch's tables; the offset follows below) */
      audio_lds(d, C);
    }
    /* the clip's int16 PCM: one 16-byte aligned place of the stage (every frame's PCM is a multiple of 1152 bytes) */
    pc[nd].mp3 = c->mp3; pc[nd].n = c->n; pc[nd].index = ix;
    pc[nd].first_frame = a; pc[nd].n_frames = e - a;
    pc[nd].dst_cap = (size_t)(ix->off[e] - ix->off[a]);
    d->src = in_bytes;                               /* (offsets until the stages are there) */
    in_bytes += pc[nd].dst_cap;
    n_ft += (size_t)(e - a);
    const size_t row_bytes = ((size_t)(C - 1) * c->chan_stride + (size_t)T) * sizeof(float);
    if (pdmp3_hip_host_is_pinned(c->dst, row_bytes) == 2) { host[nd] = -1; d->dst = (uint64_t)(uintptr_t)c->dst; }
    else { host[nd] = k; d->dst = out_floats; d->chan_stride = (uint64_t)T; out_floats += (size_t)C * (size_t)T; }
    nd++;
  }
  if (!nd) goto out;
  /* the frame table and the launch's tables, each table at a multiple of four floats */
  ft = (uint32_t*)malloc((n_ft + 1) * sizeof *ft);
  size_t* tab_at = (size_t*)calloc((size_t)ntab + 1, sizeof *tab_at);
  if (tab_at) for (int i = 0; i < ntab; i++) { tab_at[i] = n_coef; n_coef += ((size_t)tabs[i]->p.L * (size_t)tabs[i]->p.taps + 3) & ~(size_t)3; }
  if (tab_at) coef = (float*)calloc(n_coef + 4, sizeof *coef);
  if (!ft || !tab_at || !coef || n_coef > 0xffffffffu) { free(tab_at); rc = -1; goto out; }
  for (int i = 0; i < ntab; i++) memcpy(coef + tab_at[i], tabs[i]->h, (size_t)tabs[i]->p.L * (size_t)tabs[i]->p.taps * sizeof(float));
  if (pdmp3_amd_bulk_wait(b) != 0) { free(tab_at); rc = -1; goto out; }
  uint8_t* in_stage = (uint8_t*)pdmp3_hip_stream_audio_stage(b->hs, 0, in_bytes);
  float* out_stage = out_floats ? (float*)pdmp3_hip_stream_audio_stage(b->hs, 1, out_floats * sizeof(float)) : NULL;
  if (!in_stage || (out_floats && !out_stage)) { free(tab_at); rc = -1; goto out; }
  for (int i = 0; i < nd; i++) {
    pdmp3_audio_desc* d = &ds[i];
    const pdmp3_amd_index* ix = pc[i].index;
    pc[i].dst = in_stage + d->src;
    d->src = (uint64_t)(uintptr_t)pc[i].dst;
    if (host[i] >= 0) d->dst = (uint64_t)(uintptr_t)(out_stage + d->dst);
    if (d->M != d->L) d->table = (uint32_t)tab_at[d->table];
    for (uint32_t f = 0; f < d->n_frames; f++) {
      const long long at = ix->off[d->frame0 + f] - ix->off[d->frame0];
      const int mono = ((ix->fr[d->frame0 + f] >> PDMP3_FR_MODE_SHIFT) & 3) == 3;
      ft[d->frame_tab + f] = (uint32_t)(at / 1152) << 1 | (uint32_t)mono;
    }
  }
  free(tab_at);
  /* the clips' frames through the clip path as it is, into the stage; then the one kernel behind the last window */
  {
    const int r = pdmp3_amd_bulk_decode_clips(b, pc, nd, pb);
    if (r != 0) { rc = -1; goto out; }
  }
  if (pdmp3_hip_clip_audio(b->hs, CLIP_SLOT, ds, nd, ft, n_ft, coef, n_coef, T, C) != PDMP3_HIP_OK) {
    fprintf(stderr, "pdmp3: engine failure: %s\n", pdmp3_hip_last_error());
    rc = -1; goto out;
  }
  if (copy_rows_out(clips, host, nd, C, (size_t)T, &ds[0].dst, sizeof *ds) != 0) rc = -1;
out:
  free(pc); free(pb); free(ds); free(host); free((void*)tabs); free(ft); free(coef);
  return rc;
}

/* ---- the course of a feature call (DESIGN.md sections 10-17) ---- */
/* Every feature kernel reads its clips' rows through one descriptor: the Kaldi pair's carries the clip's valid frames where
 * the others carry the zeros in front of the row.  The course fills pdmp3_mel_desc and hands it to either. */
_Static_assert(sizeof(pdmp3_mel_desc) == 40 && sizeof(pdmp3_fbank_desc) == 40, "one descriptor for every feature kernel");
_Static_assert(offsetof(pdmp3_fbank_desc, src) == offsetof(pdmp3_mel_desc, src) && offsetof(pdmp3_fbank_desc, dst) == offsetof(pdmp3_mel_desc, dst) &&
               offsetof(pdmp3_fbank_desc, src_chan_stride) == offsetof(pdmp3_mel_desc, src_chan_stride) &&
               offsetof(pdmp3_fbank_desc, dst_chan_stride) == offsetof(pdmp3_mel_desc, dst_chan_stride) &&
               offsetof(pdmp3_fbank_desc, valid) == offsetof(pdmp3_mel_desc, lead), "one descriptor for every feature kernel");

typedef struct {
  struct bulk* b;
  const pdmp3_amd_audio_clip* clips;
  int n_clips;
  long long* valid;
  long long F;                       /* frames of a row */
  int C; long sr;                    /* the call's channels and sampling frequency */
  int width; double rolloff;         /* the resampling filter's shape */
  int rc;                            /* 0, or what the clips refused so far say (PDMP3_BULK_REPLAY before PDMP3_BULK_MIXED_FORMAT) */
  size_t per;                        /* floats of a channel's output */
  long long T; size_t Ts;            /* samples of a row: what F frames read; rounded up to four */
  pdmp3_amd_audio_clip* ac;          /* the rows as the audio call takes them */
  long long* av;
  pdmp3_mel_desc* ds;                /* nd descriptors */
  int* host;                         /* per descriptor: its clip, if that one's rows go to host memory, else -1 */
  int nd;
  size_t out_floats;                 /* floats of stage 1 the host destinations' rows take */
  /* the tempogram and separation calls' extension, zero for every other call: a row is read for `front` frames in front of frame 0 and `back`
   * frames behind frame F - 1 as well (valid[] stays relative to `start` and F); per_fixed: floats of a channel's output where
   * they are not per_frame F */
  int front, back;
  size_t per_fixed;
} clip_course;

/* the arguments, and the call's channels and sampling frequency from the clips (0, or -1: nothing is allocated yet) */
static int course_begin(clip_course* cc, struct bulk* b, const pdmp3_amd_audio_clip* clips, int n_clips, long long* valid, long long n_frames,
                        int channels, long rate, int width, double rolloff) {
  memset(cc, 0, sizeof *cc);
  if (!b || !b->hs || !b->bits_mode || n_clips < 0 || (n_clips && (!clips || !valid)) || n_frames < 0) return -1;
  const long long F = n_frames;
  int C = channels;
  long sr = rate;
  if (C < 0 || C > 2 || sr < 0) return -1;
  for (int k = 0; k < n_clips; k++) {
    const pdmp3_amd_audio_clip* c = &clips[k];
    if (!c->index || (!c->mp3 && c->n) || c->n != c->index->n || c->start < 0 || (F && !c->dst)) return -1;
    if ((c->index->iso & PDMP3_ISO_LSF) != (b->id->iso & PDMP3_ISO_LSF)) return -1;
    if (c->index->frames < 0 || c->index->mixed) continue;
    const int cs = c->index->stereo ? 2 : 1;
    if (!channels) {
      if (C && C != cs) return -1;                   /* (no channel count asked for, and the clips' differ) */
      C = cs;
    }
    if (!rate && c->index->frames) {
      if (sr && sr != c->index->rate) return -1;     /* (no rate asked for, and the clips' differ: one time line, one set of tables a call) */
      sr = c->index->rate;
    }
  }
  cc->b = b; cc->clips = clips; cc->n_clips = n_clips; cc->valid = valid;
  cc->F = F; cc->C = C ? C : 1;
  cc->sr = sr ? sr : 44100;                           /* (no clip to decode, or only streams without frames) */
  cc->width = width; cc->rolloff = rolloff;
  return 0;
}

/* The rows of the call: a frame reads N samples, the next one H further on, and writes per_frame floats.  centred: frame f's
 * centre is the sample start + f H -- the row is the span from max(0, start - N / 2) on, `lead` zeros in front of it, and valid
 * counts the frames whose centres lie inside the stream (with cc->front / cc->back the row begins `front` frames earlier and ends
 * `back` frames later; lead counts the zeros in front of that span).  Else frame f begins there -- the row is the span from `start` on, and
 * valid, pdmp3_amd_fbank_valid's, goes into the descriptor too.  Fills valid[], the descriptors and host[] (0, or -1). */
static int course_rows(clip_course* cc, int N, int H, int per_frame, int centred) {
  const long long F = cc->F;
  const int C = cc->C;
  const long long Fr = F ? F + cc->front + cc->back : 0;                                     /* frames a row is read for */
  if (Fr > 0x7fffffffLL / (per_frame > H ? per_frame : H) - 2 * N) return -1;               /* (a row's samples and floats stay inside 31 bits) */
  const size_t per = cc->per = cc->per_fixed ? cc->per_fixed : (size_t)per_frame * (size_t)F;
  for (int k = 0; k < cc->n_clips; k++) if (C == 2 && F && cc->clips[k].chan_stride < per) return -1;
  cc->T = F ? (Fr - 1) * H + N : 0;
  const size_t Ts = cc->Ts = ((size_t)cc->T + 3) & ~(size_t)3;
  cc->ac = (pdmp3_amd_audio_clip*)calloc((size_t)cc->n_clips + 1, sizeof *cc->ac);
  cc->av = (long long*)calloc((size_t)cc->n_clips + 1, sizeof *cc->av);
  cc->ds = (pdmp3_mel_desc*)calloc((size_t)cc->n_clips + 1, sizeof *cc->ds);
  cc->host = (int*)calloc((size_t)cc->n_clips + 1, sizeof *cc->host);
  if (!cc->ac || !cc->av || !cc->ds || !cc->host) return -1;
  for (int k = 0; k < cc->n_clips; k++) {
    const pdmp3_amd_audio_clip* c = &cc->clips[k];
    const pdmp3_amd_index* ix = c->index;
    if (ix->frames < 0) { cc->valid[k] = PDMP3_BULK_REPLAY; cc->rc = PDMP3_BULK_REPLAY; continue; }
    if (ix->mixed) { cc->valid[k] = PDMP3_BULK_MIXED_FORMAT; if (cc->rc != PDMP3_BULK_REPLAY) cc->rc = PDMP3_BULK_MIXED_FORMAT; continue; }
    audio_plan p;
    if (audio_plan_init(&p, ix->frames ? ix->rate : cc->sr, cc->sr, cc->width, cc->rolloff) != 0) return -1;
    const long long Nin = ix->frames * (ix->frames ? ix->spf : 0);
    const long long J = (long long)(((__int128)Nin * p.L + p.M - 1) / p.M);
    const long long left = J - c->start;
    cc->valid[k] = !centred ? pdmp3_amd_fbank_valid(J, c->start, N, H, F) : left <= 0 ? 0 : (left + H - 1) / H < F ? (left + H - 1) / H : F;
    if (!F) continue;
    const long long c0 = c->start - (long long)cc->front * H;                      /* the centre of the row's first frame */
    const long long s0 = !centred ? c->start : c0 > N / 2 ? c0 - N / 2 : 0;
    pdmp3_amd_audio_clip* a = &cc->ac[cc->nd];
    pdmp3_mel_desc* d = &cc->ds[cc->nd];
    a->mp3 = c->mp3; a->n = c->n; a->index = ix;
    a->start = s0;
    a->chan_stride = Ts;
    d->lead = centred ? (uint32_t)(s0 - (c0 - N / 2)) : (uint32_t)cc->valid[k];
    d->src_chan_stride = Ts;
    const size_t row_bytes = ((size_t)(C - 1) * c->chan_stride + per) * sizeof(float);
    if (pdmp3_hip_host_is_pinned(c->dst, row_bytes) == 2) { cc->host[cc->nd] = -1; d->dst = (uint64_t)(uintptr_t)c->dst; d->dst_chan_stride = c->chan_stride; }
    else { cc->host[cc->nd] = k; d->dst = cc->out_floats; d->dst_chan_stride = per; cc->out_floats += (size_t)C * per; }
    cc->nd++;
  }
  return 0;
}

/* the rows through the audio call into stage 2 (device destinations: k_clip_audio writes them itself); the rows of host
 * destinations get their places in stage 1 (0, or -1) */
static int course_signal(clip_course* cc) {
  struct bulk* b = cc->b;
  if (pdmp3_amd_bulk_wait(b) != 0) return -1;
  float* sig = (float*)pdmp3_hip_stream_audio_stage(b->hs, 2, (size_t)cc->nd * (size_t)cc->C * cc->Ts * sizeof(float));
  if (!sig) return -1;
  for (int i = 0; i < cc->nd; i++) {
    cc->ac[i].dst = sig + (size_t)i * (size_t)cc->C * cc->Ts;
    cc->ds[i].src = (uint64_t)(uintptr_t)cc->ac[i].dst;
  }
  pdmp3_amd_audio_spec as;
  memset(&as, 0, sizeof as);
  as.rate = cc->sr; as.channels = cc->C; as.n_samples = cc->T; as.width = cc->width; as.rolloff = cc->rolloff;
  if (pdmp3_amd_bulk_decode_clips_audio(b, cc->ac, cc->nd, &as, cc->av) != 0) return -1;
  /* (the audio call may have grown stage 1 for nothing of ours: it is free for the rows of host destinations) */
  float* out_stage = cc->out_floats ? (float*)pdmp3_hip_stream_audio_stage(b->hs, 1, cc->out_floats * sizeof(float)) : NULL;
  if (cc->out_floats && !out_stage) return -1;
  for (int i = 0; i < cc->nd; i++) if (cc->host[i] >= 0) cc->ds[i].dst = (uint64_t)(uintptr_t)(out_stage + cc->ds[i].dst);
  return 0;
}

/* the launch's verdict (0, or -1 with the engine's text on stderr) */
static int course_launched(int hip_rc) {
  if (hip_rc == PDMP3_HIP_OK) return 0;
  fprintf(stderr, "pdmp3: engine failure: %s\n", pdmp3_hip_last_error());
  return -1;
}

/* the end of every call, a failed one's (rc == -1) too: the rows of host destinations leave the stage, the scratch goes; the
 * call's return value.  It may follow a course_rows that refused before it allocated anything: course_begin zeroed the struct,
 * so nd is 0 and the pointers are NULL then. */
static int course_finish(clip_course* cc, int rc) {
  if (rc != -1 && copy_rows_out(cc->clips, cc->host, cc->nd, cc->C, cc->per, &cc->ds[0].dst, sizeof *cc->ds) != 0) rc = -1;
  free(cc->ac); free(cc->av); free(cc->ds); free(cc->host);
  return rc;
}

/* ---- log-mel features of clips ---- */
/* the decoder's DFT table of n_fft, or (fb) its filterbank as k_clip_mel reads it: [bins16][mels16], made once, kept */
static const mel_tab* mel_table(struct bulk* b, int fb, long sr, const pdmp3_amd_mel_spec* s) {
  const int K = s->n_fft / 2 + 1, Kp = (K + 15) & ~15, Mp = (s->n_mels + 15) & ~15;
  for (mel_tab* t = b->mel_tabs; t; t = t->next) {
    if (t->fb != fb || t->n_fft != s->n_fft) continue;
    if (!fb || (t->sr == sr && t->n_mels == s->n_mels && t->f_min == s->f_min && t->f_max == s->f_max && t->scale == s->scale && t->norm == s->norm))
      return t;
  }
  mel_tab* t = (mel_tab*)calloc(1, sizeof *t);
  if (!t) return NULL;
  t->fb = fb; t->n_fft = s->n_fft;
  if (!fb) {
    t->t = (float*)malloc((size_t)((s->n_fft + 3) & ~3) * (size_t)(2 * Kp) * sizeof(float));
    if (t->t) mel_dft_fill(s->n_fft, t->t);
  } else {
    t->sr = sr; t->n_mels = s->n_mels; t->f_min = s->f_min; t->f_max = s->f_max; t->scale = s->scale; t->norm = s->norm;
    float* w = (float*)malloc((size_t)s->n_mels * (size_t)K * sizeof(float));
    t->t = (float*)calloc((size_t)Kp * (size_t)Mp, sizeof(float));
    if (w && t->t && mel_fb_fill(sr, s->n_fft, s->n_mels, s->f_min, s->f_max, s->scale, s->norm, w) == 0) {
      for (int m = 0; m < s->n_mels; m++)
        for (int k = 0; k < K; k++) t->t[(size_t)k * (size_t)Mp + (size_t)m] = w[(size_t)m * (size_t)K + (size_t)k];
    } else { free(t->t); t->t = NULL; }
    free(w);
  }
  if (!t->t) { free(t); return NULL; }
  t->next = b->mel_tabs;
  b->mel_tabs = t;
  return t;
}

int pdmp3_amd_bulk_decode_clips_mel(struct bulk* b, const pdmp3_amd_audio_clip* clips, int n_clips, const pdmp3_amd_mel_spec* spec,
                                    long long* valid) {
  clip_course cc;
  if (!spec || course_begin(&cc, b, clips, n_clips, valid, spec->n_frames, spec->channels, spec->rate, spec->width, spec->rolloff) != 0) return -1;
  if (pdmp3_amd_mel_check(spec, cc.sr) != 0) return -1;
  pdmp3_mel_params P;
  memset(&P, 0, sizeof P);
  if (mel_plan(spec->n_fft, spec->hop, spec->n_mels, &P) != 0) return -1;
  if (course_rows(&cc, spec->n_fft, spec->hop, spec->n_mels, 1) != 0) return course_finish(&cc, -1);
  if (!cc.nd) return course_finish(&cc, cc.rc);
  const mel_tab* dft = mel_table(b, 0, cc.sr, spec);
  const mel_tab* fbt = mel_table(b, 1, cc.sr, spec);
  if (!dft || !fbt || course_signal(&cc) != 0) return course_finish(&cc, -1);
  P.n_in = cc.T; P.n_frames = (int32_t)cc.F; P.channels = cc.C; P.out_mode = spec->out_mode; P.floor = (float)spec->floor;
  if (course_launched(pdmp3_hip_clip_mel(b->hs, CLIP_SLOT, cc.ds, cc.nd, dft->t, fbt->t, &P)) != 0) return course_finish(&cc, -1);
  return course_finish(&cc, cc.rc);
}

/* ---- the short-time Fourier transform of clips ---- */
int pdmp3_amd_bulk_decode_clips_stft(struct bulk* b, const pdmp3_amd_audio_clip* clips, int n_clips, const pdmp3_amd_stft_spec* spec,
                                     long long* valid) {
  clip_course cc;
  if (!spec || course_begin(&cc, b, clips, n_clips, valid, spec->n_frames, spec->channels, spec->rate, spec->width, spec->rolloff) != 0) return -1;
  if (pdmp3_amd_stft_check(spec, cc.sr) != 0) return -1;
  pdmp3_stft_params P;
  memset(&P, 0, sizeof P);
  if (stft_plan(spec->n_fft, spec->hop, spec->out_mode, &P) != 0) return -1;
  const int per_frame = P.bins * (spec->out_mode == 0 ? 2 : 1);       /* floats of a frame */
  if (course_rows(&cc, spec->n_fft, spec->hop, per_frame, 1) != 0) return course_finish(&cc, -1);
  if (!cc.nd) return course_finish(&cc, cc.rc);
  const float* table = stft_table(b, spec);
  if (!table || course_signal(&cc) != 0) return course_finish(&cc, -1);
  P.n_in = cc.T; P.n_frames = (int32_t)cc.F; P.channels = cc.C; P.floor = spec->out_mode >= 3 ? (float)spec->floor : 0.0f;
  if (course_launched(pdmp3_hip_clip_stft(b->hs, CLIP_SLOT, cc.ds, cc.nd, table, &P)) != 0) return course_finish(&cc, -1);
  return course_finish(&cc, cc.rc);
}

/* ---- the pitch of clips ---- */
int pdmp3_amd_bulk_decode_clips_pitch(struct bulk* b, const pdmp3_amd_audio_clip* clips, int n_clips, const pdmp3_amd_pitch_spec* spec,
                                      long long* valid) {
  clip_course cc;
  if (!spec || course_begin(&cc, b, clips, n_clips, valid, spec->n_frames, spec->channels, spec->rate, spec->width, spec->rolloff) != 0) return -1;
  pdmp3_pitch_params P;
  memset(&P, 0, sizeof P);
  if (pitch_plan(spec, cc.sr, &P) != 0) return -1;                      /* (the check is its first step) */
  const int per_frame = spec->out_mode == 0 ? 3 : P.tmax + 1;            /* floats of a frame */
  if (course_rows(&cc, P.n, P.hop, per_frame, 1) != 0) return course_finish(&cc, -1);
  if (!cc.nd) return course_finish(&cc, cc.rc);
  if (course_signal(&cc) != 0) return course_finish(&cc, -1);
  P.n_in = cc.T; P.n_frames = (int32_t)cc.F; P.channels = cc.C;
  if (course_launched(pdmp3_hip_clip_pitch(b->hs, CLIP_SLOT, cc.ds, cc.nd, &P)) != 0) return course_finish(&cc, -1);
  return course_finish(&cc, cc.rc);
}

/* ---- pYIN pitch tracking of clips ---- */
/* The pitch call's course with its kernel writing the curve into audio stage 3 instead of the destination; behind the clips'
 * curves there lie (mode 0) their observations and their back-pointers. */
int pdmp3_amd_bulk_decode_clips_pyin(struct bulk* b, const pdmp3_amd_audio_clip* clips, int n_clips, const pdmp3_amd_pyin_spec* spec,
                                     long long* valid) {
  clip_course cc;
  if (!spec) return -1;
  pdmp3_amd_pitch_spec ps = spec->pitch;
  ps.threshold = 0.1; ps.out_mode = 1;                                   /* (the curve: no threshold is read) */
  if (course_begin(&cc, b, clips, n_clips, valid, ps.n_frames, ps.channels, ps.rate, ps.width, ps.rolloff) != 0) return -1;
  pdmp3_pitch_params P;
  pdmp3_pyin_params Q;
  memset(&P, 0, sizeof P);
  if (pyin_plan(spec, cc.sr, &Q) != 0 || pitch_plan(&ps, cc.sr, &P) != 0) return -1;   /* (the check is the first step of either) */
  const int mode = spec->out_mode;
  if (course_rows(&cc, P.n, P.hop, mode == 0 ? 4 : Q.n_bins + 1, 1) != 0) return course_finish(&cc, -1);
  if (!cc.nd) return course_finish(&cc, cc.rc);
  const size_t F = (size_t)cc.F, C = (size_t)cc.C;
  const size_t curve_floats = ((size_t)P.tmax + 1) * F;                  /* of a channel in the stage */
  const size_t obs_floats = mode == 0 ? ((size_t)Q.n_bins + 1) * F : 0, bp_floats = mode == 0 ? (size_t)Q.n_bins * F : 0;   /* (two bytes a state) */
  pdmp3_mel_desc* md = (pdmp3_mel_desc*)calloc((size_t)cc.nd, sizeof *md);
  pdmp3_pyin_desc* qd = (pdmp3_pyin_desc*)calloc((size_t)cc.nd, sizeof *qd);
  double* tables = (double*)calloc(pyin_table_bytes(&Q) / sizeof(double) + 1, sizeof *tables);
  int rc = -1;
  if (!md || !qd || !tables || pyin_tables_fill(spec, cc.sr, &Q, tables) != 0 || course_signal(&cc) != 0) goto out;
  float* const stage = (float*)pdmp3_hip_stream_audio_stage(b->hs, 3, (size_t)cc.nd * C * (curve_floats + obs_floats + bp_floats) * sizeof(float));
  if (!stage) goto out;
  float* const obs_stage = stage + (size_t)cc.nd * C * curve_floats;
  float* const bp_stage = obs_stage + (size_t)cc.nd * C * obs_floats;
  for (int i = 0; i < cc.nd; i++) {
    md[i] = cc.ds[i];
    md[i].dst = (uint64_t)(uintptr_t)(stage + (size_t)i * C * curve_floats);
    md[i].dst_chan_stride = curve_floats;
    qd[i].curve = md[i].dst;
    qd[i].dst = cc.ds[i].dst; qd[i].dst_chan_stride = cc.ds[i].dst_chan_stride;
    qd[i].obs = mode == 0 ? (uint64_t)(uintptr_t)(obs_stage + (size_t)i * C * obs_floats) : qd[i].dst;
    qd[i].bp = mode == 0 ? (uint64_t)(uintptr_t)(bp_stage + (size_t)i * C * bp_floats) : 0;
  }
  P.n_in = cc.T; P.n_frames = (int32_t)cc.F; P.channels = cc.C;
  if (course_launched(pdmp3_hip_clip_pitch(b->hs, CLIP_SLOT, md, cc.nd, &P)) != 0) goto out;
  Q.n_frames = (int32_t)cc.F; Q.channels = cc.C;
  if (course_launched(pdmp3_hip_clip_pyin(b->hs, CLIP_SLOT, qd, cc.nd, tables, &Q)) != 0) goto out;
  rc = cc.rc;
out:
  free(md); free(qd); free(tables);
  return course_finish(&cc, rc);
}

/* ---- the short-time Fourier transform of clips at n_fft 2048 and 4096 ---- */
int pdmp3_amd_bulk_decode_clips_stft_long(struct bulk* b, const pdmp3_amd_audio_clip* clips, int n_clips, const pdmp3_amd_stft_spec* spec,
                                          long long* valid) {
  clip_course cc;
  if (!spec || course_begin(&cc, b, clips, n_clips, valid, spec->n_frames, spec->channels, spec->rate, spec->width, spec->rolloff) != 0) return -1;
  if (pdmp3_amd_stft_long_check(spec, cc.sr) != 0) return -1;
  pdmp3_stft_long_params P;
  memset(&P, 0, sizeof P);
  if (stft_long_plan(spec->n_fft, spec->hop, spec->out_mode, &P) != 0) return -1;
  const int per_frame = P.bins * (spec->out_mode == 0 ? 2 : 1);       /* floats of a frame */
  if (course_rows(&cc, spec->n_fft, spec->hop, per_frame, 1) != 0) return course_finish(&cc, -1);
  if (!cc.nd) return course_finish(&cc, cc.rc);
  const float* table = stft_long_tables(b, spec);
  if (!table || course_signal(&cc) != 0) return course_finish(&cc, -1);
  P.n_in = cc.T; P.n_frames = (int32_t)cc.F; P.channels = cc.C; P.floor = spec->out_mode >= 3 ? (float)spec->floor : 0.0f;
  if (course_launched(pdmp3_hip_clip_stft_long(b->hs, CLIP_SLOT, cc.ds, cc.nd, table, &P)) != 0) return course_finish(&cc, -1);
  return course_finish(&cc, cc.rc);
}

/* ---- log-mel features of clips at n_fft 2048 and 4096 ---- */
/* the transform's block of tables with the filterbank operand behind it */
int pdmp3_amd_bulk_decode_clips_mel_long(struct bulk* b, const pdmp3_amd_audio_clip* clips, int n_clips, const pdmp3_amd_mel_long_spec* spec,
                                         long long* valid) {
  clip_course cc;
  if (!spec) return -1;
  const pdmp3_amd_mel_spec* m = &spec->mel;
  if (course_begin(&cc, b, clips, n_clips, valid, m->n_frames, m->channels, m->rate, m->width, m->rolloff) != 0) return -1;
  if (pdmp3_amd_mel_long_check(spec, cc.sr) != 0) return -1;
  pdmp3_mel_long_params P;
  memset(&P, 0, sizeof P);
  if (mel_long_plan(m->n_fft, m->hop, m->n_mels, &P) != 0) return -1;
  if (course_rows(&cc, m->n_fft, m->hop, m->n_mels, 1) != 0) return course_finish(&cc, -1);
  if (!cc.nd) return course_finish(&cc, cc.rc);
  pdmp3_amd_stft_spec frame;
  mel_long_stft_spec(spec, &frame);
  const float* table = stft_long_tables(b, &frame);
  const float* operand = mel_long_operand(b, cc.sr, m);
  if (!table || !operand || course_signal(&cc) != 0) return course_finish(&cc, -1);
  P.n_in = cc.T; P.n_frames = (int32_t)cc.F; P.channels = cc.C; P.out_mode = m->out_mode; P.floor = (float)m->floor;
  if (course_launched(pdmp3_hip_clip_mel_long(b->hs, CLIP_SLOT, cc.ds, cc.nd, table, operand, &P)) != 0) return course_finish(&cc, -1);
  return course_finish(&cc, cc.rc);
}

/* ---- spectral descriptors of clips at n_fft 2048 and 4096 ---- */
int pdmp3_amd_bulk_decode_clips_spectral(struct bulk* b, const pdmp3_amd_audio_clip* clips, int n_clips, const pdmp3_amd_spectral_spec* spec,
                                         long long* valid) {
  clip_course cc;
  if (!spec || course_begin(&cc, b, clips, n_clips, valid, spec->n_frames, spec->channels, spec->rate, spec->width, spec->rolloff) != 0) return -1;
  pdmp3_spectral_params P;
  memset(&P, 0, sizeof P);
  if (spectral_plan(spec, cc.sr, &P) != 0) return -1;                    /* (the check is its first step) */
  if (course_rows(&cc, spec->n_fft, spec->hop, PDMP3_SPECTRAL_ROWS, 1) != 0) return course_finish(&cc, -1);
  if (!cc.nd) return course_finish(&cc, cc.rc);
  pdmp3_amd_stft_spec frame;
  spectral_stft_spec(spec, &frame);
  const float* table = stft_long_tables(b, &frame);
  if (!table || course_signal(&cc) != 0) return course_finish(&cc, -1);
  P.n_in = cc.T; P.n_frames = (int32_t)cc.F; P.channels = cc.C;
  if (course_launched(pdmp3_hip_clip_spectral(b->hs, CLIP_SLOT, cc.ds, cc.nd, table, &P)) != 0) return course_finish(&cc, -1);
  return course_finish(&cc, cc.rc);
}

/* ---- onset strength, tempogram and tempo of clips ---- */
/* The log-mel call's course on rows widened by the frames the flux and the tempogram's window reach, its kernel writing into
 * audio stage 3 instead of the destination; the envelope (modes 1, 2) and the tempogram (mode 2) lie behind the log-mel there. */
int pdmp3_amd_bulk_decode_clips_tempogram(struct bulk* b, const pdmp3_amd_audio_clip* clips, int n_clips, const pdmp3_amd_tempogram_spec* spec,
                                          long long* valid) {
  clip_course cc;
  if (!spec) return -1;
  const pdmp3_amd_mel_spec* m = &spec->mel.mel;
  if (course_begin(&cc, b, clips, n_clips, valid, m->n_frames, m->channels, m->rate, m->width, m->rolloff) != 0) return -1;
  pdmp3_tempogram_params Q;
  pdmp3_mel_long_params P;
  memset(&Q, 0, sizeof Q);
  memset(&P, 0, sizeof P);
  if (tempogram_plan(spec, cc.sr, &Q, &cc.front, &cc.back) != 0) return -1;  /* (the check is its first step) */
  if (mel_long_plan(m->n_fft, m->hop, m->n_mels, &P) != 0) return -1;
  const int mode = spec->out_mode, Wt = spec->win_length;
  if (mode == 2) cc.per_fixed = 4;
  if (course_rows(&cc, m->n_fft, m->hop, mode == 1 ? Wt : 1, 1) != 0) return course_finish(&cc, -1);
  if (!cc.nd) return course_finish(&cc, cc.rc);
  const long long F = cc.F, Fe = mode == 0 ? F : F + Wt - 1, Fm = Fe + spec->lag;
  const size_t mel_floats = (size_t)m->n_mels * (size_t)Fm, env_stride = ((size_t)Fe + 3) & ~(size_t)3;
  const size_t env_floats = mode == 0 ? 0 : env_stride, tg_floats = mode == 2 ? (size_t)Wt * (size_t)F : 0;
  pdmp3_amd_mel_long_spec ms = spec->mel;
  ms.mel.out_mode = 2;
  pdmp3_amd_stft_spec frame;
  mel_long_stft_spec(&ms, &frame);
  const float* table = stft_long_tables(b, &frame);
  const float* operand = mel_long_operand(b, cc.sr, m);
  pdmp3_mel_desc* md = (pdmp3_mel_desc*)calloc((size_t)cc.nd, sizeof *md);
  pdmp3_tempogram_desc* td = (pdmp3_tempogram_desc*)calloc((size_t)cc.nd, sizeof *td);
  float* w = (float*)malloc((size_t)Wt * sizeof *w);
  double* prior = (double*)malloc((size_t)Wt * sizeof *prior);
  int rc = -1;
  if (!table || !operand || !md || !td || !w || !prior || course_signal(&cc) != 0) goto out;
  if (pdmp3_amd_tempogram_window(Wt, w, (size_t)Wt) != Wt || pdmp3_amd_tempogram_prior(spec, cc.sr, prior, (size_t)Wt, NULL) != 0) goto out;
  float* const stage = (float*)pdmp3_hip_stream_audio_stage(b->hs, 3, (size_t)cc.nd * (size_t)cc.C * (mel_floats + env_floats + tg_floats) * sizeof(float));
  if (!stage) goto out;
  float* const env_stage = stage + (size_t)cc.nd * (size_t)cc.C * mel_floats;
  float* const tg_stage = env_stage + (size_t)cc.nd * (size_t)cc.C * env_floats;
  for (int i = 0; i < cc.nd; i++) {
    md[i] = cc.ds[i];
    md[i].dst = (uint64_t)(uintptr_t)(stage + (size_t)i * (size_t)cc.C * mel_floats);
    md[i].dst_chan_stride = mel_floats;
    td[i].mel = md[i].dst;
    td[i].dst = cc.ds[i].dst; td[i].dst_chan_stride = cc.ds[i].dst_chan_stride;
    td[i].env = mode == 0 ? td[i].dst : (uint64_t)(uintptr_t)(env_stage + (size_t)i * (size_t)cc.C * env_floats);
    td[i].tg = mode == 1 ? td[i].dst : mode == 2 ? (uint64_t)(uintptr_t)(tg_stage + (size_t)i * (size_t)cc.C * tg_floats) : 0;
  }
  P.n_in = cc.T; P.n_frames = (int32_t)Fm; P.channels = cc.C; P.out_mode = 2; P.floor = (float)m->floor;
  if (course_launched(pdmp3_hip_clip_mel_long(b->hs, CLIP_SLOT, md, cc.nd, table, operand, &P)) != 0) goto out;
  Q.n_frames = (int32_t)F; Q.n_env = (int32_t)Fe; Q.n_mel_frames = (int32_t)Fm; Q.env_stride = (uint32_t)env_stride; Q.channels = cc.C;
  if (course_launched(pdmp3_hip_clip_tempogram(b->hs, CLIP_SLOT, td, cc.nd, w, prior, &Q)) != 0) goto out;
  rc = cc.rc;
out:
  free(md); free(td); free(w); free(prior);
  return course_finish(&cc, rc);
}

/* ---- harmonic-percussive separation of clips ---- */
/* The two-stage transform's course on rows widened by the frames the harmonic median reaches, its kernel writing into audio
 * stage 3 instead of the destination: magnitudes, or (mode 2) complex values; k_clip_hpss reads them there. */
int pdmp3_amd_bulk_decode_clips_hpss(struct bulk* b, const pdmp3_amd_audio_clip* clips, int n_clips, const pdmp3_amd_hpss_spec* spec,
                                     long long* valid) {
  clip_course cc;
  if (!spec || course_begin(&cc, b, clips, n_clips, valid, spec->n_frames, spec->channels, spec->rate, spec->width, spec->rolloff) != 0) return -1;
  pdmp3_hpss_params Q;
  pdmp3_stft_long_params P;
  memset(&Q, 0, sizeof Q);
  memset(&P, 0, sizeof P);
  if (hpss_plan(spec, cc.sr, &Q, &cc.front, &cc.back) != 0) return -1;       /* (the check is its first step) */
  pdmp3_amd_stft_spec frame;
  hpss_stft_spec(spec, &frame);
  if (stft_long_plan(frame.n_fft, frame.hop, frame.out_mode, &P) != 0) return -1;
  const int e = spec->out_mode == 2 ? 2 : 1;                                  /* floats of a value */
  if (course_rows(&cc, spec->n_fft, spec->hop, 2 * e * P.bins, 1) != 0) return course_finish(&cc, -1);
  if (!cc.nd) return course_finish(&cc, cc.rc);
  const long long F = cc.F, Fs = F + cc.front + cc.back;
  const size_t spec_floats = (size_t)e * (size_t)P.bins * (size_t)Fs;         /* of a channel in the stage */
  const float* table = stft_long_tables(b, &frame);
  pdmp3_mel_desc* sd = (pdmp3_mel_desc*)calloc((size_t)cc.nd, sizeof *sd);
  pdmp3_mel_desc* hd = (pdmp3_mel_desc*)calloc((size_t)cc.nd, sizeof *hd);
  int rc = -1;
  if (!table || !sd || !hd || course_signal(&cc) != 0) goto out;
  float* const stage = (float*)pdmp3_hip_stream_audio_stage(b->hs, 3, (size_t)cc.nd * (size_t)cc.C * spec_floats * sizeof(float));
  if (!stage) goto out;
  for (int i = 0; i < cc.nd; i++) {
    sd[i] = cc.ds[i];
    sd[i].dst = (uint64_t)(uintptr_t)(stage + (size_t)i * (size_t)cc.C * spec_floats);
    sd[i].dst_chan_stride = spec_floats;
    hd[i].src = sd[i].dst; hd[i].src_chan_stride = spec_floats;
    hd[i].dst = cc.ds[i].dst; hd[i].dst_chan_stride = cc.ds[i].dst_chan_stride;
  }
  P.n_in = cc.T; P.n_frames = (int32_t)Fs; P.channels = cc.C; P.floor = 0.0f;
  if (course_launched(pdmp3_hip_clip_stft_long(b->hs, CLIP_SLOT, sd, cc.nd, table, &P)) != 0) goto out;
  Q.n_frames = (int32_t)F; Q.n_stage = (int32_t)Fs; Q.channels = cc.C;
  if (course_launched(pdmp3_hip_clip_hpss(b->hs, CLIP_SLOT, hd, cc.nd, &Q)) != 0) goto out;
  rc = cc.rc;
out:
  free(sd); free(hd);
  return course_finish(&cc, rc);
}

/* ---- MFCC, deltas and dB mel of clips at n_fft 2048 and 4096 ---- */
/* The log-mel call's course on rows widened by the frames the delta stencil reaches, its kernel writing into audio stage 3
 * instead of the destination; behind a clip's log-mel there lies one float per channel, the plane's threshold. */
int pdmp3_amd_bulk_decode_clips_mfcc_long(struct bulk* b, const pdmp3_amd_audio_clip* clips, int n_clips,
                                          const pdmp3_amd_mfcc_long_spec* spec, long long* valid) {
  clip_course cc;
  if (!spec) return -1;
  const pdmp3_amd_mel_spec* m = &spec->mel.mel;
  if (course_begin(&cc, b, clips, n_clips, valid, m->n_frames, m->channels, m->rate, m->width, m->rolloff) != 0) return -1;
  pdmp3_mfcc_long_params Q;
  pdmp3_mel_long_params P;
  memset(&P, 0, sizeof P);
  if (mfcc_long_plan(spec, cc.sr, &Q, &cc.front, &cc.back) != 0) return -1;   /* (the check is its first step) */
  if (mel_long_plan(m->n_fft, m->hop, m->n_mels, &P) != 0) return -1;
  const int rows = spec->out_mode == 1 ? m->n_mels : (1 + spec->deltas) * spec->n_mfcc;
  if (course_rows(&cc, m->n_fft, m->hop, rows, 1) != 0) return course_finish(&cc, -1);
  if (!cc.nd) return course_finish(&cc, cc.rc);
  const long long F = cc.F, Fs = F + cc.front + cc.back;
  const size_t mel_floats = (size_t)m->n_mels * (size_t)Fs;                    /* of a channel in the stage */
  const size_t clip_floats = ((size_t)cc.C * mel_floats + (size_t)cc.C + 3) & ~(size_t)3;
  pdmp3_amd_mel_long_spec ms = spec->mel;
  ms.mel.out_mode = 2;
  pdmp3_amd_stft_spec frame;
  mel_long_stft_spec(&ms, &frame);
  const float* table = stft_long_tables(b, &frame);
  const float* operand = mel_long_operand(b, cc.sr, m);
  const float* dct = spec->out_mode == 0 ? mfcc_long_table(b, m->n_mels, spec->n_mfcc, spec->lifter) : NULL;
  pdmp3_mel_desc* md = (pdmp3_mel_desc*)calloc((size_t)cc.nd, sizeof *md);
  pdmp3_mel_desc* qd = (pdmp3_mel_desc*)calloc((size_t)cc.nd, sizeof *qd);
  int rc = -1;
  if (!table || !operand || (spec->out_mode == 0 && !dct) || !md || !qd || course_signal(&cc) != 0) goto out;
  float* const stage = (float*)pdmp3_hip_stream_audio_stage(b->hs, 3, (size_t)cc.nd * clip_floats * sizeof(float));
  if (!stage) goto out;
  for (int i = 0; i < cc.nd; i++) {
    md[i] = cc.ds[i];
    md[i].dst = (uint64_t)(uintptr_t)(stage + (size_t)i * clip_floats);
    md[i].dst_chan_stride = mel_floats;
    qd[i].src = md[i].dst; qd[i].src_chan_stride = mel_floats;
    qd[i].dst = cc.ds[i].dst; qd[i].dst_chan_stride = cc.ds[i].dst_chan_stride;
  }
  P.n_in = cc.T; P.n_frames = (int32_t)Fs; P.channels = cc.C; P.out_mode = 2; P.floor = (float)m->floor;
  if (course_launched(pdmp3_hip_clip_mel_long(b->hs, CLIP_SLOT, md, cc.nd, table, operand, &P)) != 0) goto out;
  Q.n_frames = (int32_t)F; Q.n_stage = (int32_t)Fs; Q.channels = cc.C;
  if (course_launched(pdmp3_hip_clip_mfcc_long(b->hs, CLIP_SLOT, qd, cc.nd, dct, &Q)) != 0) goto out;
  rc = cc.rc;
out:
  free(md); free(qd);
  return course_finish(&cc, rc);
}

/* ---- Kaldi-style filterbank features of clips ---- */
/* the decoder's folded table of the spec's framing, or (fb) its filterbank as k_clip_fbank reads it: [bins16][mels16], made
 * once, kept */
static const fbank_tab* fbank_table(struct bulk* b, int fb, long sr, const pdmp3_amd_fbank_spec* s) {
  const int N = pdmp3_amd_fbank_dft_length(s->win_length, s->round_to_power_of_two);
  const int K = N / 2, Kp = (K + 15) & ~15, Mp = (s->n_mels + 15) & ~15;
  for (fbank_tab* t = b->fbank_tabs; t; t = t->next) {
    if (t->fb != fb || t->n_dft != N) continue;
    if (fb ? (t->sr == sr && t->n_mels == s->n_mels && t->lo == s->low_freq && t->hi == s->high_freq)
           : (t->win == s->win_length && t->window == s->window && t->dc == s->remove_dc_offset && t->rho == s->preemphasis &&
              t->scale == s->scale && (s->window != 4 || t->b == s->blackman_coeff)))
      return t;
  }
  fbank_tab* t = (fbank_tab*)calloc(1, sizeof *t);
  if (!t) return NULL;
  t->fb = fb; t->n_dft = N;
  if (!fb) {
    t->win = s->win_length; t->window = s->window; t->dc = s->remove_dc_offset; t->rho = s->preemphasis; t->scale = s->scale; t->b = s->blackman_coeff;
    t->t = (float*)malloc((size_t)((s->win_length + 3) & ~3) * (size_t)(2 * Kp) * sizeof(float));
    if (t->t) fbank_table_fill(s, t->t);
  } else {
    t->sr = sr; t->n_mels = s->n_mels; t->lo = s->low_freq; t->hi = s->high_freq;
    float* w = (float*)malloc((size_t)s->n_mels * (size_t)K * sizeof(float));
    t->t = (float*)calloc((size_t)Kp * (size_t)Mp, sizeof(float));
    if (w && t->t) {
      fbank_fb_fill(sr, N, s->n_mels, s->low_freq, s->high_freq, w);
      for (int m = 0; m < s->n_mels; m++)
        for (int k = 0; k < K; k++) t->t[(size_t)k * (size_t)Mp + (size_t)m] = w[(size_t)m * (size_t)K + (size_t)k];
    } else { free(t->t); t->t = NULL; }
    free(w);
  }
  if (!t->t) { free(t); return NULL; }
  t->next = b->fbank_tabs;
  b->fbank_tabs = t;
  return t;
}

/* the decoder's folded DCT table of the spec as k_clip_mfcc reads it: [mels16][ceps16], made once, kept */
static const mfcc_tab* mfcc_table(struct bulk* b, const pdmp3_amd_mfcc_spec* s) {
  const pdmp3_amd_fbank_spec* f = &s->fbank;
  for (mfcc_tab* t = b->mfcc_tabs; t; t = t->next)
    if (t->n_mels == f->n_mels && t->n_ceps == s->num_ceps && t->lifter == s->cepstral_lifter && t->htk == f->htk_compat && t->energy == f->use_energy)
      return t;
  mfcc_tab* t = (mfcc_tab*)calloc(1, sizeof *t);
  if (!t) return NULL;
  t->n_mels = f->n_mels; t->n_ceps = s->num_ceps; t->lifter = s->cepstral_lifter; t->htk = f->htk_compat; t->energy = f->use_energy;
  t->t = (float*)malloc((size_t)((f->n_mels + 15) & ~15) * (size_t)((s->num_ceps + 15) & ~15) * sizeof(float));
  if (!t->t) { free(t); return NULL; }
  mfcc_dct_fill(s, t->t);
  t->next = b->mfcc_tabs;
  b->mfcc_tabs = t;
  return t;
}

/* the filterbank call (mfcc == NULL) and the MFCC call (spec == &mfcc->fbank): they differ in the check, the coefficients of a
 * frame, the plan of a workgroup and the launch.  Their frames begin at `start`: whole-frame rows */
static int kaldi_clips(struct bulk* b, const pdmp3_amd_audio_clip* clips, int n_clips, const pdmp3_amd_fbank_spec* spec,
                       const pdmp3_amd_mfcc_spec* mfcc, long long* valid) {
  clip_course cc;
  if (!spec || course_begin(&cc, b, clips, n_clips, valid, spec->n_frames, spec->channels, spec->rate, spec->width, spec->rolloff) != 0) return -1;
  if ((mfcc ? pdmp3_amd_mfcc_check(mfcc, cc.sr) : pdmp3_amd_fbank_check(spec, cc.sr)) != 0) return -1;
  const int Nw = spec->win_length, H = spec->hop, D = mfcc ? mfcc->num_ceps : spec->n_mels + spec->use_energy;
  pdmp3_mfcc_params Q;
  memset(&Q, 0, sizeof Q);
  pdmp3_fbank_params* const P = &Q.fb;
  if ((mfcc ? mfcc_plan(Nw, pdmp3_amd_fbank_dft_length(Nw, spec->round_to_power_of_two), H, spec->n_mels, mfcc->num_ceps, &Q)
            : fbank_plan(Nw, pdmp3_amd_fbank_dft_length(Nw, spec->round_to_power_of_two), H, spec->n_mels, P)) != 0) return -1;
  if (course_rows(&cc, Nw, H, D, 0) != 0) return course_finish(&cc, -1);
  if (!cc.nd) return course_finish(&cc, cc.rc);
  const fbank_tab* dft = fbank_table(b, 0, cc.sr, spec);
  const fbank_tab* fbt = fbank_table(b, 1, cc.sr, spec);
  const mfcc_tab* dct = mfcc ? mfcc_table(b, mfcc) : NULL;
  if (!dft || !fbt || (mfcc && !dct) || course_signal(&cc) != 0) return course_finish(&cc, -1);
  P->n_in = cc.T; P->n_frames = (int32_t)cc.F; P->channels = cc.C; P->out_mode = spec->out_mode;
  P->use_energy = spec->use_energy; P->htk_compat = spec->htk_compat; P->subtract_mean = spec->subtract_mean; P->remove_dc = spec->remove_dc_offset;
  P->scale = (float)spec->scale; P->eps = 0x1p-23f;
  P->energy_log_floor = spec->energy_floor > 0.0 ? (float)log(spec->energy_floor) : -INFINITY;
  const pdmp3_fbank_desc* ds = (const pdmp3_fbank_desc*)cc.ds;
  if (course_launched(mfcc ? pdmp3_hip_clip_mfcc(b->hs, CLIP_SLOT, ds, cc.nd, dft->t, fbt->t, dct->t, &Q)
                           : pdmp3_hip_clip_fbank(b->hs, CLIP_SLOT, ds, cc.nd, dft->t, fbt->t, P)) != 0) return course_finish(&cc, -1);
  return course_finish(&cc, cc.rc);
}

int pdmp3_amd_bulk_decode_clips_fbank(struct bulk* b, const pdmp3_amd_audio_clip* clips, int n_clips, const pdmp3_amd_fbank_spec* spec,
                                      long long* valid) {
  return kaldi_clips(b, clips, n_clips, spec, NULL, valid);
}

/* ---- Kaldi-style MFCC features of clips ---- */
int pdmp3_amd_bulk_decode_clips_mfcc(struct bulk* b, const pdmp3_amd_audio_clip* clips, int n_clips, const pdmp3_amd_mfcc_spec* spec,
                                     long long* valid) {
  if (!spec) return -1;
  return kaldi_clips(b, clips, n_clips, &spec->fbank, spec, valid);
}

/* ---- the constant-Q transform of clips ---- */
/* With `chroma` (whose cqt is `spec`) the plan is chroma_plan's, a frame n_chroma floats and the kernel
 * k_clip_chroma; the table and its cache are the same. */
static int cqt_clips(struct bulk* b, const pdmp3_amd_audio_clip* clips, int n_clips, const pdmp3_amd_cqt_spec* spec,
                     const pdmp3_amd_chroma_spec* chroma, long long* valid) {
  clip_course cc;
  if (!spec || course_begin(&cc, b, clips, n_clips, valid, spec->n_frames, spec->channels, spec->rate, spec->width, spec->rolloff) != 0) return -1;
  pdmp3_cqt_params P;
  pdmp3_chroma_params S;
  if (chroma) {
    if (chroma_plan(chroma, cc.sr, &S) != 0) return -1;
    P = S.cqt;
  } else if (cqt_plan(spec, cc.sr, &P) != 0) return -1;                /* (the check's verdict and the plan in one) */
  /* a frame reads N = N_0 = 2 h_0 + 1 samples, its centre the sample N / 2 = h_0; the table's rows behind them are zeros */
  const int per_frame = chroma ? chroma->n_chroma : P.n_bins * (spec->out_mode == 0 ? 2 : 1);     /* floats of a frame */
  if (course_rows(&cc, 2 * P.half0 + 1, spec->hop, per_frame, 1) != 0) return course_finish(&cc, -1);
  if (!cc.nd) return course_finish(&cc, cc.rc);
  const float* table = cqt_table(b, spec, cc.sr, &P);
  if (!table || course_signal(&cc) != 0) return course_finish(&cc, -1);
  P.n_in = cc.T; P.n_frames = (int32_t)cc.F; P.channels = cc.C; P.floor = spec->out_mode >= 3 ? (float)spec->floor : 0.0f;
  const size_t table_rows = (size_t)P.tile_at[P.n_tiles - 1] + (size_t)P.tile_rows[P.n_tiles - 1];
  if (chroma) S.cqt = P;
  if (course_launched(chroma ? pdmp3_hip_clip_chroma(b->hs, CLIP_SLOT, cc.ds, cc.nd, table, table_rows, &S)
                             : pdmp3_hip_clip_cqt(b->hs, CLIP_SLOT, cc.ds, cc.nd, table, table_rows, &P)) != 0) return course_finish(&cc, -1);
  return course_finish(&cc, cc.rc);
}
int pdmp3_amd_bulk_decode_clips_cqt(struct bulk* b, const pdmp3_amd_audio_clip* clips, int n_clips, const pdmp3_amd_cqt_spec* spec,
                                    long long* valid) {
  return cqt_clips(b, clips, n_clips, spec, NULL, valid);
}

/* ---- chroma features of clips: the constant-Q call's course, the fold inside its kernel ---- */
int pdmp3_amd_bulk_decode_clips_chroma(struct bulk* b, const pdmp3_amd_audio_clip* clips, int n_clips, const pdmp3_amd_chroma_spec* spec,
                                       long long* valid) {
  if (!spec) return -1;
  return cqt_clips(b, clips, n_clips, &spec->cqt, spec, valid);
}

/* ---- the loudness of clips ---- */
/* The call is a feature call whose "frame" is one sample: the rows through the audio call into stage 2, the kernels behind them.
 * stats and momentary are destinations beside the rows: in device memory the kernel writes clip k's floats itself, for host
 * memory they lie in stage 1 behind the rows of host destinations and are copied out, the floats of consecutive clips in one
 * copy.  With n_samples 0 nothing but valid is written. */
static int copy_floats_out(float* dst, const float* stage, const int* clip_of, int nd, size_t per) {
  for (int i = 0; i < nd; i++) {
    int j = i + 1;
    while (j < nd && clip_of[j] == clip_of[j - 1] + 1) j++;
    if (pdmp3_hip_copy_from_device(dst + (size_t)clip_of[i] * per, stage + (size_t)i * per, (size_t)(j - i) * per * sizeof(float)) != PDMP3_HIP_OK) return -1;
    i = j - 1;
  }
  return 0;
}

/* the loudness call (r128 == NULL) and the true-peak call (spec == &r128->loudness): they differ in the
 * check and plan, the floats of a row of stats (8 or 16), the short-term destination and the launch */
static int loud_clips(struct bulk* b, const pdmp3_amd_audio_clip* clips, int n_clips, const pdmp3_amd_loudness_spec* spec,
                      const pdmp3_amd_r128_spec* r128, float* stats, float* momentary, float* short_term, long long* valid) {
  clip_course cc;
  if (!spec || course_begin(&cc, b, clips, n_clips, valid, spec->n_samples, spec->channels, spec->rate, spec->width, spec->rolloff) != 0) return -1;
  if ((n_clips && !stats) || (r128 ? pdmp3_amd_r128_check(r128, cc.sr, cc.C) : pdmp3_amd_loudness_check(spec, cc.sr, cc.C)) != 0) return -1;
  pdmp3_r128_params Q;
  pdmp3_loud_params* const P = &Q.loud;
  if ((r128 ? r128_plan(cc.sr, spec->n_samples, &Q) : loud_plan(cc.sr, spec->n_samples, P)) != 0) return -1;
  if (course_rows(&cc, 1, 1, 1, 0) != 0) return course_finish(&cc, -1);
  if (!cc.nd) return course_finish(&cc, cc.rc);
  const size_t J = (size_t)P->n_mom, Js = r128 ? (size_t)Q.n_st : 0, S = r128 ? 16 : 8;
  if (!J) momentary = NULL;
  if (!Js) short_term = NULL;
  const int stats_dev = pdmp3_hip_host_is_pinned(stats, (size_t)n_clips * S * sizeof(float)) == 2;
  const int mom_dev = momentary && pdmp3_hip_host_is_pinned(momentary, (size_t)n_clips * J * sizeof(float)) == 2;
  const int st_dev = short_term && pdmp3_hip_host_is_pinned(short_term, (size_t)n_clips * Js * sizeof(float)) == 2;
  const size_t stat_at = cc.out_floats;
  if (!stats_dev) cc.out_floats += (size_t)cc.nd * S;
  const size_t mom_at = cc.out_floats;
  if (momentary && !mom_dev) cc.out_floats += (size_t)cc.nd * J;
  const size_t st_at = cc.out_floats;
  if (short_term && !st_dev) cc.out_floats += (size_t)cc.nd * Js;
  const pdmp3_loud_tables* tab = loud_tables(b, cc.sr);
  int* clip_of = (int*)calloc((size_t)cc.nd, sizeof *clip_of);                 /* the clip of every descriptor */
  uint64_t* at = (uint64_t*)calloc(3 * (size_t)cc.nd, sizeof *at);             /* where its stats go on the device, its momentary, its short-term values */
  int rc = -1;
  if (!tab || !clip_of || !at || course_signal(&cc) != 0) goto out;
  float* const stage = cc.out_floats ? (float*)pdmp3_hip_stream_audio_stage(b->hs, 1, cc.out_floats * sizeof(float)) : NULL;
  if (cc.out_floats && !stage) goto out;
  for (int k = 0, i = 0; k < n_clips; k++) {
    if (clips[k].index->frames < 0 || clips[k].index->mixed) continue;
    clip_of[i] = k;
    at[i] = (uint64_t)(uintptr_t)(stats_dev ? stats + (size_t)k * S : stage + stat_at + (size_t)i * S);
    at[cc.nd + i] = !momentary ? 0 : (uint64_t)(uintptr_t)(mom_dev ? momentary + (size_t)k * J : stage + mom_at + (size_t)i * J);
    at[2 * cc.nd + i] = !short_term ? 0 : (uint64_t)(uintptr_t)(st_dev ? short_term + (size_t)k * Js : stage + st_at + (size_t)i * Js);
    i++;
  }
  P->channels = cc.C; P->dual_mono = spec->dual_mono; P->target = spec->target; P->peak_limit = spec->peak_limit;
  if (r128) {
    float taps[3 * PDMP3_R128_TAPS];
    pdmp3_amd_r128_taps(NULL, taps);
    Q.limit_true_peak = r128->limit_true_peak;
    if (course_launched(pdmp3_hip_clip_r128(b->hs, CLIP_SLOT, cc.ds, cc.nd, tab, taps, at, at + cc.nd, at + 2 * cc.nd, &Q)) != 0) goto out;
  } else if (course_launched(pdmp3_hip_clip_loudness(b->hs, CLIP_SLOT, cc.ds, cc.nd, tab, at, at + cc.nd, P)) != 0) goto out;
  if (!stats_dev && copy_floats_out(stats, stage + stat_at, clip_of, cc.nd, S) != 0) goto out;
  if (momentary && !mom_dev && copy_floats_out(momentary, stage + mom_at, clip_of, cc.nd, J) != 0) goto out;
  if (short_term && !st_dev && copy_floats_out(short_term, stage + st_at, clip_of, cc.nd, Js) != 0) goto out;
  rc = cc.rc;
out:
  free(clip_of); free(at);
  return course_finish(&cc, rc);
}

int pdmp3_amd_bulk_decode_clips_loudness(struct bulk* b, const pdmp3_amd_audio_clip* clips, int n_clips, const pdmp3_amd_loudness_spec* spec,
                                         float* stats, float* momentary, long long* valid) {
  return loud_clips(b, clips, n_clips, spec, NULL, stats, momentary, NULL, valid);
}

/* ---- true peak, short-term loudness and loudness range of clips: the loudness call's course with the
 * short-term values a third destination beside the rows ---- */
int pdmp3_amd_bulk_decode_clips_r128(struct bulk* b, const pdmp3_amd_audio_clip* clips, int n_clips, const pdmp3_amd_r128_spec* spec,
                                     float* stats, float* momentary, float* short_term, long long* valid) {
  if (!spec) return -1;
  return loud_clips(b, clips, n_clips, &spec->loudness, spec, stats, momentary, short_term, valid);
}

/* ---- beat tracking of clips ---- */
/* The tempogram call's course in its mode 0 (bpm given) or 2 (bpm 0) with every output of its kernels in audio stage 3: the
 * log-mel, the envelope, (mode 2) the tempogram, and behind them the beat kernels' scratch of every (clip, channel), whose
 * header takes k_clip_tempo's four floats.  stats is a destination beside the rows, as the loudness call's. */
int pdmp3_amd_bulk_decode_clips_beats(struct bulk* b, const pdmp3_amd_audio_clip* clips, int n_clips, const pdmp3_amd_beat_spec* spec,
                                      float* stats, long long* valid) {
  clip_course cc;
  if (!spec) return -1;
  pdmp3_amd_tempogram_spec tg = spec->tg;
  tg.out_mode = spec->bpm == 0.0 ? 2 : 0;
  const pdmp3_amd_mel_spec* m = &tg.mel.mel;
  if (course_begin(&cc, b, clips, n_clips, valid, m->n_frames, m->channels, m->rate, m->width, m->rolloff) != 0) return -1;
  pdmp3_beat_params B;
  pdmp3_tempogram_params Q;
  pdmp3_mel_long_params P;
  memset(&Q, 0, sizeof Q);
  memset(&P, 0, sizeof P);
  if (beat_plan(spec, cc.sr, &B) != 0 || tempogram_plan(&tg, cc.sr, &Q, &cc.front, &cc.back) != 0) return -1;   /* (the check is the first step of either) */
  if (mel_long_plan(m->n_fft, m->hop, m->n_mels, &P) != 0) return -1;
  const int tmode = tg.out_mode, Wt = tg.win_length;
  if (course_rows(&cc, m->n_fft, m->hop, spec->out_mode == 0 ? 1 : 2, 1) != 0) return course_finish(&cc, -1);
  if (!cc.nd) return course_finish(&cc, cc.rc);
  const size_t C = (size_t)cc.C, S = 8 * C;
  const int stats_dev = stats && pdmp3_hip_host_is_pinned(stats, (size_t)n_clips * S * sizeof(float)) == 2;
  const size_t stat_at = cc.out_floats;
  if (stats && !stats_dev) cc.out_floats += (size_t)cc.nd * S;
  const long long F = cc.F, Fe = tmode == 0 ? F : F + Wt - 1, Fm = Fe + tg.lag;
  const size_t mel_floats = (size_t)m->n_mels * (size_t)Fm, env_floats = ((size_t)Fe + 3) & ~(size_t)3;
  const size_t tg_floats = tmode == 2 ? (size_t)Wt * (size_t)F : 0;
  const size_t front_floats = ((size_t)cc.nd * C * (mel_floats + env_floats + tg_floats) + 1) & ~(size_t)1;   /* (the scratch is binary64) */
  pdmp3_amd_mel_long_spec ms = tg.mel;
  ms.mel.out_mode = 2;
  pdmp3_amd_stft_spec frame;
  mel_long_stft_spec(&ms, &frame);
  const float* table = stft_long_tables(b, &frame);
  const float* operand = mel_long_operand(b, cc.sr, m);
  pdmp3_mel_desc* md = (pdmp3_mel_desc*)calloc((size_t)cc.nd, sizeof *md);
  pdmp3_tempogram_desc* td = (pdmp3_tempogram_desc*)calloc((size_t)cc.nd, sizeof *td);
  pdmp3_beat_desc* bd = (pdmp3_beat_desc*)calloc((size_t)cc.nd, sizeof *bd);
  int* clip_of = (int*)calloc((size_t)cc.nd, sizeof *clip_of);
  float* w = (float*)malloc((size_t)Wt * sizeof *w);
  double* prior = (double*)malloc((size_t)Wt * sizeof *prior);
  double* tables = (double*)malloc(beat_table_bytes(&B) + sizeof(double));
  int rc = -1;
  if (!table || !operand || !md || !td || !bd || !clip_of || !w || !prior || !tables || course_signal(&cc) != 0) goto out;
  if (pdmp3_amd_tempogram_window(Wt, w, (size_t)Wt) != Wt || pdmp3_amd_tempogram_prior(&tg, cc.sr, prior, (size_t)Wt, NULL) != 0) goto out;
  if (beat_tables_fill(spec, &B, tables) != 0) goto out;
  float* const out_stage = cc.out_floats ? (float*)pdmp3_hip_stream_audio_stage(b->hs, 1, cc.out_floats * sizeof(float)) : NULL;
  float* const stage = (float*)pdmp3_hip_stream_audio_stage(b->hs, 3, (front_floats + 2 * (size_t)cc.nd * C * (size_t)B.work_stride) * sizeof(float));
  if (!stage || (cc.out_floats && !out_stage)) goto out;
  float* const env_stage = stage + (size_t)cc.nd * C * mel_floats;
  float* const tg_stage = env_stage + (size_t)cc.nd * C * env_floats;
  double* const work = (double*)(stage + front_floats);
  for (int k = 0, i = 0; k < n_clips; k++) {
    if (clips[k].index->frames < 0 || clips[k].index->mixed) continue;
    clip_of[i] = k;
    md[i] = cc.ds[i];
    md[i].dst = (uint64_t)(uintptr_t)(stage + (size_t)i * C * mel_floats);
    md[i].dst_chan_stride = mel_floats;
    td[i].mel = md[i].dst;
    td[i].env = (uint64_t)(uintptr_t)(env_stage + (size_t)i * C * env_floats);
    if (tmode == 0) { td[i].dst = td[i].env; td[i].dst_chan_stride = env_floats; }        /* (mode 0 writes the envelope as its rows) */
    else {
      td[i].tg = (uint64_t)(uintptr_t)(tg_stage + (size_t)i * C * tg_floats);
      td[i].dst = (uint64_t)(uintptr_t)(work + (size_t)i * C * (size_t)B.work_stride);  /* the scratch's header */
      td[i].dst_chan_stride = 2 * (size_t)B.work_stride;
    }
    bd[i].env = td[i].env + (tmode == 2 ? (uint64_t)(Wt / 2) * sizeof(float) : 0);
    bd[i].stats = !stats ? 0 : (uint64_t)(uintptr_t)(stats_dev ? stats + (size_t)k * S : out_stage + stat_at + (size_t)i * S);
    bd[i].dst = cc.ds[i].dst; bd[i].dst_chan_stride = cc.ds[i].dst_chan_stride;
    bd[i].n = (uint32_t)cc.valid[k];
    i++;
  }
  P.n_in = cc.T; P.n_frames = (int32_t)Fm; P.channels = cc.C; P.out_mode = 2; P.floor = (float)m->floor;
  if (course_launched(pdmp3_hip_clip_mel_long(b->hs, CLIP_SLOT, md, cc.nd, table, operand, &P)) != 0) goto out;
  Q.n_frames = (int32_t)F; Q.n_env = (int32_t)Fe; Q.n_mel_frames = (int32_t)Fm; Q.env_stride = (uint32_t)env_floats; Q.channels = cc.C;
  if (course_launched(pdmp3_hip_clip_tempogram(b->hs, CLIP_SLOT, td, cc.nd, w, prior, &Q)) != 0) goto out;
  B.env_stride = (uint32_t)env_floats; B.channels = cc.C;
  if (course_launched(pdmp3_hip_clip_beat(b->hs, CLIP_SLOT, bd, cc.nd, tables, work, &B)) != 0) goto out;
  if (stats && !stats_dev && copy_floats_out(stats, out_stage + stat_at, clip_of, cc.nd, S) != 0) goto out;
  rc = cc.rc;
out:
  free(md); free(td); free(bd); free(clip_of); free(w); free(prior); free(tables);
  return course_finish(&cc, rc);
}
