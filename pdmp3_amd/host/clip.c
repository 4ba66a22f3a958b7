/* clip.c -- libpdmp3.so: stream indices, the exact halo of a frame range, and the whole-stream decoder's clips
 * (include/pdmp3_bulk.h: pdmp3_amd_index_*, pdmp3_amd_bulk_decode_clips, pdmp3_amd_bulk_parse_range).  The halo rule and
 * its reasoning: DESIGN.md section 8.  See host_internal.h for the map of the library. */
#include "bulk_internal.h"
#include "../../include/pdmp3_node.h"

#include <math.h>

#define IX_SPACING 256               /* frames between two snapshots: a clip's scan starts at most this far in front of it */

/* What a frame does to the state the merge carries from frame to frame (frame_parse.c apply_main, unpack_core.h): per
 * granule-channel g four bits -- present (ch < nch, and granule 0 of an LSF frame), short block, mixed block, count1
 * written (part2_3_length != 0 or LSF, H6) -- the scfsi bits of both channels and the LSF bit. */
#define HB_PRESENT 1u
#define HB_SHORT 2u
#define HB_MIXED 4u
#define HB_COUNT1 8u
#define HB_SCFSI_SHIFT 16
#define HB_LSF (1u << 24)
/* The state in groups, eight per granule-channel g (bit 8 g + k): scalefac_l bands 0-5, 6-7, 8-10, 11-15, 16-20 (the scfsi
 * groups, the second split where a mixed block stops), scalefac_s bands 0-2, 3-11 (a mixed block writes the second only),
 * count1. */
#define IX_GROUPS 32

struct pdmp3_amd_index {
  long long frames;                  /* or PDMP3_BULK_REPLAY */
  size_t n;                          /* bytes of the stream it was built from */
  unsigned iso;                      /* PDMP3_ISO_LSF or 0 */
  int spacing;
  int split;                         /* the pre-pass took the stream: rec / snap are there */
  int oom;
  long long cap;                     /* capacity of the per-frame arrays (while building) */
  long long* off;                    /* [frames + 1] PCM bytes in front of each frame */
  uint8_t* fr;                       /* [frames] PDMP3_FR mode bits and RESET (what pdmp3_node_halo_start reads) */
  uint32_t* hb;                      /* [frames] HB_* */
  int32_t* org;                      /* [frames / spacing + 1][IX_GROUPS]: in front of frame k * spacing, the frame each group's
                                        value came from (-1: none since the stream's start, the value is 0) */
  hop_rec* rec;                      /* split: the pre-pass's records */
  span_snap* snap; long long n_snap; /* split: snap[k] in front of frame k * spacing (k >= 1, where ready) */
  long rate; int spf;                /* the first frame's sampling frequency and samples per frame and channel ... */
  int mixed, stereo;                 /* ... a later frame's differ (no time line: DESIGN.md section 9); some frame is stereo */
};

/* granule 0's writes (w0), granule 1's copies from granule 0 (cp, as bits of gc 2 / 3), granule 1's writes (w1) and the groups
 * the frame's records read (rd: every group of a present granule-channel, and the first band of the next one's scalefac_l /
 * scalefac_s, which the records carry as the reference's one-past-the-end values) */
static void hb_effect(uint32_t hb, uint32_t* w0, uint32_t* cp, uint32_t* w1, uint32_t* rd) {
  static const uint32_t g4m[4] = {0x01, 0x06, 0x08, 0x10};
  *w0 = *cp = *w1 = *rd = 0;
  for (unsigned g = 0; g < 4; g++) {
    const unsigned q = (hb >> (4 * g)) & 15u, gr = g >> 1, ch = g & 1;
    if (!(q & HB_PRESENT)) continue;
    uint32_t w = 0, c = 0;
    if (hb & HB_LSF) w = 0x7f;                      /* (an LSF granule writes every scalefactor) */
    else if (q & HB_SHORT) w = (q & HB_MIXED) ? 0x43 : 0x60;
    else
      for (unsigned k = 0; k < 4; k++) {
        if (gr == 1 && ((hb >> (HB_SCFSI_SHIFT + 4 * ch + k)) & 1u)) c |= g4m[k];
        else w |= g4m[k];
      }
    if (q & HB_COUNT1) w |= 0x80;
    if (gr) { *w1 |= w << (8 * g); *cp |= c << (8 * g); }
    else *w0 |= w << (8 * g);
    *rd |= 0xffu << (8 * g);
    *rd |= g < 3 ? 0x21u << (8 * (g + 1)) : 0x20u;
  }
}
/* the origins after frame f */
static void org_step(int32_t* org, uint32_t hb, int32_t f) {
  uint32_t w0, cp, w1, rd;
  hb_effect(hb, &w0, &cp, &w1, &rd);
  for (unsigned i = 0; i < IX_GROUPS; i++) if ((w0 >> i) & 1u) org[i] = f;
  for (unsigned i = 16; i < IX_GROUPS; i++) if ((cp >> i) & 1u) org[i] = org[i - 16];
  for (unsigned i = 0; i < IX_GROUPS; i++) if ((w1 >> i) & 1u) org[i] = f;
}

/* the first frame a decode of [a, b) has to start at */
static long long ix_first(const pdmp3_amd_index* ix, long long a, long long b, int lookback) {
  if (a <= 0) return 0;
  /* synthesis state: node.hip, the node layer's own rule -- the state in front of `a` is a function of the records of
   * [s, a) alone, whatever the state in front of s was */
  const long long s = pdmp3_node_halo_start(a, ix->fr);
  if (!lookback) return s;
  /* ... so the records of [s, b) must be the whole stream's: every group they read before they write it must hold the
   * whole stream's value at s, which it does when the decode starts at or before the frame that value came from */
  long long first = s;
  int32_t org[IX_GROUPS];
  const long long k = s / ix->spacing;
  memcpy(org, ix->org + k * IX_GROUPS, sizeof org);
  for (long long f = k * ix->spacing; f < s; f++) org_step(org, ix->hb[f], (int32_t)f);
  /* the groups [s, b) reads before it writes them */
  uint32_t done = 0, live = 0;
  for (long long f = s; f < b && (done | live) != 0xffffffffu; f++) {
    uint32_t w0, cp, w1, rd;
    hb_effect(ix->hb[f], &w0, &cp, &w1, &rd);
    done |= w0;
    live |= (cp >> 16) & ~done;                    /* a copy reads granule 0's group after granule 0's writes */
    done |= cp | w1;
    live |= rd & ~done;
  }
  for (unsigned i = 0; i < IX_GROUPS; i++)
    if (((live >> i) & 1u) && org[i] >= 0 && org[i] < first) first = org[i];
  return first;
}

/* ---- building an index ---- */
static void ix_note(struct bulk* b) {                /* bulk_push, count-only scan: the frame just staged */
  pdmp3_amd_index* ix = b->ix;
  const long long f = b->frames - 1;
  if (ix->oom) return;
  if (f + 1 >= ix->cap) {
    const long long cap = ix->cap * 2 + 1024;
    long long* off = (long long*)realloc(ix->off, (size_t)(cap + 1) * sizeof *off);
    if (off) ix->off = off;
    uint8_t* fr = (uint8_t*)realloc(ix->fr, (size_t)cap);
    if (fr) ix->fr = fr;
    uint32_t* hb = (uint32_t*)realloc(ix->hb, (size_t)cap * sizeof *hb);
    if (hb) ix->hb = hb;
    if (!off || !fr || !hb) { ix->oom = 1; return; }
    ix->cap = cap;
  }
  const pdmp3_handle* id = b->id;
  const frame_header* H = &id->hdr;
  const side_info* S = &id->si;
  const unsigned nch = H->mode == 3 ? 1 : 2;
  ix->off[f + 1] = ix->off[f] + 2LL * frame_samples(H) * nch;
  const long rate = (long)kLsfSampleRates[sfreq9(H)];
  if (f == 0) { ix->rate = rate; ix->spf = (int)frame_samples(H); }
  else if (rate != ix->rate || (int)frame_samples(H) != ix->spf) ix->mixed = 1;
  if (nch == 2) ix->stereo = 1;
  ix->fr[f] = (uint8_t)((H->mode << PDMP3_FR_MODE_SHIFT) | (id->need_reset ? PDMP3_FR_RESET : 0));
  uint32_t hb = H->ver ? HB_LSF : 0;
  for (unsigned ch = 0; ch < nch; ch++)
    for (unsigned k = 0; k < 4; k++) if (S->scfsi[ch][k]) hb |= 1u << (HB_SCFSI_SHIFT + 4 * ch + k);
  for (unsigned g = 0; g < 4; g++) {
    const unsigned gr = g >> 1, ch = g & 1;
    if (ch >= nch || (H->ver && gr == 1)) continue;
    unsigned q = HB_PRESENT;
    if (S->win_switch[gr][ch] && S->block_type[gr][ch] == 2) q |= HB_SHORT | (S->mixed[gr][ch] ? HB_MIXED : 0);
    if (S->part2_3_length[gr][ch] != 0 || H->ver) q |= HB_COUNT1;
    hb |= q << (4 * g);
  }
  ix->hb[f] = hb;
}

void pdmp3_amd_index_delete(pdmp3_amd_index* ix) {
  if (!ix) return;
  if (ix->snap) for (long long k = 0; k < ix->n_snap; k++) free(ix->snap[k].sky);
  free(ix->snap); free(ix->rec); free(ix->org); free(ix->off); free(ix->fr); free(ix->hb);
  free(ix);
}

/* the split scan's pre-pass over the whole stream on the calling thread, with a snapshot every `spacing` frames */
static void ix_prepass(pdmp3_amd_index* ix, const unsigned char* mp3, size_t n) {
  if (!mp3 || ix->frames <= ix->spacing || n > 0xfff00000u) return;
  struct par_scan* P = (struct par_scan*)calloc(1, sizeof *P);
  if (!P) return;
  P->mp3 = mp3; P->n = n; P->K = 1; P->J = 1; P->sub = ix->spacing; P->t0 = now_s();
  P->published = 1;
  P->rec_cap = (long long)(n / 96) + 8;             /* (no Layer III frame is shorter than 96 bytes) */
  P->rec = (hop_rec*)malloc((size_t)P->rec_cap * sizeof(hop_rec));
  P->snap_cap = P->rec_cap / ix->spacing + 8;
  P->snap = (span_snap*)calloc((size_t)P->snap_cap, sizeof(span_snap));
  pthread_mutex_init(&P->mu, NULL); pthread_cond_init(&P->cv, NULL);
  if (P->rec && P->snap && par_prepass(P) == 0 && P->n_frames == ix->frames) {
    /* (the pre-pass sized its arrays by the stream's bytes: the records of frames [0, frames) and the snapshots up to the
     *  last frame are all a scan reads) */
    const long long keep = ix->frames / ix->spacing + 1;
    for (long long k = keep; k < P->snap_cap; k++) { free(P->snap[k].sky); P->snap[k].sky = NULL; }
    hop_rec* rec = (hop_rec*)realloc(P->rec, (size_t)ix->frames * sizeof(hop_rec));
    span_snap* snap = (span_snap*)realloc(P->snap, (size_t)keep * sizeof(span_snap));
    if (rec) P->rec = rec;
    if (snap) { P->snap = snap; P->snap_cap = keep; }
    ix->split = 1;
    ix->rec = P->rec; P->rec = NULL;
    ix->snap = P->snap; ix->n_snap = P->snap_cap; P->snap = NULL;
  }
  if (P->snap) for (long long k = 0; k < P->snap_cap; k++) free(P->snap[k].sky);
  free(P->snap); free(P->rec);
  pthread_mutex_destroy(&P->mu); pthread_cond_destroy(&P->cv);
  free(P);
}

pdmp3_amd_index* pdmp3_amd_index_new_spacing(const unsigned char* mp3, size_t n, unsigned iso_mask, int spacing) {
  pthread_once(&g_lut_once, build_luts);
  if (!mp3 && n) return NULL;
  pdmp3_amd_index* ix = (pdmp3_amd_index*)calloc(1, sizeof *ix);
  if (!ix) return NULL;
  ix->n = n; ix->iso = iso_mask & PDMP3_ISO_LSF; ix->spacing = spacing > 0 ? spacing : IX_SPACING;
  ix->cap = 1024;
  ix->off = (long long*)calloc((size_t)ix->cap + 1, sizeof *ix->off);
  ix->fr = (uint8_t*)malloc((size_t)ix->cap);
  ix->hb = (uint32_t*)malloc((size_t)ix->cap * sizeof *ix->hb);
  struct bulk* b = (struct bulk*)calloc(1, sizeof *b);
  if (b) b->id = (pdmp3_handle*)calloc(1, sizeof *b->id);
  if (!ix->off || !ix->fr || !ix->hb || !b || !b->id) { if (b) free(b->id); free(b); pdmp3_amd_index_delete(ix); return NULL; }
  /* the one-thread scan, count only (pdmp3_amd_scan_buffer_iso), noting every frame */
  b->id->host_only = 1;
  b->id->iso = iso_mask & (PDMP3_ISO_ALL | PDMP3_ISO_LSF);
  b->count_only = 1;
  b->ix_note = ix_note; b->ix = ix;
  const long long total = bulk_drive(b, mp3 ? mp3 : (const unsigned char*)"", mp3 ? n : 0);
  const long long frames = b->frames;
  free(b->id); free(b);
  if (ix->oom) { pdmp3_amd_index_delete(ix); return NULL; }
  if (total == PDMP3_BULK_REPLAY) { ix->frames = PDMP3_BULK_REPLAY; return ix; }
  ix->frames = frames;
  if (total != ix->off[frames]) {                   /* (the scan's own byte count: cannot differ) */
    fprintf(stderr, "pdmp3: stream index: %lld PCM bytes by frame, %lld by the scan\n", ix->off[frames], total);
    pdmp3_amd_index_delete(ix);
    return NULL;
  }
  {                                                 /* (grown by doubling while the scan ran) */
    const size_t keep = (size_t)(frames > 0 ? frames : 1);
    long long* off = (long long*)realloc(ix->off, (keep + 1) * sizeof *off);
    if (off) ix->off = off;
    uint8_t* fr = (uint8_t*)realloc(ix->fr, keep);
    if (fr) ix->fr = fr;
    uint32_t* hb = (uint32_t*)realloc(ix->hb, keep * sizeof *hb);
    if (hb) ix->hb = hb;
    ix->cap = (long long)keep;
  }
  /* the halo rule's checkpoints */
  ix->org = (int32_t*)malloc((size_t)(frames / ix->spacing + 1) * IX_GROUPS * sizeof(int32_t));
  if (!ix->org) { pdmp3_amd_index_delete(ix); return NULL; }
  int32_t org[IX_GROUPS];
  for (unsigned i = 0; i < IX_GROUPS; i++) org[i] = -1;
  for (long long f = 0; f <= frames; f++) {
    if (f % ix->spacing == 0) memcpy(ix->org + (f / ix->spacing) * IX_GROUPS, org, sizeof org);
    if (f < frames) org_step(org, ix->hb[f], (int32_t)f);
  }
  ix_prepass(ix, mp3, n);
  return ix;
}
pdmp3_amd_index* pdmp3_amd_index_new(const unsigned char* mp3, size_t n, unsigned iso_mask) {
  return pdmp3_amd_index_new_spacing(mp3, n, iso_mask, 0);
}
long long pdmp3_amd_index_frames(const pdmp3_amd_index* ix) { return ix ? ix->frames : -1; }
long long pdmp3_amd_index_pcm_offset(const pdmp3_amd_index* ix, long long frame) {
  if (!ix || ix->frames < 0 || frame < 0 || frame > ix->frames) return -1;
  return ix->off[frame];
}
long long pdmp3_amd_index_pcm_offsets(const pdmp3_amd_index* ix, long long* out, size_t cap) {
  if (!ix) return -1;
  if (ix->frames < 0) return ix->frames;
  const size_t k = (size_t)ix->frames + 1 < cap ? (size_t)ix->frames + 1 : cap;
  if (out && k) memcpy(out, ix->off, k * sizeof *out);
  return ix->frames + 1;
}
int pdmp3_amd_index_split(const pdmp3_amd_index* ix) { return ix ? ix->split : 0; }
int pdmp3_amd_index_format(const pdmp3_amd_index* ix, long* rate, int* channels, int* frame_samples) {
  if (!ix || ix->frames < 0) return -1;
  if (channels) *channels = ix->stereo ? 2 : 1;
  if (ix->mixed) return 0;
  if (rate) *rate = ix->rate;
  if (frame_samples) *frame_samples = ix->spf;
  return 1;
}
long long pdmp3_amd_index_samples(const pdmp3_amd_index* ix) {
  return ix && ix->frames >= 0 && !ix->mixed ? ix->frames * ix->spf : -1;
}

/* ---- scanning a range ---- */
/* bulk_drive's loop from wherever the handle stands (fed: stream bytes fed so far), until the sink's frame limit.
 * 0, -1 or PDMP3_BULK_REPLAY */
static long long ix_drive(struct bulk* s, const unsigned char* mp3, size_t n, size_t* fed_io) {
  pdmp3_handle* id = s->id;
  size_t fed = *fed_io, done;
  int res;
  while (!bulk_at_limit(s) && (res = read_impl_sink(id, INBUF_SIZE, &done, s)) != PDMP3_ERR) {
    if (s->failed) break;
    if (id->processed > fed) { *fed_io = fed; return PDMP3_BULK_REPLAY; }      /* (the index says so first) */
    if (res == PDMP3_NEED_MORE) {
      const size_t take = n - fed < 4096 ? n - fed : 4096;
      if (!take) break;
      if (id->vsrc && take > ring_free_logical(id)) {                         /* H16: as bulk_drive */
        for (unsigned k = 0, f = ring_filled(id); k < f; k++) id->in[(id->istart + k) % INBUF_SIZE] = id->vsrc[id->vfed - f + k];
        id->vsrc = NULL;
      }
      (void)pdmp3_feed(id, mp3 + fed, take);
      fed += take;
    }
  }
  *fed_io = fed;
  return s->failed ? -1 : 0;
}

/* Frames [first, first + count) as the whole-stream scan sees them, into the sink `s` (host records, or bits + snapshot
 * rows), from the index's nearest snapshot at or before `first` (frame 0 without one): the frames in front of `first` are
 * scanned count-only; `first` then starts like a stream's first frame -- PDMP3_FR_RESET, and the parse state that survives
 * frames at zero (the records: PDMP3_FR_NEWSTREAM) -- so that its records are the decode of [first, ...) by itself.  The
 * handle's switches and scan flags are kept.  Returns the frames delivered, -1 or PDMP3_BULK_REPLAY. */
static long long ix_scan(const pdmp3_amd_index* ix, const unsigned char* mp3, size_t n, long long first, long long count, struct bulk* s) {
  pdmp3_handle* id = s->id;
  const unsigned iso = id->iso;
  const int stb = id->side_to_bits, bs = id->bits_scan, bl = id->bits_lsf;
  memset(id, 0, sizeof *id);
  id->host_only = 1;
  id->iso = iso;
  size_t fed = 0;
  const long long k = ix->split ? first / ix->spacing : 0;
  if (k >= 1 && k < ix->n_snap && ix->snap[k].ready) {
    span_init(mp3, ix->rec, &ix->snap[k], id);
    fed = ix->snap[k].fed;
    s->frames = ix->snap[k].frame;
  } else {
    pdmp3_open_feed(id);
    id->vsrc = mp3; id->vfed = 0;
    s->frames = 0;
  }
  id->side_to_bits = stb; id->bits_scan = bs; id->bits_lsf = bl; id->pool_sink = NULL;
  s->failed = 0; s->bits_open = 0; s->bits_n = 0;
  long long rc;
  if (s->frames < first) {
    s->count_only = 1; s->limit_frames = first;
    rc = ix_drive(s, mp3, n, &fed);
    if (rc < 0) return rc;
    if (s->frames != first) return -1;
  }
  s->count_only = 0; s->frames = 0; s->limit_frames = count;
  id->need_reset = 1;
  memset(id->scalefac_l, 0, sizeof id->scalefac_l);
  memset(id->scalefac_s, 0, sizeof id->scalefac_s);
  memset(id->count1, 0, sizeof id->count1);
  rc = ix_drive(s, mp3, n, &fed);
  s->limit_frames = 0;
  if (rc < 0) return rc;
  return s->frames;
}

static void clamp_range(const pdmp3_amd_index* ix, long long first, long long count, long long* a, long long* e) {
  if (first < 0) first = 0;
  if (first > ix->frames) first = ix->frames;
  if (count < 0) count = 0;
  if (count > ix->frames - first) count = ix->frames - first;
  *a = first; *e = first + count;
}

/* ---- the host tests' form ---- */
long long pdmp3_amd_bulk_parse_range(struct bulk* b, const unsigned char* mp3, size_t n, const pdmp3_amd_index* ix,
                                     long long first_frame, long long n_frames, int lookback, int16_t* spectra, pdmp3_gc_side* side,
                                     size_t cap_frames, long long* decoded_from) {
  if (!b || b->hs || b->bits_mode || !ix || ix->n != n || (!mp3 && n)) return -1;
  if (ix->frames < 0) return ix->frames;
  if ((ix->iso & PDMP3_ISO_LSF) != (b->id->iso & PDMP3_ISO_LSF)) return -1;
  long long a, e;
  clamp_range(ix, first_frame, n_frames, &a, &e);
  const long long f0 = a < e ? ix_first(ix, a, e, lookback) : a;
  if (decoded_from) *decoded_from = f0;
  if (a == e) return 0;
  if ((size_t)(e - f0) > cap_frames || !spectra || !side) return -1;
  bulk_begin(b);
  b->rec_spectra = spectra; b->rec_side = side; b->rec_cap = cap_frames;
  const long long got = ix_scan(ix, mp3, n, f0, e - f0, b);
  int ok = got == e - f0 && !b->failed && bulk_rotate(b) == PDMP3_OK;
  ok = bulk_finish_b(b) == PDMP3_OK && ok;
  bulk_wait_b(b);
  b->in_b = NULL;
  if (got == PDMP3_BULK_REPLAY) return PDMP3_BULK_REPLAY;
  return ok ? got : -1;
}

/* ---- clips on the GPU ---- */
typedef struct { unsigned char* dst; size_t off, bytes; } stage_copy;
typedef struct {
  int n, kind;                        /* frames in the window, their kind: 0 MPEG-1, else (version << 1) | mono (LSF) */
  int np, nh;
  size_t stage;                       /* bytes of the slot's clip stage taken */
  pdmp3_clip_piece* pieces;
  stage_copy* copies;                 /* host destinations: stage bytes -> caller memory, after the download */
} clip_win;
#define CLIP_SLOT 0
/* where frame i of a window of this kind lies in the slot's PCM (include/pdmp3_hip.h pdmp3_hip_decode_lsf_frames) */
static uint32_t clip_src(int kind, int i) {
  if (!kind) return (uint32_t)i * PDMP3_FRAME_PCM_BYTES;
  if (!(kind & 1)) return (uint32_t)i * (PDMP3_FRAME_PCM_BYTES / 2);
  return (uint32_t)(i >> 1) * PDMP3_FRAME_PCM_BYTES + (uint32_t)(i & 1) * (PDMP3_FRAME_PCM_BYTES / 4);
}
static int clip_flush(struct bulk* b, clip_win* W) {
  if (!W->n) return 0;
  int ok = pdmp3_hip_stream_set_lsf(b->hs, W->kind != 0) == PDMP3_HIP_OK &&
           pdmp3_hip_stream_submit_bits_clips(b->hs, CLIP_SLOT, W->n, W->pieces, W->np, W->stage) == PDMP3_HIP_OK;
  ok = pdmp3_hip_stream_wait(b->hs, CLIP_SLOT) == PDMP3_HIP_OK && ok;
  if (!ok) fprintf(stderr, "pdmp3: engine failure: %s\n", pdmp3_hip_last_error());
  if (ok && W->nh) {
    const unsigned char* src = (const unsigned char*)pdmp3_hip_stream_slot_pcm(b->hs, CLIP_SLOT);
    for (int i = 0; i < W->nh; i++) memcpy(W->copies[i].dst, src + W->copies[i].off, W->copies[i].bytes);
  }
  W->n = W->np = W->nh = 0;
  W->stage = 0;
  return ok ? 0 : -1;
}

int pdmp3_amd_bulk_decode_clips(struct bulk* b, const pdmp3_amd_clip* clips, int n_clips, long long* pcm_bytes) {
  if (!b || !b->hs || !b->bits_mode || n_clips < 0 || (n_clips && (!clips || !pcm_bytes))) return -1;
  for (int k = 0; k < n_clips; k++) {
    const pdmp3_amd_clip* c = &clips[k];
    if (!c->index || (!c->mp3 && c->n) || c->n != c->index->n || (!c->dst && c->dst_cap)) return -1;
    if ((c->index->iso & PDMP3_ISO_LSF) != (b->id->iso & PDMP3_ISO_LSF)) return -1;
  }
  if (pdmp3_amd_bulk_wait(b) != 0) return -1;       /* (the slots are the clips' from here on) */
  const int cap = b->cap;
  pdmp3_frame_bits* wbits = pdmp3_hip_stream_slot_bits(b->hs, CLIP_SLOT);
  uint8_t* wres = pdmp3_hip_stream_slot_reservoir(b->hs, CLIP_SLOT);
  uint8_t* stage = (uint8_t*)pdmp3_hip_stream_slot_clip_stage(b->hs, CLIP_SLOT);
  clip_win W;
  memset(&W, 0, sizeof W);
  W.pieces = (pdmp3_clip_piece*)malloc((size_t)cap * sizeof *W.pieces);
  W.copies = (stage_copy*)malloc((size_t)cap * sizeof *W.copies);
  struct bulk* sb = (struct bulk*)calloc(1, sizeof *sb);          /* the scan's sink: bits + snapshot rows into `sbits` / `sres` */
  if (sb) sb->id = (pdmp3_handle*)calloc(1, sizeof *sb->id);
  pdmp3_frame_bits* sbits = NULL;
  uint8_t* sres = NULL;
  long long scap = 0;
  int rc = 0;
  if (!wbits || !wres || !stage || !W.pieces || !W.copies || !sb || !sb->id) { rc = -1; goto out; }
  sb->bits_mode = 1;
  sb->id->iso = b->id->iso;
  sb->id->side_to_bits = !getenv("PDMP3_BULK_SLOW_SIDE_INFO");
  sb->id->bits_scan = 1;
  sb->id->bits_lsf = b->bits_lsf;
  for (int k = 0; k < n_clips; k++) {
    const pdmp3_amd_clip* c = &clips[k];
    const pdmp3_amd_index* ix = c->index;
    if (ix->frames < 0) { pcm_bytes[k] = ix->frames; rc = PDMP3_BULK_REPLAY; continue; }
    long long a, e;
    clamp_range(ix, c->first_frame, c->n_frames, &a, &e);
    pcm_bytes[k] = ix->off[e] - ix->off[a];
    if (a == e) continue;
    const long long f0 = ix_first(ix, a, e, 1), need = e - f0;
    if (need > scap) {
      free(sbits); free(sres);
      scap = need;
      sbits = (pdmp3_frame_bits*)malloc((size_t)scap * sizeof *sbits);
      sres = (uint8_t*)malloc((size_t)scap * RESERVOIR_BYTES);
      if (!sbits || !sres) { scap = 0; rc = -1; goto out; }
    }
    sb->rec_bits = sbits; sb->rec_res = sres; sb->rec_cap = (size_t)need;
    if (ix_scan(ix, c->mp3, c->n, f0, need, sb) != need) { rc = -1; goto out; }
    b->clip_frames += e - a;
    b->clip_halo += a - f0;
    const int to_device = c->dst_cap && pdmp3_hip_host_is_pinned(c->dst, c->dst_cap) == 2;
    for (long long i = 0; i < need; i++) {
      const long long f = f0 + i;
      const pdmp3_frame_bits* fb = &sbits[i];
      const int mono = ((fb->frame & PDMP3_FR_MODE_MASK) >> PDMP3_FR_MODE_SHIFT) == 3;
      const int kind = fb->lsf ? (fb->lsf << 1) | mono : 0;
      if (W.n && (kind != W.kind || W.n == cap) && clip_flush(b, &W) != 0) { rc = -1; goto out; }
      if (!W.n) W.kind = kind;
      wbits[W.n] = *fb;
      memcpy(wres + (size_t)W.n * RESERVOIR_BYTES, sres + (size_t)i * RESERVOIR_BYTES, RESERVOIR_BYTES);
      const long long rel = ix->off[f] - ix->off[a];
      if (f >= a && (size_t)rel < c->dst_cap) {         /* a kept frame with room in its destination */
        const size_t size = (size_t)(ix->off[f + 1] - ix->off[f]);
        const size_t bytes = size < c->dst_cap - (size_t)rel ? size : c->dst_cap - (size_t)rel;
        pdmp3_clip_piece* p = &W.pieces[W.np++];
        p->src = clip_src(kind, W.n);
        p->bytes = (uint32_t)bytes;
        unsigned char* to = (unsigned char*)c->dst + rel;
        if (to_device) p->dst = (uint64_t)(uintptr_t)to;
        else {
          p->dst = (uint64_t)(uintptr_t)(stage + W.stage);
          W.copies[W.nh].dst = to; W.copies[W.nh].off = W.stage; W.copies[W.nh].bytes = bytes;
          W.nh++;
          W.stage += bytes;
        }
      }
      W.n++;
    }
  }
  if (clip_flush(b, &W) != 0) rc = -1;
out:
  if (rc == -1) (void)pdmp3_hip_stream_wait(b->hs, CLIP_SLOT);
  free(sbits); free(sres);
  if (sb) free(sb->id);
  free(sb);
  free(W.pieces); free(W.copies);
  return rc;
}

void pdmp3_amd_bulk_clip_stats(const struct bulk* b, long long* clip_frames, long long* halo_frames) {
  if (clip_frames) *clip_frames = b ? b->clip_frames : 0;
  if (halo_frames) *halo_frames = b ? b->clip_halo : 0;
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
  /* host destinations: rows that lie one behind the other in the caller's memory as they do in the stage leave in one copy */
  for (int i = 0; i < nd; i++) {
    if (host[i] < 0) continue;
    const pdmp3_amd_audio_clip* c = &clips[host[i]];
    const float* from = (const float*)(uintptr_t)ds[i].dst;
    if (C == 2 && c->chan_stride != (size_t)T) {
      if (pdmp3_hip_copy_from_device(c->dst, from, (size_t)T * sizeof(float)) != PDMP3_HIP_OK ||
          pdmp3_hip_copy_from_device(c->dst + c->chan_stride, from + T, (size_t)T * sizeof(float)) != PDMP3_HIP_OK) { rc = -1; goto out; }
      continue;
    }
    size_t floats = (size_t)C * (size_t)T;
    int j = i + 1;
    for (; j < nd && host[j] >= 0; j++) {
      const pdmp3_amd_audio_clip* n = &clips[host[j]];
      if (n->dst != c->dst + floats || (C == 2 && n->chan_stride != (size_t)T)) break;
      floats += (size_t)C * (size_t)T;
    }
    if (pdmp3_hip_copy_from_device(c->dst, from, floats * sizeof(float)) != PDMP3_HIP_OK) { rc = -1; goto out; }
    i = j - 1;
  }
out:
  free(pc); free(pb); free(ds); free(host); free((void*)tabs); free(ft); free(coef);
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
  if (!b || !b->hs || !b->bits_mode || !spec || n_clips < 0 || (n_clips && (!clips || !valid)) || spec->n_frames < 0) return -1;
  const long long F = spec->n_frames;
  int C = spec->channels, rc = 0;
  long sr = spec->rate;
  if (C < 0 || C > 2 || sr < 0) return -1;
  for (int k = 0; k < n_clips; k++) {
    const pdmp3_amd_audio_clip* c = &clips[k];
    if (!c->index || (!c->mp3 && c->n) || c->n != c->index->n || c->start < 0 || (F && !c->dst)) return -1;
    if ((c->index->iso & PDMP3_ISO_LSF) != (b->id->iso & PDMP3_ISO_LSF)) return -1;
    if (c->index->frames < 0 || c->index->mixed) continue;
    const int cs = c->index->stereo ? 2 : 1;
    if (!spec->channels) {
      if (C && C != cs) return -1;                   /* (no channel count asked for, and the clips' differ) */
      C = cs;
    }
    if (!spec->rate && c->index->frames) {
      if (sr && sr != c->index->rate) return -1;     /* (no rate asked for, and the clips' differ: one filterbank a call) */
      sr = c->index->rate;
    }
  }
  if (!C) C = 1;
  if (!sr) sr = 44100;                               /* (no clip to decode, or only streams without frames) */
  if (pdmp3_amd_mel_check(spec, sr) != 0) return -1;
  const int N = spec->n_fft, H = spec->hop;
  pdmp3_mel_params P;
  memset(&P, 0, sizeof P);
  if (mel_plan(N, H, spec->n_mels, &P) != 0) return -1;
  if (F > 0x7fffffffLL / (spec->n_mels > H ? spec->n_mels : H) - 2 * N) return -1;          /* (a row's samples and floats stay inside 31 bits) */
  const size_t per = (size_t)spec->n_mels * (size_t)F;                /* floats of a channel's output */
  for (int k = 0; k < n_clips; k++) if (C == 2 && F && clips[k].chan_stride < per) return -1;
  const long long T = F ? (F - 1) * H + N : 0;                        /* samples of a row: what F frames read */
  const size_t Ts = ((size_t)T + 3) & ~(size_t)3;
  pdmp3_amd_audio_clip* ac = (pdmp3_amd_audio_clip*)calloc((size_t)n_clips + 1, sizeof *ac);
  long long* av = (long long*)calloc((size_t)n_clips + 1, sizeof *av);
  pdmp3_mel_desc* ds = (pdmp3_mel_desc*)calloc((size_t)n_clips + 1, sizeof *ds);
  int* host = (int*)calloc((size_t)n_clips + 1, sizeof *host);       /* per descriptor: its clip, if that one's rows go to host memory, else -1 */
  int nd = 0;
  size_t out_floats = 0;
  if (!ac || !av || !ds || !host) { rc = -1; goto out; }
  for (int k = 0; k < n_clips; k++) {
    const pdmp3_amd_audio_clip* c = &clips[k];
    const pdmp3_amd_index* ix = c->index;
    if (ix->frames < 0) { valid[k] = PDMP3_BULK_REPLAY; rc = PDMP3_BULK_REPLAY; continue; }
    if (ix->mixed) { valid[k] = PDMP3_BULK_MIXED_FORMAT; if (rc != PDMP3_BULK_REPLAY) rc = PDMP3_BULK_MIXED_FORMAT; continue; }
    audio_plan p;
    if (audio_plan_init(&p, ix->frames ? ix->rate : sr, sr, spec->width, spec->rolloff) != 0) { rc = -1; goto out; }
    const long long Nin = ix->frames * (ix->frames ? ix->spf : 0);
    const long long J = (long long)(((__int128)Nin * p.L + p.M - 1) / p.M);
    const long long left = J - c->start;
    valid[k] = left <= 0 ? 0 : (left + H - 1) / H < F ? (left + H - 1) / H : F;
    if (!F) continue;
    /* the row: the span from max(0, start - N / 2) on, `lead` zeros in front of it */
    const long long s0 = c->start > N / 2 ? c->start - N / 2 : 0;
    ac[nd].mp3 = c->mp3; ac[nd].n = c->n; ac[nd].index = ix;
    ac[nd].start = s0;
    ac[nd].chan_stride = Ts;
    ds[nd].lead = (uint32_t)(s0 - (c->start - N / 2));
    ds[nd].src_chan_stride = Ts;
    const size_t row_bytes = ((size_t)(C - 1) * c->chan_stride + per) * sizeof(float);
    if (pdmp3_hip_host_is_pinned(c->dst, row_bytes) == 2) { host[nd] = -1; ds[nd].dst = (uint64_t)(uintptr_t)c->dst; ds[nd].dst_chan_stride = c->chan_stride; }
    else { host[nd] = k; ds[nd].dst = out_floats; ds[nd].dst_chan_stride = per; out_floats += (size_t)C * per; }
    nd++;
  }
  if (!nd) goto out;
  const mel_tab* dft = mel_table(b, 0, sr, spec);
  const mel_tab* fbt = mel_table(b, 1, sr, spec);
  if (!dft || !fbt) { rc = -1; goto out; }
  if (pdmp3_amd_bulk_wait(b) != 0) { rc = -1; goto out; }
  float* sig = (float*)pdmp3_hip_stream_audio_stage(b->hs, 2, (size_t)nd * (size_t)C * Ts * sizeof(float));
  if (!sig) { rc = -1; goto out; }
  for (int i = 0; i < nd; i++) {
    ac[i].dst = sig + (size_t)i * (size_t)C * Ts;
    ds[i].src = (uint64_t)(uintptr_t)ac[i].dst;
  }
  /* the rows through the audio call as it is (device destinations: k_clip_audio writes them itself) */
  {
    pdmp3_amd_audio_spec as;
    memset(&as, 0, sizeof as);
    as.rate = sr; as.channels = C; as.n_samples = T; as.width = spec->width; as.rolloff = spec->rolloff;
    if (pdmp3_amd_bulk_decode_clips_audio(b, ac, nd, &as, av) != 0) { rc = -1; goto out; }
  }
  /* (the audio call may have grown stage 1 for nothing of ours: it is free for the rows of host destinations) */
  float* out_stage = out_floats ? (float*)pdmp3_hip_stream_audio_stage(b->hs, 1, out_floats * sizeof(float)) : NULL;
  if (out_floats && !out_stage) { rc = -1; goto out; }
  for (int i = 0; i < nd; i++) if (host[i] >= 0) ds[i].dst = (uint64_t)(uintptr_t)(out_stage + ds[i].dst);
  P.n_in = T; P.n_frames = (int32_t)F; P.channels = C; P.out_mode = spec->out_mode; P.floor = (float)spec->floor;
  if (pdmp3_hip_clip_mel(b->hs, CLIP_SLOT, ds, nd, dft->t, fbt->t, &P) != PDMP3_HIP_OK) {
    fprintf(stderr, "pdmp3: engine failure: %s\n", pdmp3_hip_last_error());
    rc = -1; goto out;
  }
  /* host destinations: rows that lie one behind the other in the caller's memory as they do in the stage leave in one copy */
  for (int i = 0; i < nd; i++) {
    if (host[i] < 0) continue;
    const pdmp3_amd_audio_clip* c = &clips[host[i]];
    const float* from = (const float*)(uintptr_t)ds[i].dst;
    if (C == 2 && c->chan_stride != per) {
      if (pdmp3_hip_copy_from_device(c->dst, from, per * sizeof(float)) != PDMP3_HIP_OK ||
          pdmp3_hip_copy_from_device(c->dst + c->chan_stride, from + per, per * sizeof(float)) != PDMP3_HIP_OK) { rc = -1; goto out; }
      continue;
    }
    size_t floats = (size_t)C * per;
    int j = i + 1;
    for (; j < nd && host[j] >= 0; j++) {
      const pdmp3_amd_audio_clip* n = &clips[host[j]];
      if (n->dst != c->dst + floats || (C == 2 && n->chan_stride != per)) break;
      floats += (size_t)C * per;
    }
    if (pdmp3_hip_copy_from_device(c->dst, from, floats * sizeof(float)) != PDMP3_HIP_OK) { rc = -1; goto out; }
    i = j - 1;
  }
out:
  free(ac); free(av); free(ds); free(host);
  return rc;
}

/* ---- the short-time Fourier transform of clips ---- */
/* The log-mel call's course with another plan, table and launch: the rows through the audio call into stage 2, k_clip_stft
 * behind it, host destinations through stage 1. */
int pdmp3_amd_bulk_decode_clips_stft(struct bulk* b, const pdmp3_amd_audio_clip* clips, int n_clips, const pdmp3_amd_stft_spec* spec,
                                     long long* valid) {
  if (!b || !b->hs || !b->bits_mode || !spec || n_clips < 0 || (n_clips && (!clips || !valid)) || spec->n_frames < 0) return -1;
  const long long F = spec->n_frames;
  int C = spec->channels, rc = 0;
  long sr = spec->rate;
  if (C < 0 || C > 2 || sr < 0) return -1;
  for (int k = 0; k < n_clips; k++) {
    const pdmp3_amd_audio_clip* c = &clips[k];
    if (!c->index || (!c->mp3 && c->n) || c->n != c->index->n || c->start < 0 || (F && !c->dst)) return -1;
    if ((c->index->iso & PDMP3_ISO_LSF) != (b->id->iso & PDMP3_ISO_LSF)) return -1;
    if (c->index->frames < 0 || c->index->mixed) continue;
    const int cs = c->index->stereo ? 2 : 1;
    if (!spec->channels) {
      if (C && C != cs) return -1;                   /* (no channel count asked for, and the clips' differ) */
      C = cs;
    }
    if (!spec->rate && c->index->frames) {
      if (sr && sr != c->index->rate) return -1;     /* (no rate asked for, and the clips' differ: one time line a call) */
      sr = c->index->rate;
    }
  }
  if (!C) C = 1;
  if (!sr) sr = 44100;                               /* (no clip to decode, or only streams without frames) */
  if (pdmp3_amd_stft_check(spec, sr) != 0) return -1;
  const int N = spec->n_fft, H = spec->hop;
  pdmp3_stft_params P;
  memset(&P, 0, sizeof P);
  if (stft_plan(N, H, spec->out_mode, &P) != 0) return -1;
  const int per_frame = P.bins * (spec->out_mode == 0 ? 2 : 1);       /* floats of a frame */
  if (F > 0x7fffffffLL / (per_frame > H ? per_frame : H) - 2 * N) return -1;                /* (a row's samples and floats stay inside 31 bits) */
  const size_t per = (size_t)per_frame * (size_t)F;                   /* floats of a channel's output */
  for (int k = 0; k < n_clips; k++) if (C == 2 && F && clips[k].chan_stride < per) return -1;
  const long long T = F ? (F - 1) * H + N : 0;                        /* samples of a row: what F frames read */
  const size_t Ts = ((size_t)T + 3) & ~(size_t)3;
  pdmp3_amd_audio_clip* ac = (pdmp3_amd_audio_clip*)calloc((size_t)n_clips + 1, sizeof *ac);
  long long* av = (long long*)calloc((size_t)n_clips + 1, sizeof *av);
  pdmp3_mel_desc* ds = (pdmp3_mel_desc*)calloc((size_t)n_clips + 1, sizeof *ds);
  int* host = (int*)calloc((size_t)n_clips + 1, sizeof *host);       /* per descriptor: its clip, if that one's rows go to host memory, else -1 */
  int nd = 0;
  size_t out_floats = 0;
  if (!ac || !av || !ds || !host) { rc = -1; goto out; }
  for (int k = 0; k < n_clips; k++) {
    const pdmp3_amd_audio_clip* c = &clips[k];
    const pdmp3_amd_index* ix = c->index;
    if (ix->frames < 0) { valid[k] = PDMP3_BULK_REPLAY; rc = PDMP3_BULK_REPLAY; continue; }
    if (ix->mixed) { valid[k] = PDMP3_BULK_MIXED_FORMAT; if (rc != PDMP3_BULK_REPLAY) rc = PDMP3_BULK_MIXED_FORMAT; continue; }
    audio_plan p;
    if (audio_plan_init(&p, ix->frames ? ix->rate : sr, sr, spec->width, spec->rolloff) != 0) { rc = -1; goto out; }
    const long long Nin = ix->frames * (ix->frames ? ix->spf : 0);
    const long long J = (long long)(((__int128)Nin * p.L + p.M - 1) / p.M);
    const long long left = J - c->start;
    valid[k] = left <= 0 ? 0 : (left + H - 1) / H < F ? (left + H - 1) / H : F;
    if (!F) continue;
    /* the row: the span from max(0, start - N / 2) on, `lead` zeros in front of it */
    const long long s0 = c->start > N / 2 ? c->start - N / 2 : 0;
    ac[nd].mp3 = c->mp3; ac[nd].n = c->n; ac[nd].index = ix;
    ac[nd].start = s0;
    ac[nd].chan_stride = Ts;
    ds[nd].lead = (uint32_t)(s0 - (c->start - N / 2));
    ds[nd].src_chan_stride = Ts;
    const size_t row_bytes = ((size_t)(C - 1) * c->chan_stride + per) * sizeof(float);
    if (pdmp3_hip_host_is_pinned(c->dst, row_bytes) == 2) { host[nd] = -1; ds[nd].dst = (uint64_t)(uintptr_t)c->dst; ds[nd].dst_chan_stride = c->chan_stride; }
    else { host[nd] = k; ds[nd].dst = out_floats; ds[nd].dst_chan_stride = per; out_floats += (size_t)C * per; }
    nd++;
  }
  if (!nd) goto out;
  const float* table = stft_table(b, spec);
  if (!table) { rc = -1; goto out; }
  if (pdmp3_amd_bulk_wait(b) != 0) { rc = -1; goto out; }
  float* sig = (float*)pdmp3_hip_stream_audio_stage(b->hs, 2, (size_t)nd * (size_t)C * Ts * sizeof(float));
  if (!sig) { rc = -1; goto out; }
  for (int i = 0; i < nd; i++) {
    ac[i].dst = sig + (size_t)i * (size_t)C * Ts;
    ds[i].src = (uint64_t)(uintptr_t)ac[i].dst;
  }
  /* the rows through the audio call as it is (device destinations: k_clip_audio writes them itself) */
  {
    pdmp3_amd_audio_spec as;
    memset(&as, 0, sizeof as);
    as.rate = sr; as.channels = C; as.n_samples = T; as.width = spec->width; as.rolloff = spec->rolloff;
    if (pdmp3_amd_bulk_decode_clips_audio(b, ac, nd, &as, av) != 0) { rc = -1; goto out; }
  }
  /* (the audio call may have grown stage 1 for nothing of ours: it is free for the rows of host destinations) */
  float* out_stage = out_floats ? (float*)pdmp3_hip_stream_audio_stage(b->hs, 1, out_floats * sizeof(float)) : NULL;
  if (out_floats && !out_stage) { rc = -1; goto out; }
  for (int i = 0; i < nd; i++) if (host[i] >= 0) ds[i].dst = (uint64_t)(uintptr_t)(out_stage + ds[i].dst);
  P.n_in = T; P.n_frames = (int32_t)F; P.channels = C; P.floor = spec->out_mode >= 3 ? (float)spec->floor : 0.0f;
  if (pdmp3_hip_clip_stft(b->hs, CLIP_SLOT, ds, nd, table, &P) != PDMP3_HIP_OK) {
    fprintf(stderr, "pdmp3: engine failure: %s\n", pdmp3_hip_last_error());
    rc = -1; goto out;
  }
  /* host destinations: rows that lie one behind the other in the caller's memory as they do in the stage leave in one copy */
  for (int i = 0; i < nd; i++) {
    if (host[i] < 0) continue;
    const pdmp3_amd_audio_clip* c = &clips[host[i]];
    const float* from = (const float*)(uintptr_t)ds[i].dst;
    if (C == 2 && c->chan_stride != per) {
      if (pdmp3_hip_copy_from_device(c->dst, from, per * sizeof(float)) != PDMP3_HIP_OK ||
          pdmp3_hip_copy_from_device(c->dst + c->chan_stride, from + per, per * sizeof(float)) != PDMP3_HIP_OK) { rc = -1; goto out; }
      continue;
    }
    size_t floats = (size_t)C * per;
    int j = i + 1;
    for (; j < nd && host[j] >= 0; j++) {
      const pdmp3_amd_audio_clip* n = &clips[host[j]];
      if (n->dst != c->dst + floats || (C == 2 && n->chan_stride != per)) break;
      floats += (size_t)C * per;
    }
    if (pdmp3_hip_copy_from_device(c->dst, from, floats * sizeof(float)) != PDMP3_HIP_OK) { rc = -1; goto out; }
    i = j - 1;
  }
out:
  free(ac); free(av); free(ds); free(host);
  return rc;
}

/* ---- the short-time Fourier transform of clips at n_fft 2048 and 4096 ---- */
/* The call above with another check, plan, block of tables and launch: the rows through the audio call into stage 2,
 * k_clip_stft_long behind it, host destinations through stage 1. */
int pdmp3_amd_bulk_decode_clips_stft_long(struct bulk* b, const pdmp3_amd_audio_clip* clips, int n_clips, const pdmp3_amd_stft_spec* spec,
                                          long long* valid) {
  if (!b || !b->hs || !b->bits_mode || !spec || n_clips < 0 || (n_clips && (!clips || !valid)) || spec->n_frames < 0) return -1;
  const long long F = spec->n_frames;
  int C = spec->channels, rc = 0;
  long sr = spec->rate;
  if (C < 0 || C > 2 || sr < 0) return -1;
  for (int k = 0; k < n_clips; k++) {
    const pdmp3_amd_audio_clip* c = &clips[k];
    if (!c->index || (!c->mp3 && c->n) || c->n != c->index->n || c->start < 0 || (F && !c->dst)) return -1;
    if ((c->index->iso & PDMP3_ISO_LSF) != (b->id->iso & PDMP3_ISO_LSF)) return -1;
    if (c->index->frames < 0 || c->index->mixed) continue;
    const int cs = c->index->stereo ? 2 : 1;
    if (!spec->channels) {
      if (C && C != cs) return -1;                   /* (no channel count asked for, and the clips' differ) */
      C = cs;
    }
    if (!spec->rate && c->index->frames) {
      if (sr && sr != c->index->rate) return -1;     /* (no rate asked for, and the clips' differ: one time line a call) */
      sr = c->index->rate;
    }
  }
  if (!C) C = 1;
  if (!sr) sr = 44100;                               /* (no clip to decode, or only streams without frames) */
  if (pdmp3_amd_stft_long_check(spec, sr) != 0) return -1;
  const int N = spec->n_fft, H = spec->hop;
  pdmp3_stft_long_params P;
  memset(&P, 0, sizeof P);
  if (stft_long_plan(N, H, spec->out_mode, &P) != 0) return -1;
  const int per_frame = P.bins * (spec->out_mode == 0 ? 2 : 1);       /* floats of a frame */
  if (F > 0x7fffffffLL / (per_frame > H ? per_frame : H) - 2 * N) return -1;                /* (a row's samples and floats stay inside 31 bits) */
  const size_t per = (size_t)per_frame * (size_t)F;                   /* floats of a channel's output */
  for (int k = 0; k < n_clips; k++) if (C == 2 && F && clips[k].chan_stride < per) return -1;
  const long long T = F ? (F - 1) * H + N : 0;                        /* samples of a row: what F frames read */
  const size_t Ts = ((size_t)T + 3) & ~(size_t)3;
  pdmp3_amd_audio_clip* ac = (pdmp3_amd_audio_clip*)calloc((size_t)n_clips + 1, sizeof *ac);
  long long* av = (long long*)calloc((size_t)n_clips + 1, sizeof *av);
  pdmp3_mel_desc* ds = (pdmp3_mel_desc*)calloc((size_t)n_clips + 1, sizeof *ds);
  int* host = (int*)calloc((size_t)n_clips + 1, sizeof *host);       /* per descriptor: its clip, if that one's rows go to host memory, else -1 */
  int nd = 0;
  size_t out_floats = 0;
  if (!ac || !av || !ds || !host) { rc = -1; goto out; }
  for (int k = 0; k < n_clips; k++) {
    const pdmp3_amd_audio_clip* c = &clips[k];
    const pdmp3_amd_index* ix = c->index;
    if (ix->frames < 0) { valid[k] = PDMP3_BULK_REPLAY; rc = PDMP3_BULK_REPLAY; continue; }
    if (ix->mixed) { valid[k] = PDMP3_BULK_MIXED_FORMAT; if (rc != PDMP3_BULK_REPLAY) rc = PDMP3_BULK_MIXED_FORMAT; continue; }
    audio_plan p;
    if (audio_plan_init(&p, ix->frames ? ix->rate : sr, sr, spec->width, spec->rolloff) != 0) { rc = -1; goto out; }
    const long long Nin = ix->frames * (ix->frames ? ix->spf : 0);
    const long long J = (long long)(((__int128)Nin * p.L + p.M - 1) / p.M);
    const long long left = J - c->start;
    valid[k] = left <= 0 ? 0 : (left + H - 1) / H < F ? (left + H - 1) / H : F;
    if (!F) continue;
    /* the row: the span from max(0, start - N / 2) on, `lead` zeros in front of it */
    const long long s0 = c->start > N / 2 ? c->start - N / 2 : 0;
    ac[nd].mp3 = c->mp3; ac[nd].n = c->n; ac[nd].index = ix;
    ac[nd].start = s0;
    ac[nd].chan_stride = Ts;
    ds[nd].lead = (uint32_t)(s0 - (c->start - N / 2));
    ds[nd].src_chan_stride = Ts;
    const size_t row_bytes = ((size_t)(C - 1) * c->chan_stride + per) * sizeof(float);
    if (pdmp3_hip_host_is_pinned(c->dst, row_bytes) == 2) { host[nd] = -1; ds[nd].dst = (uint64_t)(uintptr_t)c->dst; ds[nd].dst_chan_stride = c->chan_stride; }
    else { host[nd] = k; ds[nd].dst = out_floats; ds[nd].dst_chan_stride = per; out_floats += (size_t)C * per; }
    nd++;
  }
  if (!nd) goto out;
  const float* table = stft_long_tables(b, spec);
  if (!table) { rc = -1; goto out; }
  if (pdmp3_amd_bulk_wait(b) != 0) { rc = -1; goto out; }
  float* sig = (float*)pdmp3_hip_stream_audio_stage(b->hs, 2, (size_t)nd * (size_t)C * Ts * sizeof(float));
  if (!sig) { rc = -1; goto out; }
  for (int i = 0; i < nd; i++) {
    ac[i].dst = sig + (size_t)i * (size_t)C * Ts;
    ds[i].src = (uint64_t)(uintptr_t)ac[i].dst;
  }
  /* the rows through the audio call as it is (device destinations: k_clip_audio writes them itself) */
  {
    pdmp3_amd_audio_spec as;
    memset(&as, 0, sizeof as);
    as.rate = sr; as.channels = C; as.n_samples = T; as.width = spec->width; as.rolloff = spec->rolloff;
    if (pdmp3_amd_bulk_decode_clips_audio(b, ac, nd, &as, av) != 0) { rc = -1; goto out; }
  }
  /* (the audio call may have grown stage 1 for nothing of ours: it is free for the rows of host destinations) */
  float* out_stage = out_floats ? (float*)pdmp3_hip_stream_audio_stage(b->hs, 1, out_floats * sizeof(float)) : NULL;
  if (out_floats && !out_stage) { rc = -1; goto out; }
  for (int i = 0; i < nd; i++) if (host[i] >= 0) ds[i].dst = (uint64_t)(uintptr_t)(out_stage + ds[i].dst);
  P.n_in = T; P.n_frames = (int32_t)F; P.channels = C; P.floor = spec->out_mode >= 3 ? (float)spec->floor : 0.0f;
  if (pdmp3_hip_clip_stft_long(b->hs, CLIP_SLOT, ds, nd, table, &P) != PDMP3_HIP_OK) {
    fprintf(stderr, "pdmp3: engine failure: %s\n", pdmp3_hip_last_error());
    rc = -1; goto out;
  }
  /* host destinations: rows that lie one behind the other in the caller's memory as they do in the stage leave in one copy */
  for (int i = 0; i < nd; i++) {
    if (host[i] < 0) continue;
    const pdmp3_amd_audio_clip* c = &clips[host[i]];
    const float* from = (const float*)(uintptr_t)ds[i].dst;
    if (C == 2 && c->chan_stride != per) {
      if (pdmp3_hip_copy_from_device(c->dst, from, per * sizeof(float)) != PDMP3_HIP_OK ||
          pdmp3_hip_copy_from_device(c->dst + c->chan_stride, from + per, per * sizeof(float)) != PDMP3_HIP_OK) { rc = -1; goto out; }
      continue;
    }
    size_t floats = (size_t)C * per;
    int j = i + 1;
    for (; j < nd && host[j] >= 0; j++) {
      const pdmp3_amd_audio_clip* n = &clips[host[j]];
      if (n->dst != c->dst + floats || (C == 2 && n->chan_stride != per)) break;
      floats += (size_t)C * per;
    }
    if (pdmp3_hip_copy_from_device(c->dst, from, floats * sizeof(float)) != PDMP3_HIP_OK) { rc = -1; goto out; }
    i = j - 1;
  }
out:
  free(ac); free(av); free(ds); free(host);
  return rc;
}

/* ---- log-mel features of clips at n_fft 2048 and 4096 ---- */
/* The call above with another spec, check and plan, its block of tables with the filterbank operand behind it, and another
 * launch: the rows through the audio call into stage 2, k_clip_mel_long behind it, host destinations through stage 1. */
int pdmp3_amd_bulk_decode_clips_mel_long(struct bulk* b, const pdmp3_amd_audio_clip* clips, int n_clips, const pdmp3_amd_mel_long_spec* spec,
                                         long long* valid) {
  if (!b || !b->hs || !b->bits_mode || !spec || n_clips < 0 || (n_clips && (!clips || !valid)) || spec->mel.n_frames < 0) return -1;
  const long long F = spec->mel.n_frames;
  int C = spec->mel.channels, rc = 0;
  long sr = spec->mel.rate;
  if (C < 0 || C > 2 || sr < 0) return -1;
  for (int k = 0; k < n_clips; k++) {
    const pdmp3_amd_audio_clip* c = &clips[k];
    if (!c->index || (!c->mp3 && c->n) || c->n != c->index->n || c->start < 0 || (F && !c->dst)) return -1;
    if ((c->index->iso & PDMP3_ISO_LSF) != (b->id->iso & PDMP3_ISO_LSF)) return -1;
    if (c->index->frames < 0 || c->index->mixed) continue;
    const int cs = c->index->stereo ? 2 : 1;
    if (!spec->mel.channels) {
      if (C && C != cs) return -1;                   /* (no channel count asked for, and the clips' differ) */
      C = cs;
    }
    if (!spec->mel.rate && c->index->frames) {
      if (sr && sr != c->index->rate) return -1;     /* (no rate asked for, and the clips' differ: one time line a call) */
      sr = c->index->rate;
    }
  }
  if (!C) C = 1;
  if (!sr) sr = 44100;                               /* (no clip to decode, or only streams without frames) */
  if (pdmp3_amd_mel_long_check(spec, sr) != 0) return -1;
  const int N = spec->mel.n_fft, H = spec->mel.hop;
  pdmp3_mel_long_params P;
  memset(&P, 0, sizeof P);
  if (mel_long_plan(N, H, spec->mel.n_mels, &P) != 0) return -1;
  const int per_frame = spec->mel.n_mels;                             /* floats of a frame */
  if (F > 0x7fffffffLL / (per_frame > H ? per_frame : H) - 2 * N) return -1;                /* (a row's samples and floats stay inside 31 bits) */
  const size_t per = (size_t)per_frame * (size_t)F;                   /* floats of a channel's output */
  for (int k = 0; k < n_clips; k++) if (C == 2 && F && clips[k].chan_stride < per) return -1;
  const long long T = F ? (F - 1) * H + N : 0;                        /* samples of a row: what F frames read */
  const size_t Ts = ((size_t)T + 3) & ~(size_t)3;
  pdmp3_amd_audio_clip* ac = (pdmp3_amd_audio_clip*)calloc((size_t)n_clips + 1, sizeof *ac);
  long long* av = (long long*)calloc((size_t)n_clips + 1, sizeof *av);
  pdmp3_mel_desc* ds = (pdmp3_mel_desc*)calloc((size_t)n_clips + 1, sizeof *ds);
  int* host = (int*)calloc((size_t)n_clips + 1, sizeof *host);       /* per descriptor: its clip, if that one's rows go to host memory, else -1 */
  int nd = 0;
  size_t out_floats = 0;
  if (!ac || !av || !ds || !host) { rc = -1; goto out; }
  for (int k = 0; k < n_clips; k++) {
    const pdmp3_amd_audio_clip* c = &clips[k];
    const pdmp3_amd_index* ix = c->index;
    if (ix->frames < 0) { valid[k] = PDMP3_BULK_REPLAY; rc = PDMP3_BULK_REPLAY; continue; }
    if (ix->mixed) { valid[k] = PDMP3_BULK_MIXED_FORMAT; if (rc != PDMP3_BULK_REPLAY) rc = PDMP3_BULK_MIXED_FORMAT; continue; }
    audio_plan p;
    if (audio_plan_init(&p, ix->frames ? ix->rate : sr, sr, spec->mel.width, spec->mel.rolloff) != 0) { rc = -1; goto out; }
    const long long Nin = ix->frames * (ix->frames ? ix->spf : 0);
    const long long J = (long long)(((__int128)Nin * p.L + p.M - 1) / p.M);
    const long long left = J - c->start;
    valid[k] = left <= 0 ? 0 : (left + H - 1) / H < F ? (left + H - 1) / H : F;
    if (!F) continue;
    /* the row: the span from max(0, start - N / 2) on, `lead` zeros in front of it */
    const long long s0 = c->start > N / 2 ? c->start - N / 2 : 0;
    ac[nd].mp3 = c->mp3; ac[nd].n = c->n; ac[nd].index = ix;
    ac[nd].start = s0;
    ac[nd].chan_stride = Ts;
    ds[nd].lead = (uint32_t)(s0 - (c->start - N / 2));
    ds[nd].src_chan_stride = Ts;
    const size_t row_bytes = ((size_t)(C - 1) * c->chan_stride + per) * sizeof(float);
    if (pdmp3_hip_host_is_pinned(c->dst, row_bytes) == 2) { host[nd] = -1; ds[nd].dst = (uint64_t)(uintptr_t)c->dst; ds[nd].dst_chan_stride = c->chan_stride; }
    else { host[nd] = k; ds[nd].dst = out_floats; ds[nd].dst_chan_stride = per; out_floats += (size_t)C * per; }
    nd++;
  }
  if (!nd) goto out;
  pdmp3_amd_stft_spec frame;
  mel_long_stft_spec(spec, &frame);
  const float* table = stft_long_tables(b, &frame);
  const float* operand = mel_long_operand(b, sr, &spec->mel);
  if (!table || !operand) { rc = -1; goto out; }
  if (pdmp3_amd_bulk_wait(b) != 0) { rc = -1; goto out; }
  float* sig = (float*)pdmp3_hip_stream_audio_stage(b->hs, 2, (size_t)nd * (size_t)C * Ts * sizeof(float));
  if (!sig) { rc = -1; goto out; }
  for (int i = 0; i < nd; i++) {
    ac[i].dst = sig + (size_t)i * (size_t)C * Ts;
    ds[i].src = (uint64_t)(uintptr_t)ac[i].dst;
  }
  /* the rows through the audio call as it is (device destinations: k_clip_audio writes them itself) */
  {
    pdmp3_amd_audio_spec as;
    memset(&as, 0, sizeof as);
    as.rate = sr; as.channels = C; as.n_samples = T; as.width = spec->mel.width; as.rolloff = spec->mel.rolloff;
    if (pdmp3_amd_bulk_decode_clips_audio(b, ac, nd, &as, av) != 0) { rc = -1; goto out; }
  }
  /* (the audio call may have grown stage 1 for nothing of ours: it is free for the rows of host destinations) */
  float* out_stage = out_floats ? (float*)pdmp3_hip_stream_audio_stage(b->hs, 1, out_floats * sizeof(float)) : NULL;
  if (out_floats && !out_stage) { rc = -1; goto out; }
  for (int i = 0; i < nd; i++) if (host[i] >= 0) ds[i].dst = (uint64_t)(uintptr_t)(out_stage + ds[i].dst);
  P.n_in = T; P.n_frames = (int32_t)F; P.channels = C; P.out_mode = spec->mel.out_mode; P.floor = (float)spec->mel.floor;
  if (pdmp3_hip_clip_mel_long(b->hs, CLIP_SLOT, ds, nd, table, operand, &P) != PDMP3_HIP_OK) {
    fprintf(stderr, "pdmp3: engine failure: %s\n", pdmp3_hip_last_error());
    rc = -1; goto out;
  }
  /* host destinations: rows that lie one behind the other in the caller's memory as they do in the stage leave in one copy */
  for (int i = 0; i < nd; i++) {
    if (host[i] < 0) continue;
    const pdmp3_amd_audio_clip* c = &clips[host[i]];
    const float* from = (const float*)(uintptr_t)ds[i].dst;
    if (C == 2 && c->chan_stride != per) {
      if (pdmp3_hip_copy_from_device(c->dst, from, per * sizeof(float)) != PDMP3_HIP_OK ||
          pdmp3_hip_copy_from_device(c->dst + c->chan_stride, from + per, per * sizeof(float)) != PDMP3_HIP_OK) { rc = -1; goto out; }
      continue;
    }
    size_t floats = (size_t)C * per;
    int j = i + 1;
    for (; j < nd && host[j] >= 0; j++) {
      const pdmp3_amd_audio_clip* n = &clips[host[j]];
      if (n->dst != c->dst + floats || (C == 2 && n->chan_stride != per)) break;
      floats += (size_t)C * per;
    }
    if (pdmp3_hip_copy_from_device(c->dst, from, floats * sizeof(float)) != PDMP3_HIP_OK) { rc = -1; goto out; }
    i = j - 1;
  }
out:
  free(ac); free(av); free(ds); free(host);
  return rc;
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
 * frame, the plan of a workgroup and the launch */
static int kaldi_clips(struct bulk* b, const pdmp3_amd_audio_clip* clips, int n_clips, const pdmp3_amd_fbank_spec* spec,
                       const pdmp3_amd_mfcc_spec* mfcc, long long* valid) {
  if (!b || !b->hs || !b->bits_mode || !spec || n_clips < 0 || (n_clips && (!clips || !valid)) || spec->n_frames < 0) return -1;
  const long long F = spec->n_frames;
  int C = spec->channels, rc = 0;
  long sr = spec->rate;
  if (C < 0 || C > 2 || sr < 0) return -1;
  for (int k = 0; k < n_clips; k++) {
    const pdmp3_amd_audio_clip* c = &clips[k];
    if (!c->index || (!c->mp3 && c->n) || c->n != c->index->n || c->start < 0 || (F && !c->dst)) return -1;
    if ((c->index->iso & PDMP3_ISO_LSF) != (b->id->iso & PDMP3_ISO_LSF)) return -1;
    if (c->index->frames < 0 || c->index->mixed) continue;
    const int cs = c->index->stereo ? 2 : 1;
    if (!spec->channels) {
      if (C && C != cs) return -1;                   /* (no channel count asked for, and the clips' differ) */
      C = cs;
    }
    if (!spec->rate && c->index->frames) {
      if (sr && sr != c->index->rate) return -1;     /* (no rate asked for, and the clips' differ: one filterbank a call) */
      sr = c->index->rate;
    }
  }
  if (!C) C = 1;
  if (!sr) sr = 44100;                               /* (no clip to decode, or only streams without frames) */
  if ((mfcc ? pdmp3_amd_mfcc_check(mfcc, sr) : pdmp3_amd_fbank_check(spec, sr)) != 0) return -1;
  const int Nw = spec->win_length, H = spec->hop, D = mfcc ? mfcc->num_ceps : spec->n_mels + spec->use_energy;
  pdmp3_mfcc_params Q;
  memset(&Q, 0, sizeof Q);
  pdmp3_fbank_params* const P = &Q.fb;
  if ((mfcc ? mfcc_plan(Nw, pdmp3_amd_fbank_dft_length(Nw, spec->round_to_power_of_two), H, spec->n_mels, mfcc->num_ceps, &Q)
            : fbank_plan(Nw, pdmp3_amd_fbank_dft_length(Nw, spec->round_to_power_of_two), H, spec->n_mels, P)) != 0) return -1;
  if (F > 0x7fffffffLL / (D > H ? D : H) - 2 * Nw) return -1;          /* (a row's samples and floats stay inside 31 bits) */
  const size_t per = (size_t)D * (size_t)F;                           /* floats of a channel's output */
  for (int k = 0; k < n_clips; k++) if (C == 2 && F && clips[k].chan_stride < per) return -1;
  const long long T = F ? (F - 1) * H + Nw : 0;                       /* samples of a row: what F frames read, from `start` on */
  const size_t Ts = ((size_t)T + 3) & ~(size_t)3;
  pdmp3_amd_audio_clip* ac = (pdmp3_amd_audio_clip*)calloc((size_t)n_clips + 1, sizeof *ac);
  long long* av = (long long*)calloc((size_t)n_clips + 1, sizeof *av);
  pdmp3_fbank_desc* ds = (pdmp3_fbank_desc*)calloc((size_t)n_clips + 1, sizeof *ds);
  int* host = (int*)calloc((size_t)n_clips + 1, sizeof *host);       /* per descriptor: its clip, if that one's rows go to host memory, else -1 */
  int nd = 0;
  size_t out_floats = 0;
  if (!ac || !av || !ds || !host) { rc = -1; goto out; }
  for (int k = 0; k < n_clips; k++) {
    const pdmp3_amd_audio_clip* c = &clips[k];
    const pdmp3_amd_index* ix = c->index;
    if (ix->frames < 0) { valid[k] = PDMP3_BULK_REPLAY; rc = PDMP3_BULK_REPLAY; continue; }
    if (ix->mixed) { valid[k] = PDMP3_BULK_MIXED_FORMAT; if (rc != PDMP3_BULK_REPLAY) rc = PDMP3_BULK_MIXED_FORMAT; continue; }
    audio_plan p;
    if (audio_plan_init(&p, ix->frames ? ix->rate : sr, sr, spec->width, spec->rolloff) != 0) { rc = -1; goto out; }
    const long long Nin = ix->frames * (ix->frames ? ix->spf : 0);
    const long long J = (long long)(((__int128)Nin * p.L + p.M - 1) / p.M);
    valid[k] = pdmp3_amd_fbank_valid(J, c->start, Nw, H, F);
    if (!F) continue;
    ac[nd].mp3 = c->mp3; ac[nd].n = c->n; ac[nd].index = ix;
    ac[nd].start = c->start;
    ac[nd].chan_stride = Ts;
    ds[nd].valid = (uint32_t)valid[k];
    ds[nd].src_chan_stride = Ts;
    const size_t row_bytes = ((size_t)(C - 1) * c->chan_stride + per) * sizeof(float);
    if (pdmp3_hip_host_is_pinned(c->dst, row_bytes) == 2) { host[nd] = -1; ds[nd].dst = (uint64_t)(uintptr_t)c->dst; ds[nd].dst_chan_stride = c->chan_stride; }
    else { host[nd] = k; ds[nd].dst = out_floats; ds[nd].dst_chan_stride = per; out_floats += (size_t)C * per; }
    nd++;
  }
  if (!nd) goto out;
  const fbank_tab* dft = fbank_table(b, 0, sr, spec);
  const fbank_tab* fbt = fbank_table(b, 1, sr, spec);
  const mfcc_tab* dct = mfcc ? mfcc_table(b, mfcc) : NULL;
  if (!dft || !fbt || (mfcc && !dct)) { rc = -1; goto out; }
  if (pdmp3_amd_bulk_wait(b) != 0) { rc = -1; goto out; }
  float* sig = (float*)pdmp3_hip_stream_audio_stage(b->hs, 2, (size_t)nd * (size_t)C * Ts * sizeof(float));
  if (!sig) { rc = -1; goto out; }
  for (int i = 0; i < nd; i++) {
    ac[i].dst = sig + (size_t)i * (size_t)C * Ts;
    ds[i].src = (uint64_t)(uintptr_t)ac[i].dst;
  }
  /* the rows through the audio call as it is (device destinations: k_clip_audio writes them itself) */
  {
    pdmp3_amd_audio_spec as;
    memset(&as, 0, sizeof as);
    as.rate = sr; as.channels = C; as.n_samples = T; as.width = spec->width; as.rolloff = spec->rolloff;
    if (pdmp3_amd_bulk_decode_clips_audio(b, ac, nd, &as, av) != 0) { rc = -1; goto out; }
  }
  /* (the audio call may have grown stage 1 for nothing of ours: it is free for the rows of host destinations) */
  float* out_stage = out_floats ? (float*)pdmp3_hip_stream_audio_stage(b->hs, 1, out_floats * sizeof(float)) : NULL;
  if (out_floats && !out_stage) { rc = -1; goto out; }
  for (int i = 0; i < nd; i++) if (host[i] >= 0) ds[i].dst = (uint64_t)(uintptr_t)(out_stage + ds[i].dst);
  P->n_in = T; P->n_frames = (int32_t)F; P->channels = C; P->out_mode = spec->out_mode;
  P->use_energy = spec->use_energy; P->htk_compat = spec->htk_compat; P->subtract_mean = spec->subtract_mean; P->remove_dc = spec->remove_dc_offset;
  P->scale = (float)spec->scale; P->eps = 0x1p-23f;
  P->energy_log_floor = spec->energy_floor > 0.0 ? (float)log(spec->energy_floor) : -INFINITY;
  if ((mfcc ? pdmp3_hip_clip_mfcc(b->hs, CLIP_SLOT, ds, nd, dft->t, fbt->t, dct->t, &Q)
            : pdmp3_hip_clip_fbank(b->hs, CLIP_SLOT, ds, nd, dft->t, fbt->t, P)) != PDMP3_HIP_OK) {
    fprintf(stderr, "pdmp3: engine failure: %s\n", pdmp3_hip_last_error());
    rc = -1; goto out;
  }
  /* host destinations: rows that lie one behind the other in the caller's memory as they do in the stage leave in one copy */
  for (int i = 0; i < nd; i++) {
    if (host[i] < 0) continue;
    const pdmp3_amd_audio_clip* c = &clips[host[i]];
    const float* from = (const float*)(uintptr_t)ds[i].dst;
    if (C == 2 && c->chan_stride != per) {
      if (pdmp3_hip_copy_from_device(c->dst, from, per * sizeof(float)) != PDMP3_HIP_OK ||
          pdmp3_hip_copy_from_device(c->dst + c->chan_stride, from + per, per * sizeof(float)) != PDMP3_HIP_OK) { rc = -1; goto out; }
      continue;
    }
    size_t floats = (size_t)C * per;
    int j = i + 1;
    for (; j < nd && host[j] >= 0; j++) {
      const pdmp3_amd_audio_clip* n = &clips[host[j]];
      if (n->dst != c->dst + floats || (C == 2 && n->chan_stride != per)) break;
      floats += (size_t)C * per;
    }
    if (pdmp3_hip_copy_from_device(c->dst, from, floats * sizeof(float)) != PDMP3_HIP_OK) { rc = -1; goto out; }
    i = j - 1;
  }
out:
  free(ac); free(av); free(ds); free(host);
  return rc;
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
/* The short-time Fourier transform's course with another plan, table and launch: the rows through the audio call into stage
 * 2, k_clip_cqt behind it, host destinations through stage 1.  With `chroma` (whose cqt is `spec`) the
 * plan is chroma_plan's, a frame n_chroma floats and the kernel k_clip_chroma; the table and its cache are the same. */
static int cqt_clips(struct bulk* b, const pdmp3_amd_audio_clip* clips, int n_clips, const pdmp3_amd_cqt_spec* spec,
                     const pdmp3_amd_chroma_spec* chroma, long long* valid) {
  if (!b || !b->hs || !b->bits_mode || !spec || n_clips < 0 || (n_clips && (!clips || !valid)) || spec->n_frames < 0) return -1;
  const long long F = spec->n_frames;
  int C = spec->channels, rc = 0;
  long sr = spec->rate;
  if (C < 0 || C > 2 || sr < 0) return -1;
  for (int k = 0; k < n_clips; k++) {
    const pdmp3_amd_audio_clip* c = &clips[k];
    if (!c->index || (!c->mp3 && c->n) || c->n != c->index->n || c->start < 0 || (F && !c->dst)) return -1;
    if ((c->index->iso & PDMP3_ISO_LSF) != (b->id->iso & PDMP3_ISO_LSF)) return -1;
    if (c->index->frames < 0 || c->index->mixed) continue;
    const int cs = c->index->stereo ? 2 : 1;
    if (!spec->channels) {
      if (C && C != cs) return -1;                   /* (no channel count asked for, and the clips' differ) */
      C = cs;
    }
    if (!spec->rate && c->index->frames) {
      if (sr && sr != c->index->rate) return -1;     /* (no rate asked for, and the clips' differ: one time line a call) */
      sr = c->index->rate;
    }
  }
  if (!C) C = 1;
  if (!sr) sr = 44100;                               /* (no clip to decode, or only streams without frames) */
  pdmp3_cqt_params P;
  pdmp3_chroma_params S;
  if (chroma) {
    if (chroma_plan(chroma, sr, &S) != 0) return -1;
    P = S.cqt;
  } else if (cqt_plan(spec, sr, &P) != 0) return -1;                  /* (the check's verdict and the plan in one) */
  /* a frame reads N = N_0 = 2 h_0 + 1 samples, its centre the sample N / 2 = h_0; the table's rows behind them are zeros */
  const int N = 2 * P.half0 + 1, H = spec->hop;
  const int per_frame = chroma ? chroma->n_chroma : P.n_bins * (spec->out_mode == 0 ? 2 : 1);     /* floats of a frame */
  if (F > 0x7fffffffLL / (per_frame > H ? per_frame : H) - 2 * N) return -1;                /* (a row's samples and floats stay inside 31 bits) */
  const size_t per = (size_t)per_frame * (size_t)F;                   /* floats of a channel's output */
  for (int k = 0; k < n_clips; k++) if (C == 2 && F && clips[k].chan_stride < per) return -1;
  const long long T = F ? (F - 1) * H + N : 0;                        /* samples of a row: what F frames read */
  const size_t Ts = ((size_t)T + 3) & ~(size_t)3;
  pdmp3_amd_audio_clip* ac = (pdmp3_amd_audio_clip*)calloc((size_t)n_clips + 1, sizeof *ac);
  long long* av = (long long*)calloc((size_t)n_clips + 1, sizeof *av);
  pdmp3_mel_desc* ds = (pdmp3_mel_desc*)calloc((size_t)n_clips + 1, sizeof *ds);
  int* host = (int*)calloc((size_t)n_clips + 1, sizeof *host);       /* per descriptor: its clip, if that one's rows go to host memory, else -1 */
  int nd = 0;
  size_t out_floats = 0;
  if (!ac || !av || !ds || !host) { rc = -1; goto out; }
  for (int k = 0; k < n_clips; k++) {
    const pdmp3_amd_audio_clip* c = &clips[k];
    const pdmp3_amd_index* ix = c->index;
    if (ix->frames < 0) { valid[k] = PDMP3_BULK_REPLAY; rc = PDMP3_BULK_REPLAY; continue; }
    if (ix->mixed) { valid[k] = PDMP3_BULK_MIXED_FORMAT; if (rc != PDMP3_BULK_REPLAY) rc = PDMP3_BULK_MIXED_FORMAT; continue; }
    audio_plan p;
    if (audio_plan_init(&p, ix->frames ? ix->rate : sr, sr, spec->width, spec->rolloff) != 0) { rc = -1; goto out; }
    const long long Nin = ix->frames * (ix->frames ? ix->spf : 0);
    const long long J = (long long)(((__int128)Nin * p.L + p.M - 1) / p.M);
    const long long left = J - c->start;
    valid[k] = left <= 0 ? 0 : (left + H - 1) / H < F ? (left + H - 1) / H : F;
    if (!F) continue;
    /* the row: the span from max(0, start - N / 2) on, `lead` zeros in front of it */
    const long long s0 = c->start > N / 2 ? c->start - N / 2 : 0;
    ac[nd].mp3 = c->mp3; ac[nd].n = c->n; ac[nd].index = ix;
    ac[nd].start = s0;
    ac[nd].chan_stride = Ts;
    ds[nd].lead = (uint32_t)(s0 - (c->start - N / 2));
    ds[nd].src_chan_stride = Ts;
    const size_t row_bytes = ((size_t)(C - 1) * c->chan_stride + per) * sizeof(float);
    if (pdmp3_hip_host_is_pinned(c->dst, row_bytes) == 2) { host[nd] = -1; ds[nd].dst = (uint64_t)(uintptr_t)c->dst; ds[nd].dst_chan_stride = c->chan_stride; }
    else { host[nd] = k; ds[nd].dst = out_floats; ds[nd].dst_chan_stride = per; out_floats += (size_t)C * per; }
    nd++;
  }
  if (!nd) goto out;
  const float* table = cqt_table(b, spec, sr, &P);
  if (!table) { rc = -1; goto out; }
  if (pdmp3_amd_bulk_wait(b) != 0) { rc = -1; goto out; }
  float* sig = (float*)pdmp3_hip_stream_audio_stage(b->hs, 2, (size_t)nd * (size_t)C * Ts * sizeof(float));
  if (!sig) { rc = -1; goto out; }
  for (int i = 0; i < nd; i++) {
    ac[i].dst = sig + (size_t)i * (size_t)C * Ts;
    ds[i].src = (uint64_t)(uintptr_t)ac[i].dst;
  }
  /* the rows through the audio call as it is (device destinations: k_clip_audio writes them itself) */
  {
    pdmp3_amd_audio_spec as;
    memset(&as, 0, sizeof as);
    as.rate = sr; as.channels = C; as.n_samples = T; as.width = spec->width; as.rolloff = spec->rolloff;
    if (pdmp3_amd_bulk_decode_clips_audio(b, ac, nd, &as, av) != 0) { rc = -1; goto out; }
  }
  /* (the audio call may have grown stage 1 for nothing of ours: it is free for the rows of host destinations) */
  float* out_stage = out_floats ? (float*)pdmp3_hip_stream_audio_stage(b->hs, 1, out_floats * sizeof(float)) : NULL;
  if (out_floats && !out_stage) { rc = -1; goto out; }
  for (int i = 0; i < nd; i++) if (host[i] >= 0) ds[i].dst = (uint64_t)(uintptr_t)(out_stage + ds[i].dst);
  P.n_in = T; P.n_frames = (int32_t)F; P.channels = C; P.floor = spec->out_mode >= 3 ? (float)spec->floor : 0.0f;
  const size_t table_rows = (size_t)P.tile_at[P.n_tiles - 1] + (size_t)P.tile_rows[P.n_tiles - 1];
  if (chroma) S.cqt = P;
  if ((chroma ? pdmp3_hip_clip_chroma(b->hs, CLIP_SLOT, ds, nd, table, table_rows, &S)
              : pdmp3_hip_clip_cqt(b->hs, CLIP_SLOT, ds, nd, table, table_rows, &P)) != PDMP3_HIP_OK) {
    fprintf(stderr, "pdmp3: engine failure: %s\n", pdmp3_hip_last_error());
    rc = -1; goto out;
  }
  /* host destinations: rows that lie one behind the other in the caller's memory as they do in the stage leave in one copy */
  for (int i = 0; i < nd; i++) {
    if (host[i] < 0) continue;
    const pdmp3_amd_audio_clip* c = &clips[host[i]];
    const float* from = (const float*)(uintptr_t)ds[i].dst;
    if (C == 2 && c->chan_stride != per) {
      if (pdmp3_hip_copy_from_device(c->dst, from, per * sizeof(float)) != PDMP3_HIP_OK ||
          pdmp3_hip_copy_from_device(c->dst + c->chan_stride, from + per, per * sizeof(float)) != PDMP3_HIP_OK) { rc = -1; goto out; }
      continue;
    }
    size_t floats = (size_t)C * per;
    int j = i + 1;
    for (; j < nd && host[j] >= 0; j++) {
      const pdmp3_amd_audio_clip* n = &clips[host[j]];
      if (n->dst != c->dst + floats || (C == 2 && n->chan_stride != per)) break;
      floats += (size_t)C * per;
    }
    if (pdmp3_hip_copy_from_device(c->dst, from, floats * sizeof(float)) != PDMP3_HIP_OK) { rc = -1; goto out; }
    i = j - 1;
  }
out:
  free(ac); free(av); free(ds); free(host);
  return rc;
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
