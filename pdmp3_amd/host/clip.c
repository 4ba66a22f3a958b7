/* clip.c -- libpdmp3.so: stream indices, the exact halo of a frame range, and the whole-stream decoder's clips
 * (include/pdmp3_bulk.h: pdmp3_amd_index_*, pdmp3_amd_bulk_decode_clips, pdmp3_amd_bulk_parse_range).  The halo rule and
 * its reasoning: DESIGN.md section 8.  The calls that turn clips into float batches and features are clip_features.c's.  See
 * host_internal.h for the map of the library. */
#include "bulk_internal.h"
#include "../../include/pdmp3_node.h"

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
