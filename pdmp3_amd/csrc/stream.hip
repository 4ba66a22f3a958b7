// stream.hip -- pdmp3_hip_stream of include/pdmp3_hip.h: the host-buffer streaming helper (pinned staging,
// hipMemcpyAsync both ways).  Host code only: buffers, events and the order of a slot's commands.  Which kernel runs on
// which grid is engine.hip's business (engine_internal.h: launch_decode, unpack_window_head / _carry).
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "engine_internal.h"
#include "unpack_core.h"
#include "resample_core.h"
#include "pitch_core.h"
#include "pyin_core.h"
#include "tempogram_core.h"
#include "beat_core.h"
#include "hpss_core.h"
#include "mfcc_long_core.h"

using namespace pdmp3;

// One pdmp3_hip_stream = one decoder's carried state + up to kMaxSlots staging slots.  Each slot has its own
// HIP stream (H2D -> k_decode -> D2H), so slot w+1's upload overlaps slot w's kernel and download over the
// two PCIe directions; the kernels themselves are chained in submit order through `ev_state` because each one
// starts from the synthesis state its predecessor left (and they share the stream's d_state_tmp).
constexpr int kMaxSlots = 8;
struct StreamSlot {
  hipStream_t stream;
  hipEvent_t done;
  int16_t* h_spectra; pdmp3_gc_side* h_side; int16_t* h_pcm;     // pinned
  int16_t* d_spectra; pdmp3_gc_side* d_side; int16_t* d_pcm;
  int16_t* d_pair_sp; pdmp3_gc_side* d_pair_sd;                   // LSF launches: the regrouped records (allocated on first use, (max_frames + 1) / 2 frames)
  // bitstream-level input (allocated on first use)
  pdmp3_frame_bits* h_bits; uint8_t* h_res;                       // pinned
  pdmp3_frame_bits* d_bits; uint8_t* d_res; GcRaw* d_raw; uint32_t* d_outc; unsigned* d_mcnt;
  pdmp3_row_desc* h_desc; pdmp3_row_desc* d_desc; uint8_t* d_pool;   // compact bits input: pinned descriptors; the pool is h_res
  uint8_t* h_in; uint8_t* d_in;   // the blocks h_desc | h_bits | h_res and d_desc | d_bits | d_pool point into
  pdmp3_clip_piece* h_pieces; pdmp3_clip_piece* d_pieces; uint8_t* d_stage;   // clips (allocated on first use): the pieces' table, the stage
  int busy;
  int direct;                     // the latest record submit ran on the pinned host buffers themselves (submit_records)
};
struct pdmp3_hip_stream {
  pdmp3_hip_ctx* ctx;
  int max_frames, n_slots;
  StreamSlot s[kMaxSlots];
  hipEvent_t ev_state;       // recorded after the latest kernel + state copy
  int have_state_ev;
  float* d_state;
  float* d_state_tmp;
  float* d_state_prev;       // d_state as it was before the latest submit of decoded records (pdmp3_hip_stream_rewind)
  uint16_t* d_sfstate;       // [2][256]: scalefactors / count1 carried from frame to frame (unpack_core.h), double-buffered
  int sf_cur;
  int have_bits;
  int f32;                   // PCM as float (pdmp3_hip_stream_set_f32): the slots' PCM buffers hold 9216 bytes per frame
  int lsf;                   // the records of the submits are LSF frames (pdmp3_hip_stream_set_lsf): pdmp3_hip_decode_lsf_frames' layout
  void* d_audio[4]; size_t audio_cap[4];   // clips as float batches (allocated on first use, grown on demand): the clips' int16 PCM, float rows for host destinations, the signal of the log-mel call, the tempogram call's stages
  void* d_audio_args; size_t audio_args_cap;      // ... and a launch's descriptors | frame table | filter tables
  void* d_clip_args; size_t clip_args_cap;        // the feature calls: a launch's descriptors | parts (clip_run)
};

extern "C" void pdmp3_hip_stream_destroy(pdmp3_hip_stream* hs) {
  if (!hs) return;
  (void)hipSetDevice(hs->ctx->device);
  for (int i = 0; i < hs->n_slots; ++i) {
    StreamSlot& t = hs->s[i];
    if (t.stream) { (void)hipStreamSynchronize(t.stream); (void)hipStreamDestroy(t.stream); }
    if (t.done) (void)hipEventDestroy(t.done);
    (void)hipHostFree(t.h_spectra); (void)hipHostFree(t.h_side); (void)hipHostFree(t.h_pcm);
    (void)hipFree(t.d_spectra); (void)hipFree(t.d_side); (void)hipFree(t.d_pcm); (void)hipFree(t.d_pair_sp); (void)hipFree(t.d_pair_sd);
    (void)hipHostFree(t.h_in);
    (void)hipFree(t.d_in); (void)hipFree(t.d_res); (void)hipFree(t.d_raw); (void)hipFree(t.d_outc); (void)hipFree(t.d_mcnt);
    (void)hipHostFree(t.h_pieces); (void)hipFree(t.d_pieces); (void)hipFree(t.d_stage);
  }
  (void)hipFree(hs->d_sfstate);
  (void)hipFree(hs->d_audio[0]); (void)hipFree(hs->d_audio[1]); (void)hipFree(hs->d_audio[2]); (void)hipFree(hs->d_audio[3]); (void)hipFree(hs->d_audio_args);
  (void)hipFree(hs->d_clip_args);
  if (hs->ev_state) (void)hipEventDestroy(hs->ev_state);
  (void)hipFree(hs->d_state);
  chain_release(hs->ctx, hs);
  (void)hipFree(hs->d_state_tmp);
  (void)hipFree(hs->d_state_prev);
  free(hs);
}

extern "C" int pdmp3_hip_stream_create_slots(pdmp3_hip_ctx* ctx, int max_frames, int n_slots, pdmp3_hip_stream** out) {
  if (!ctx || !out || max_frames < 1 || n_slots < 1 || n_slots > kMaxSlots)
    return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_stream_create: bad argument", hipSuccess);
  *out = nullptr;
  HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
  pdmp3_hip_stream* hs = (pdmp3_hip_stream*)calloc(1, sizeof *hs);
  if (!hs) return fail(PDMP3_HIP_ENOMEM, "calloc", hipSuccess);
  hs->ctx = ctx;
  hs->max_frames = max_frames;
  hs->n_slots = n_slots;
  const size_t n = (size_t)max_frames;
#define HS_TRY(call, what) do { hipError_t e_ = (call); if (e_ != hipSuccess) { pdmp3_hip_stream_destroy(hs); return fail(PDMP3_HIP_EDEVICE, what, e_); } } while (0)
  for (int i = 0; i < n_slots; ++i) {
    StreamSlot& t = hs->s[i];
    HS_TRY(hipStreamCreateWithFlags(&t.stream, hipStreamNonBlocking), "hipStreamCreate");
    HS_TRY(hipEventCreateWithFlags(&t.done, hipEventDisableTiming), "hipEventCreate");
    HS_TRY(hipHostMalloc((void**)&t.h_spectra, n * PDMP3_FRAME_SPECTRA_BYTES, hipHostMallocDefault), "hipHostMalloc spectra");
    HS_TRY(hipHostMalloc((void**)&t.h_side, n * PDMP3_FRAME_SIDE_BYTES, hipHostMallocDefault), "hipHostMalloc side");
    HS_TRY(hipHostMalloc((void**)&t.h_pcm, n * PDMP3_FRAME_PCM_BYTES, hipHostMallocDefault), "hipHostMalloc pcm");
    HS_TRY(hipMalloc((void**)&t.d_spectra, n * PDMP3_FRAME_SPECTRA_BYTES), "hipMalloc spectra");
    HS_TRY(hipMalloc((void**)&t.d_side, n * PDMP3_FRAME_SIDE_BYTES), "hipMalloc side");
    HS_TRY(hipMalloc((void**)&t.d_pcm, n * PDMP3_FRAME_PCM_BYTES), "hipMalloc pcm");
  }
  HS_TRY(hipEventCreateWithFlags(&hs->ev_state, hipEventDisableTiming), "hipEventCreate");
  HS_TRY(hipMalloc((void**)&hs->d_state, pdmp3_hip_state_bytes()), "hipMalloc state");
  HS_TRY(hipMalloc((void**)&hs->d_state_tmp, pdmp3_hip_state_bytes()), "hipMalloc state");
  HS_TRY(hipMalloc((void**)&hs->d_state_prev, pdmp3_hip_state_bytes()), "hipMalloc state");
  HS_TRY(hipMemsetAsync(hs->d_state, 0, pdmp3_hip_state_bytes(), hs->s[0].stream), "memset state");
  HS_TRY(hipStreamSynchronize(hs->s[0].stream), "sync");
#undef HS_TRY
  *out = hs;
  return PDMP3_HIP_OK;
}

extern "C" int pdmp3_hip_stream_create(pdmp3_hip_ctx* ctx, int max_frames, pdmp3_hip_stream** out) {
  return pdmp3_hip_stream_create_slots(ctx, max_frames, 1, out);
}

static int drain_slots(pdmp3_hip_stream* hs) {
  for (int i = 0; i < hs->n_slots; ++i) {
    HIP_TRY(hipStreamSynchronize(hs->s[i].stream), "stream sync");
    hs->s[i].busy = 0;
  }
  return PDMP3_HIP_OK;
}

extern "C" int pdmp3_hip_stream_reset(pdmp3_hip_stream* hs) {
  if (!hs) return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_stream_reset: NULL", hipSuccess);
  HIP_TRY(hipSetDevice(hs->ctx->device), "hipSetDevice");
  int rc = drain_slots(hs);
  if (rc != PDMP3_HIP_OK) return rc;
  hs->have_state_ev = 0;
  HIP_TRY(hipMemsetAsync(hs->d_state, 0, pdmp3_hip_state_bytes(), hs->s[0].stream), "memset state");
  if (hs->d_sfstate) HIP_TRY(hipMemsetAsync(hs->d_sfstate, 0, 2 * 256 * sizeof(uint16_t), hs->s[0].stream), "memset sfstate");
  HIP_TRY(hipStreamSynchronize(hs->s[0].stream), "sync");
  return PDMP3_HIP_OK;
}

#define SLOT_OK(hs, i) ((hs) && (i) >= 0 && (i) < (hs)->n_slots)
extern "C" int pdmp3_hip_stream_slots(const pdmp3_hip_stream* hs) { return hs ? hs->n_slots : 0; }
extern "C" int pdmp3_hip_stream_capacity(const pdmp3_hip_stream* hs) { return hs ? hs->max_frames : 0; }
extern "C" int16_t* pdmp3_hip_stream_slot_spectra(pdmp3_hip_stream* hs, int slot) { return SLOT_OK(hs, slot) ? hs->s[slot].h_spectra : nullptr; }
extern "C" pdmp3_gc_side* pdmp3_hip_stream_slot_side(pdmp3_hip_stream* hs, int slot) { return SLOT_OK(hs, slot) ? hs->s[slot].h_side : nullptr; }
extern "C" const int16_t* pdmp3_hip_stream_slot_pcm(pdmp3_hip_stream* hs, int slot) { return SLOT_OK(hs, slot) ? hs->s[slot].h_pcm : nullptr; }
extern "C" int16_t* pdmp3_hip_stream_spectra(pdmp3_hip_stream* hs) { return pdmp3_hip_stream_slot_spectra(hs, 0); }
extern "C" pdmp3_gc_side* pdmp3_hip_stream_side(pdmp3_hip_stream* hs) { return pdmp3_hip_stream_slot_side(hs, 0); }
extern "C" const int16_t* pdmp3_hip_stream_pcm(pdmp3_hip_stream* hs) { return pdmp3_hip_stream_slot_pcm(hs, 0); }

// PCM of a batch to its destination: into the slot's pinned buffer, or -- when the caller hands over pinned host
// memory (pdmp3_hip_host_alloc) or DEVICE memory of its own -- straight to where it is wanted, `row` bytes per frame (4608; 2304 = mono frames
// packed densely out of their 4608-byte slots).
static int download_pcm(StreamSlot& t, size_t n, void* host_dst, int row, bool lsf = false) {
  if (lsf && host_dst) {
    // LSF frames (pdmp3_hip_decode_lsf_frames): stereo frames lie back to back, 2304 bytes each; mono frames in pairs in the
    // first half of a 4608-byte place
    if (row == PDMP3_FRAME_PCM_BYTES / 2) {
      HIP_TRY(hipMemcpyAsync(host_dst, t.d_pcm, n * (size_t)row, hipMemcpyDefault, t.stream), "pcm (direct, LSF)");
    } else {
      if (n / 2) HIP_TRY(hipMemcpy2DAsync(host_dst, 2304, t.d_pcm, PDMP3_FRAME_PCM_BYTES, 2304, n / 2, hipMemcpyDefault, t.stream), "pcm (direct, LSF mono)");
      if (n & 1) HIP_TRY(hipMemcpyAsync((char*)host_dst + (n / 2) * 2304, (const char*)t.d_pcm + (n / 2) * PDMP3_FRAME_PCM_BYTES, 1152, hipMemcpyDefault, t.stream), "pcm (direct, LSF mono tail)");
    }
    return PDMP3_HIP_OK;
  }
  if (!host_dst) {
    HIP_TRY(hipMemcpyAsync(t.h_pcm, t.d_pcm, n * PDMP3_FRAME_PCM_BYTES, hipMemcpyDeviceToHost, t.stream), "D2H pcm");
  } else if (row == PDMP3_FRAME_PCM_BYTES) {
    HIP_TRY(hipMemcpyAsync(host_dst, t.d_pcm, n * PDMP3_FRAME_PCM_BYTES, hipMemcpyDefault, t.stream), "pcm (direct)");
  } else {
    HIP_TRY(hipMemcpy2DAsync(host_dst, (size_t)row, t.d_pcm, PDMP3_FRAME_PCM_BYTES, (size_t)row, n, hipMemcpyDefault, t.stream),
            "pcm (direct, packed)");
  }
  return PDMP3_HIP_OK;
}

extern "C" int pdmp3_hip_host_alloc(size_t bytes, void** out) {
  if (!out) return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_host_alloc: out is NULL", hipSuccess);
  *out = nullptr;
  HIP_TRY(hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault), "hipHostMalloc");
  return PDMP3_HIP_OK;
}
extern "C" void pdmp3_hip_host_free(void* p) { if (p) (void)hipHostFree(p); }
// What the runtime knows of the first and the last byte of [p, p + bytes) (bytes <= 1: of the first, `last` = `first`);
// false: it does not know one of them.  What makes a range good enough differs from caller to caller.
struct PtrRange { hipPointerAttribute_t first, last; };
static bool classify_range(const void* p, size_t bytes, PtrRange* r) {
  if (hipPointerGetAttributes(&r->first, p) != hipSuccess) { (void)hipGetLastError(); return false; }
  r->last = r->first;
  if (bytes > 1 && hipPointerGetAttributes(&r->last, (const char*)p + bytes - 1) != hipSuccess) { (void)hipGetLastError(); return false; }
  return true;
}
extern "C" int pdmp3_hip_host_is_pinned(const void* p, size_t bytes) {
  PtrRange r;
  if (!p || !classify_range(p, bytes, &r)) return 0;
  if (r.first.type != hipMemoryTypeHost && r.first.type != hipMemoryTypeDevice) return 0;
  if (r.last.type != r.first.type) return 0;
  return r.first.type == hipMemoryTypeHost ? 1 : 2;
}

extern "C" int pdmp3_hip_copy_to_dest(void* dst, const void* src_host, size_t bytes) {
  if (!bytes) return PDMP3_HIP_OK;
  if (!dst || !src_host) return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_copy_to_dest: NULL", hipSuccess);
  HIP_TRY(hipMemcpy(dst, src_host, bytes, hipMemcpyDefault), "copy to destination");
  return PDMP3_HIP_OK;
}

// PCM of the record-level submits (pdmp3_hip_stream_submit / _decode) as float from now on (on != 0) or int16 again.
// Call with nothing in flight; the slots' PCM buffers are re-allocated.  The accessors return the same pointers'
// new values, to be read as float: frame f at floats [f*2304, f*2304+2304).
extern "C" int pdmp3_hip_stream_set_f32(pdmp3_hip_stream* hs, int on) {
  if (!hs) return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_stream_set_f32: NULL", hipSuccess);
  on = on ? 1 : 0;
  if (hs->f32 == on) return PDMP3_HIP_OK;
  HIP_TRY(hipSetDevice(hs->ctx->device), "hipSetDevice");
  int rc = drain_slots(hs);
  if (rc != PDMP3_HIP_OK) return rc;
  const size_t bytes = (size_t)hs->max_frames * (on ? PDMP3_FRAME_PCM_F32_BYTES : PDMP3_FRAME_PCM_BYTES);
  for (int i = 0; i < hs->n_slots; ++i) {
    StreamSlot& t = hs->s[i];
    (void)hipHostFree(t.h_pcm); t.h_pcm = nullptr;
    (void)hipFree(t.d_pcm); t.d_pcm = nullptr;
    HIP_TRY(hipHostMalloc((void**)&t.h_pcm, bytes, hipHostMallocDefault), "hipHostMalloc pcm");
    HIP_TRY(hipMalloc((void**)&t.d_pcm, bytes), "hipMalloc pcm");
  }
  hs->f32 = on;
  return PDMP3_HIP_OK;
}

static int submit_records(pdmp3_hip_stream* hs, int slot, int n_frames, void* host_dst, int row);
// row_bytes of a _to destination: 4608 / 2304 for MPEG-1 frames, 2304 (stereo) / 1152 (mono) for LSF ones
static bool row_bytes_ok(const pdmp3_hip_stream* hs, int row_bytes) {
  if (hs && hs->lsf) return row_bytes == PDMP3_FRAME_PCM_BYTES / 2 || row_bytes == PDMP3_FRAME_PCM_BYTES / 4;
  return row_bytes == PDMP3_FRAME_PCM_BYTES || row_bytes == PDMP3_FRAME_PCM_BYTES / 2;
}
extern "C" int pdmp3_hip_stream_submit(pdmp3_hip_stream* hs, int slot, int n_frames) {
  return submit_records(hs, slot, n_frames, nullptr, PDMP3_FRAME_PCM_BYTES);
}
extern "C" int pdmp3_hip_stream_submit_to(pdmp3_hip_stream* hs, int slot, int n_frames, void* pinned_dst, int row_bytes) {
  if (pinned_dst && !row_bytes_ok(hs, row_bytes))
    return fail(PDMP3_HIP_EINVAL, hs && hs->lsf ? "pdmp3_hip_stream_submit_to: row_bytes of LSF frames must be 2304 (stereo) or 1152 (mono)"
                                                : "pdmp3_hip_stream_submit_to: row_bytes must be 4608 or 2304", hipSuccess);
  return submit_records(hs, slot, n_frames, pinned_dst, row_bytes);
}
// the slot's buffers for an LSF launch's regrouped records (launch_decode pair_sp / pair_sd): allocated once, on the first LSF submit
static int slot_pairs(pdmp3_hip_stream* hs, StreamSlot& t) {
  if (!hs->lsf || t.d_pair_sp) return PDMP3_HIP_OK;
  const size_t np = ((size_t)hs->max_frames + 1) / 2;
  HIP_TRY(hipMalloc((void**)&t.d_pair_sp, np * PDMP3_FRAME_SPECTRA_BYTES), "hipMalloc LSF pairs");
  if (hipMalloc((void**)&t.d_pair_sd, np * PDMP3_FRAME_SIDE_BYTES) != hipSuccess) { (void)hipFree(t.d_pair_sp); t.d_pair_sp = nullptr; return fail(PDMP3_HIP_ENOMEM, "hipMalloc LSF pairs", hipGetLastError()); }
  return PDMP3_HIP_OK;
}
// The decode launch of n of the slot's records at sp / sd on the slot's HIP stream: PCM to `pcm` (float if the stream object
// is set so), from the stream object's state to its state_tmp.
static DecodeLaunch slot_request(pdmp3_hip_stream* hs, StreamSlot& t, const int16_t* sp, const pdmp3_gc_side* sd, int n, void* pcm, bool leave_state_in_tmp) {
  DecodeLaunch q;
  q.spectra = sp; q.side = sd; q.n_frames = n;
  q.lsf = hs->lsf != 0; q.pair_sp = t.d_pair_sp; q.pair_sd = t.d_pair_sd;
  q.pcm = pcm; q.f32 = hs->f32 != 0;
  q.state = hs->d_state; q.state_tmp = hs->d_state_tmp; q.leave_state_in_tmp = leave_state_in_tmp;
  q.stream = t.stream; q.owner = hs;
  return q;
}
static int submit_records(pdmp3_hip_stream* hs, int slot, int n_frames, void* host_dst, int row) {
  if (!SLOT_OK(hs, slot) || n_frames < 0 || n_frames > hs->max_frames)
    return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_stream_submit: bad argument", hipSuccess);
  StreamSlot& t = hs->s[slot];
  if (t.busy) return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_stream_submit: slot still in flight (wait for it first)", hipSuccess);
  if (n_frames == 0) return PDMP3_HIP_OK;
  HIP_TRY(hipSetDevice(hs->ctx->device), "hipSetDevice");
  { const int rcp = slot_pairs(hs, t); if (rcp != PDMP3_HIP_OK) return rcp; }
  const size_t n = (size_t)n_frames;
  if (hs->f32 && host_dst) return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_stream_submit_to: not with float PCM", hipSuccess);
  // Small batches (the streaming API's read-ahead: a handful of frames per call): no copies at all.  The kernel reads the
  // records from the slot's PINNED host buffers and writes the PCM into pinned host memory itself -- a few KB each way,
  // one PCIe round trip under the waves' first phase instead of two copy commands in front of the kernel and one behind
  // it -- and the three state buffers rotate instead of being copied (previous <- current <- next).  Per batch: one
  // launch, two event records, one wait.  (PDMP3_HIP_DIRECT_MAX: largest such batch in frames, 0 = never.)
  t.direct = 0;
  // (the kernel itself stores into host_dst on this path: only where it certainly can -- pinned host memory, or memory of
  //  THIS device; registered / managed memory and another GPU's memory take the copy path, whose hipMemcpyAsync sorts it out)
  bool dst_ok = true;
  if (host_dst) {
    PtrRange r;                                  // (its first byte)
    dst_ok = classify_range(host_dst, 1, &r) &&
             ((r.first.type == hipMemoryTypeHost && !r.first.isManaged) || (r.first.type == hipMemoryTypeDevice && r.first.device == hs->ctx->device));
  }
  if (n_frames <= hs->ctx->direct_max_frames && dst_ok && (!host_dst || row == PDMP3_FRAME_PCM_BYTES) && !(hs->lsf && host_dst)) {
    // (a stream object with ONE slot -- the streaming API's -- has one HIP stream: its batches are in order anyway, and
    //  its wait is for that stream: no events at all, each of which is a call here and a packet of its own on the queue)
    const bool lone = hs->n_slots == 1;
    if (!lone && hs->have_state_ev) HIP_TRY(hipStreamWaitEvent(t.stream, hs->ev_state, 0), "wait for the previous batch's state");
    void* dst = host_dst ? host_dst : (void*)t.h_pcm;
    int rc = launch_decode(hs->ctx, slot_request(hs, t, t.h_spectra, t.h_side, n_frames, dst, true));
    if (rc != PDMP3_HIP_OK) return rc;
    float* const was_prev = hs->d_state_prev;
    hs->d_state_prev = hs->d_state;            // (what pdmp3_hip_stream_rewind goes back to)
    hs->d_state = hs->d_state_tmp;             // the kernel left the new state here
    hs->d_state_tmp = was_prev;
    if (!lone) {
      HIP_TRY(hipEventRecord(hs->ev_state, t.stream), "record state event");
      hs->have_state_ev = 1;
      HIP_TRY(hipEventRecord(t.done, t.stream), "record done event");
    }
    t.busy = 1;
    t.direct = lone ? 2 : 1;                   // 2: pdmp3_hip_stream_wait synchronises the stream
    return PDMP3_HIP_OK;
  }
  HIP_TRY(hipMemcpyAsync(t.d_spectra, t.h_spectra, n * PDMP3_FRAME_SPECTRA_BYTES, hipMemcpyHostToDevice, t.stream), "H2D spectra");
  HIP_TRY(hipMemcpyAsync(t.d_side, t.h_side, n * PDMP3_FRAME_SIDE_BYTES, hipMemcpyHostToDevice, t.stream), "H2D side");
  if (hs->have_state_ev) HIP_TRY(hipStreamWaitEvent(t.stream, hs->ev_state, 0), "wait for the previous batch's state");
  HIP_TRY(hipMemcpyAsync(hs->d_state_prev, hs->d_state, pdmp3_hip_state_bytes(), hipMemcpyDeviceToDevice, t.stream), "keep the state");
  int rc = launch_decode(hs->ctx, slot_request(hs, t, t.d_spectra, t.d_side, n_frames, t.d_pcm, false));
  if (rc != PDMP3_HIP_OK) return rc;
  HIP_TRY(hipEventRecord(hs->ev_state, t.stream), "record state event");
  hs->have_state_ev = 1;
  if (hs->f32) HIP_TRY(hipMemcpyAsync(t.h_pcm, t.d_pcm, n * PDMP3_FRAME_PCM_F32_BYTES, hipMemcpyDeviceToHost, t.stream), "D2H pcm");
  else rc = download_pcm(t, n, host_dst, row, hs->lsf != 0);
  if (rc != PDMP3_HIP_OK) return rc;
  HIP_TRY(hipEventRecord(t.done, t.stream), "record done event");
  t.busy = 1;
  return PDMP3_HIP_OK;
}

// The records of this stream object's following submits are LSF frames (on != 0: decoded like pdmp3_hip_decode_lsf_frames,
// the PCM in its layout) or MPEG-1 frames again.  A setting of the host's for the next submit; the synthesis state is
// the same block either way.
extern "C" int pdmp3_hip_stream_set_lsf(pdmp3_hip_stream* hs, int on) {
  if (!hs) return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_stream_set_lsf: NULL", hipSuccess);
  hs->lsf = on != 0;
  return PDMP3_HIP_OK;
}

extern "C" int pdmp3_hip_stream_wait(pdmp3_hip_stream* hs, int slot) {
  if (!SLOT_OK(hs, slot)) return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_stream_wait: bad argument", hipSuccess);
  StreamSlot& t = hs->s[slot];
  if (!t.busy) return PDMP3_HIP_OK;
  HIP_TRY(hipSetDevice(hs->ctx->device), "hipSetDevice");
  if (t.direct == 2) HIP_TRY(hipStreamSynchronize(t.stream), "stream sync");
  else HIP_TRY(hipEventSynchronize(t.done), "event sync");
  t.busy = 0;
  return PDMP3_HIP_OK;
}

// 1: pdmp3_hip_stream_wait(hs, slot) would return at once (nothing submitted, or the GPU is through with it); 0: not yet.
// For the thread that would call the wait (the whole-stream decoder asks how much the GPU still has to do before it
// decides how many frames the next window gets).
extern "C" int pdmp3_hip_stream_done(pdmp3_hip_stream* hs, int slot) {
  if (!SLOT_OK(hs, slot)) return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_stream_done: bad argument", hipSuccess);
  StreamSlot& t = hs->s[slot];
  if (!t.busy) return 1;
  const hipError_t e = t.direct == 2 ? hipStreamQuery(t.stream) : hipEventQuery(t.done);
  if (e == hipErrorNotReady) { (void)hipGetLastError(); return 0; }
  return 1;                                     // (done, or an error the wait will report)
}

// Undo the slot's latest pdmp3_hip_stream_submit beyond its first keep_frames frames: the carried synthesis state
// becomes what it was after frame keep_frames - 1 of that batch (the state before the batch, then the kept frames
// again -- their records are still in the slot's device buffers).  Blocks until done.
extern "C" int pdmp3_hip_stream_rewind(pdmp3_hip_stream* hs, int slot, int keep_frames) {
  if (!SLOT_OK(hs, slot) || keep_frames < 0 || keep_frames > hs->max_frames)
    return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_stream_rewind: bad argument", hipSuccess);
  HIP_TRY(hipSetDevice(hs->ctx->device), "hipSetDevice");
  StreamSlot& t = hs->s[slot];
  HIP_TRY(hipStreamSynchronize(t.stream), "stream sync");
  t.busy = 0;
  HIP_TRY(hipMemcpyAsync(hs->d_state, hs->d_state_prev, pdmp3_hip_state_bytes(), hipMemcpyDeviceToDevice, t.stream), "restore the state");
  if (keep_frames) {
    // (the records are where the submit took them from: the pinned host buffers if it ran on those)
    const int16_t* sp = t.direct ? t.h_spectra : t.d_spectra;
    const pdmp3_gc_side* sd = t.direct ? t.h_side : t.d_side;
    const int rc = launch_decode(hs->ctx, slot_request(hs, t, sp, sd, keep_frames, t.d_pcm, false));
    if (rc != PDMP3_HIP_OK) return rc;
  }
  HIP_TRY(hipEventRecord(hs->ev_state, t.stream), "record state event");
  hs->have_state_ev = 1;
  HIP_TRY(hipStreamSynchronize(t.stream), "stream sync");
  return PDMP3_HIP_OK;
}

// ---- bitstream-level input ------------------------------------------------
static int ensure_bits(pdmp3_hip_stream* hs) {
  if (hs->have_bits) return PDMP3_HIP_OK;
  HIP_TRY(hipSetDevice(hs->ctx->device), "hipSetDevice");
  const size_t n = (size_t)hs->max_frames;
  for (int i = 0; i < hs->n_slots; ++i) {
    StreamSlot& t = hs->s[i];
    // descriptors | side info | rows or pool: ONE pinned block and one device block with the same layout, so that the
    // compact input of a window goes up in one copy (a hipMemcpyAsync call costs the submitting thread 20-40 us here)
    const size_t desc_bytes = n * sizeof(pdmp3_row_desc), bits_bytes = n * sizeof(pdmp3_frame_bits);
    const size_t pool_cap = n * PDMP3_RESERVOIR_BYTES + PDMP3_POOL_SLACK_BYTES + 16;
    HIP_TRY(hipHostMalloc((void**)&t.h_in, desc_bytes + bits_bytes + pool_cap, hipHostMallocDefault), "hipHostMalloc window input");
    HIP_TRY(hipMalloc((void**)&t.d_in, desc_bytes + bits_bytes + pool_cap), "hipMalloc window input");
    t.h_desc = reinterpret_cast<pdmp3_row_desc*>(t.h_in);
    t.h_bits = reinterpret_cast<pdmp3_frame_bits*>(t.h_in + desc_bytes);
    t.h_res = t.h_in + desc_bytes + bits_bytes;
    t.d_desc = reinterpret_cast<pdmp3_row_desc*>(t.d_in);
    t.d_bits = reinterpret_cast<pdmp3_frame_bits*>(t.d_in + desc_bytes);
    t.d_pool = t.d_in + desc_bytes + bits_bytes;
    HIP_TRY(hipMalloc((void**)&t.d_res, n * PDMP3_RESERVOIR_BYTES + 16), "hipMalloc reservoir");
    HIP_TRY(hipMalloc((void**)&t.d_raw, n * 4 * sizeof(GcRaw)), "hipMalloc raw");
    // rows of outcomes: one per block of kMergeBlk frames, then one per super-block; the super-blocks' counters (zero between launches)
    const size_t mblk = (n + kMergeBlk - 1) / kMergeBlk, msup = (mblk + kMergeSuper - 1) / kMergeSuper;
    HIP_TRY(hipMalloc((void**)&t.d_outc, (mblk + msup) * kMergeLanes * sizeof(uint32_t)), "hipMalloc merge outcomes");
    HIP_TRY(hipMalloc((void**)&t.d_mcnt, (msup + 1) * sizeof(unsigned)), "hipMalloc merge counters");
    HIP_TRY(hipMemset(t.d_mcnt, 0, (msup + 1) * sizeof(unsigned)), "memset merge counters");
  }
  HIP_TRY(hipMalloc((void**)&hs->d_sfstate, 2 * 256 * sizeof(uint16_t)), "hipMalloc sfstate");
  HIP_TRY(hipMemset(hs->d_sfstate, 0, 2 * 256 * sizeof(uint16_t)), "memset sfstate");
  // hipMemset returns before the device has run it, and the slots' streams are non-blocking: they do not wait for the null
  // stream.  Without this wait the zeroing of the scalefactor state could land AFTER the first window's k_merge_apply had
  // written it -- the second window of a fresh decoder then started from zeros (round 6: one whole-stream decode in ~2000
  // with fresh decoders differed by 1-3 LSB in frames 17-18; tools/ubench/malloc_async_probe.cpp mode M shows the mechanism)
  HIP_TRY(hipDeviceSynchronize(), "device sync after the memsets");
  hs->have_bits = 1;
  return PDMP3_HIP_OK;
}

extern "C" pdmp3_frame_bits* pdmp3_hip_stream_slot_bits(pdmp3_hip_stream* hs, int slot) {
  if (!SLOT_OK(hs, slot) || ensure_bits(hs) != PDMP3_HIP_OK) return nullptr;
  return hs->s[slot].h_bits;
}
extern "C" uint8_t* pdmp3_hip_stream_slot_reservoir(pdmp3_hip_stream* hs, int slot) {
  if (!SLOT_OK(hs, slot) || ensure_bits(hs) != PDMP3_HIP_OK) return nullptr;
  return hs->s[slot].h_res;
}

extern "C" pdmp3_row_desc* pdmp3_hip_stream_slot_rowdesc(pdmp3_hip_stream* hs, int slot) {
  if (!SLOT_OK(hs, slot) || ensure_bits(hs) != PDMP3_HIP_OK) return nullptr;
  return hs->s[slot].h_desc;
}
extern "C" uint8_t* pdmp3_hip_stream_slot_pool(pdmp3_hip_stream* hs, int slot) { return pdmp3_hip_stream_slot_reservoir(hs, slot); }
extern "C" size_t pdmp3_hip_stream_pool_bytes(const pdmp3_hip_stream* hs) { return hs ? (size_t)hs->max_frames * PDMP3_RESERVOIR_BYTES + PDMP3_POOL_SLACK_BYTES : 0; }

static int submit_bits(pdmp3_hip_stream* hs, int slot, int n_frames, void* host_dst, int row, size_t pool_bytes = 0, int clip_pieces = -1,
                       size_t stage_bytes = 0);
extern "C" int pdmp3_hip_stream_submit_pool_to(pdmp3_hip_stream* hs, int slot, int n_frames, size_t pool_bytes, void* pinned_dst, int row_bytes) {
  if (pinned_dst && !row_bytes_ok(hs, row_bytes))
    return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_stream_submit_pool_to: row_bytes must be 4608 or 2304 (LSF: 2304 or 1152)", hipSuccess);
  if (!pool_bytes || !hs || pool_bytes > pdmp3_hip_stream_pool_bytes(hs))
    return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_stream_submit_pool_to: bad pool size", hipSuccess);
  return submit_bits(hs, slot, n_frames, pinned_dst, row_bytes, pool_bytes);
}
extern "C" int pdmp3_hip_stream_submit_bits(pdmp3_hip_stream* hs, int slot, int n_frames) {
  return submit_bits(hs, slot, n_frames, nullptr, PDMP3_FRAME_PCM_BYTES);
}
extern "C" int pdmp3_hip_stream_submit_bits_to(pdmp3_hip_stream* hs, int slot, int n_frames, void* pinned_dst, int row_bytes) {
  if (pinned_dst && !row_bytes_ok(hs, row_bytes))
    return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_stream_submit_bits_to: row_bytes must be 4608 or 2304 (LSF: 2304 or 1152)", hipSuccess);
  return submit_bits(hs, slot, n_frames, pinned_dst, row_bytes);
}
static int ensure_clip(pdmp3_hip_stream* hs, StreamSlot& t) {
  if (t.d_stage) return PDMP3_HIP_OK;
  HIP_TRY(hipSetDevice(hs->ctx->device), "hipSetDevice");
  const size_t n = (size_t)hs->max_frames;
  HIP_TRY(hipHostMalloc((void**)&t.h_pieces, n * sizeof(pdmp3_clip_piece), hipHostMallocDefault), "hipHostMalloc clip pieces");
  HIP_TRY(hipMalloc((void**)&t.d_pieces, n * sizeof(pdmp3_clip_piece)), "hipMalloc clip pieces");
  HIP_TRY(hipMalloc((void**)&t.d_stage, n * PDMP3_FRAME_PCM_BYTES), "hipMalloc clip stage");
  return PDMP3_HIP_OK;
}
extern "C" void* pdmp3_hip_stream_slot_clip_stage(pdmp3_hip_stream* hs, int slot) {
  if (!SLOT_OK(hs, slot) || ensure_clip(hs, hs->s[slot]) != PDMP3_HIP_OK) return nullptr;
  return hs->s[slot].d_stage;
}
extern "C" int pdmp3_hip_stream_submit_bits_clips(pdmp3_hip_stream* hs, int slot, int n_frames, const pdmp3_clip_piece* pieces, int n_pieces,
                                                  size_t stage_bytes) {
  if (!SLOT_OK(hs, slot) || n_pieces < 0 || n_pieces > hs->max_frames || (n_pieces && !pieces) ||
      stage_bytes > (size_t)hs->max_frames * PDMP3_FRAME_PCM_BYTES || hs->f32)
    return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_stream_submit_bits_clips: bad argument", hipSuccess);
  StreamSlot& t = hs->s[slot];
  if (t.busy) return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_stream_submit_bits_clips: slot still in flight (wait for it first)", hipSuccess);
  const int rc = ensure_clip(hs, t);
  if (rc != PDMP3_HIP_OK) return rc;
  if (n_pieces) memcpy(t.h_pieces, pieces, (size_t)n_pieces * sizeof *pieces);
  return submit_bits(hs, slot, n_frames, nullptr, PDMP3_FRAME_PCM_BYTES, 0, n_pieces, stage_bytes);
}
static int submit_bits(pdmp3_hip_stream* hs, int slot, int n_frames, void* host_dst, int row, size_t pool_bytes, int clip_pieces,
                       size_t stage_bytes) {
  if (!SLOT_OK(hs, slot) || n_frames < 0 || n_frames > hs->max_frames)
    return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_stream_submit_bits: bad argument", hipSuccess);
  StreamSlot& t = hs->s[slot];
  if (t.busy) return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_stream_submit_bits: slot still in flight (wait for it first)", hipSuccess);
  if (n_frames == 0) return PDMP3_HIP_OK;
  int rc = ensure_bits(hs);
  if (rc != PDMP3_HIP_OK) return rc;
  HIP_TRY(hipSetDevice(hs->ctx->device), "hipSetDevice");
  const bool lsf = hs->lsf != 0;
  if (lsf) { rc = slot_pairs(hs, t); if (rc != PDMP3_HIP_OK) return rc; }   // (the records regrouped for the transforms: launch_decode)
  const size_t n = (size_t)n_frames;
  t.direct = 0;               // (the records of this submit are the device's: a rewind replays d_spectra, never h_spectra)
  if (pool_bytes) {           // compact input: descriptors, side info and pool up in one copy, rows rebuilt on the device
    // (Tried: k_rows reading descriptors, side info and pool straight from the pinned host block, no copy at all -- the
    //  kernel then runs at PCIe speed and the pipeline, which is bound by the kernels of a window, lost 20 %.)
    const size_t head = (size_t)hs->max_frames * (sizeof(pdmp3_row_desc) + sizeof(pdmp3_frame_bits));
    HIP_TRY(hipMemcpyAsync(t.d_in, t.h_in, head + pool_bytes, hipMemcpyHostToDevice, t.stream), "H2D window input");
  } else {
    HIP_TRY(hipMemcpyAsync(t.d_bits, t.h_bits, n * sizeof(pdmp3_frame_bits), hipMemcpyHostToDevice, t.stream), "H2D bits");
    HIP_TRY(hipMemcpyAsync(t.d_res, t.h_res, n * PDMP3_RESERVOIR_BYTES, hipMemcpyHostToDevice, t.stream), "H2D reservoir");
  }
  UnpackWindow w;
  w.stream = t.stream; w.n_frames = n_frames; w.lsf = lsf;
  w.desc = pool_bytes ? t.d_desc : nullptr; w.pool = t.d_pool;
  w.bits = t.d_bits; w.res = t.d_res;
  w.spectra = t.d_spectra; w.raw = t.d_raw;
  w.outc = t.d_outc; w.mcnt = t.d_mcnt;
  w.sf_in = hs->d_sfstate + 256 * hs->sf_cur; w.sf_out = hs->d_sfstate + 256 * (hs->sf_cur ^ 1);
  w.side = t.d_side;
  // what the window's frames do to the values that survive frames needs nothing of the batch before ...
  rc = unpack_window_head(hs->ctx, w);
  if (rc != PDMP3_HIP_OK) return rc;
  // ... everything from here on continues it (scalefactor / count1 carry, synthesis state)
  if (hs->have_state_ev) HIP_TRY(hipStreamWaitEvent(t.stream, hs->ev_state, 0), "wait for the previous batch's state");
  rc = unpack_window_carry(w);
  if (rc != PDMP3_HIP_OK) return rc;
  hs->sf_cur ^= 1;
  // A destination in THIS device's memory that takes whole 4608-byte rows: the kernel stores the PCM there itself (the
  // copy from the slot's buffer was 11 us of a window's 235 -- 75 MB through HBM for 8192 frames; end to end, A/B on one
  // box, four runs each: 26.5 against 25.9 M frames/s).  Pinned host memory
  // stays with the copy command: stores over PCIe from 256 CUs are slower than the DMA engine.
  // (LSF windows: their PCM layout is pdmp3_hip_decode_lsf_frames', which download_pcm sorts out)
  int16_t* pcm_out = t.d_pcm;
  if (!lsf && host_dst && row == PDMP3_FRAME_PCM_BYTES && !((uintptr_t)host_dst & 15)) {
    PtrRange r;                                  // (its first and its last byte)
    if (classify_range(host_dst, n * PDMP3_FRAME_PCM_BYTES, &r) && r.first.type == hipMemoryTypeDevice && r.last.type == hipMemoryTypeDevice &&
        r.first.device == hs->ctx->device && r.last.device == hs->ctx->device && !r.first.isManaged)
      pcm_out = (int16_t*)host_dst;
  }
  DecodeLaunch q = slot_request(hs, t, t.d_spectra, t.d_side, n_frames, pcm_out, true);
  q.f32 = false;              // (a window of bits comes out as int16 whatever pdmp3_hip_stream_set_f32 says)
  rc = launch_decode(hs->ctx, q);
  if (rc != PDMP3_HIP_OK) return rc;
  { float* x = hs->d_state; hs->d_state = hs->d_state_tmp; hs->d_state_tmp = x; }   // (the new state is where the kernel left it)
  HIP_TRY(hipEventRecord(hs->ev_state, t.stream), "record state event");
  hs->have_state_ev = 1;
  if (clip_pieces >= 0) {     // clips: the PCM stays in d_pcm, k_clip_pack places the kept frames (clip.hip)
    if (clip_pieces) {
      HIP_TRY(hipMemcpyAsync(t.d_pieces, t.h_pieces, (size_t)clip_pieces * sizeof(pdmp3_clip_piece), hipMemcpyHostToDevice, t.stream), "H2D clip pieces");
      HIP_TRY(pdmp3_launch_clip_pack(t.stream, t.d_pieces, clip_pieces, t.d_pcm), "launch k_clip_pack");
    }
    if (stage_bytes) HIP_TRY(hipMemcpyAsync(t.h_pcm, t.d_stage, stage_bytes, hipMemcpyDeviceToHost, t.stream), "D2H clip stage");
  } else if (pcm_out == t.d_pcm) {
    rc = download_pcm(t, n, host_dst, row, lsf);
    if (rc != PDMP3_HIP_OK) return rc;
  }
  HIP_TRY(hipEventRecord(t.done, t.stream), "record done event");
  t.busy = 1;
  return PDMP3_HIP_OK;
}

// ---- clips as float batches (resample.hip) ----
// plain hipMalloc, never stream-ordered; the old block goes first: nothing of the audio path is in flight
static int grow_device(void** p, size_t* cap, size_t bytes, const char* what) {
  if (*p && *cap >= bytes) return PDMP3_HIP_OK;
  (void)hipFree(*p);
  *p = nullptr; *cap = 0;
  const size_t want = bytes + bytes / 4 + 4096;
  HIP_TRY(hipMalloc(p, want), what);
  *cap = want;
  return PDMP3_HIP_OK;
}
extern "C" void* pdmp3_hip_stream_audio_stage(pdmp3_hip_stream* hs, int which, size_t bytes) {
  if (!hs || which < 0 || which > 3) return nullptr;
  if (hipSetDevice(hs->ctx->device) != hipSuccess) return nullptr;
  if (grow_device(&hs->d_audio[which], &hs->audio_cap[which], bytes ? bytes : 16, "hipMalloc audio stage") != PDMP3_HIP_OK) return nullptr;
  return hs->d_audio[which];
}
extern "C" int pdmp3_hip_clip_audio(pdmp3_hip_stream* hs, int slot, const pdmp3_audio_desc* descs, int n_clips, const uint32_t* frames,
                                    size_t n_frames, const float* tables, size_t n_coef, long long n_samples, int channels) {
  if (!SLOT_OK(hs, slot) || n_clips < 0 || (n_clips && !descs) || (n_frames && !frames) || (n_coef && !tables) || n_samples < 0 ||
      (channels != 1 && channels != 2))
    return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_audio: bad argument", hipSuccess);
  StreamSlot& t = hs->s[slot];
  if (t.busy) return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_audio: slot still in flight (wait for it first)", hipSuccess);
  if (!n_clips || !n_samples) return PDMP3_HIP_OK;
  HIP_TRY(hipSetDevice(hs->ctx->device), "hipSetDevice");
  // the LDS of the launch: the largest any of its clips asks for
  unsigned lds = 0;
  for (int k = 0; k < n_clips; k++) {
    const pdmp3_audio_desc& d = descs[k];
    if (d.M == d.L || !(d.flags & PDMP3_AUDIO_LDS_X)) continue;
    size_t b = (size_t)d.span_cap * channels * sizeof(float);
    if (d.flags & PDMP3_AUDIO_LDS_TABLE) b += (((size_t)d.L * (size_t)d.taps + 3) & ~(size_t)3) * sizeof(float);
    if ((d.span_cap & 3u) || (d.table & 3u) || d.taps < 1 || b > pdmp3::kAudioLdsMax)
      return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_audio: a clip's span and table do not fit LDS as its flags say", hipSuccess);
    if (b > lds) lds = (unsigned)b;
  }
  // descriptors | frame table | filter tables: one block, each part 256-byte aligned
  const size_t desc_bytes = ((size_t)n_clips * sizeof(pdmp3_audio_desc) + 255) & ~(size_t)255;
  const size_t frame_bytes = (n_frames * sizeof(uint32_t) + 255) & ~(size_t)255;
  const size_t table_bytes = n_coef * sizeof(float);
  if (const int rc = grow_device(&hs->d_audio_args, &hs->audio_args_cap, desc_bytes + frame_bytes + table_bytes + 16, "hipMalloc audio tables"); rc != PDMP3_HIP_OK)
    return rc;
  uint8_t* a = static_cast<uint8_t*>(hs->d_audio_args);
  HIP_TRY(hipMemcpyAsync(a, descs, (size_t)n_clips * sizeof(pdmp3_audio_desc), hipMemcpyHostToDevice, t.stream), "H2D audio descriptors");
  if (n_frames) HIP_TRY(hipMemcpyAsync(a + desc_bytes, frames, n_frames * sizeof(uint32_t), hipMemcpyHostToDevice, t.stream), "H2D audio frame table");
  if (n_coef) HIP_TRY(hipMemcpyAsync(a + desc_bytes + frame_bytes, tables, table_bytes, hipMemcpyHostToDevice, t.stream), "H2D filter tables");
  const int kMaxY = 32768;                     // (a grid's y extent ends at 65535)
  for (int k = 0; k < n_clips; k += kMaxY)
    HIP_TRY(pdmp3_launch_clip_audio(t.stream, reinterpret_cast<const pdmp3_audio_desc*>(a) + k, n_clips - k < kMaxY ? n_clips - k : kMaxY,
                                    reinterpret_cast<const uint32_t*>(a + desc_bytes), reinterpret_cast<const float*>(a + desc_bytes + frame_bytes),
                                    n_samples, channels, lds),
            "launch k_clip_audio");
  HIP_TRY(hipStreamSynchronize(t.stream), "stream sync");
  return PDMP3_HIP_OK;
}

// ---- the launches of the feature kernels ----
// A launch's device block is "descriptors | parts", each 256-byte aligned: a part is uploaded from host memory, zero-filled, or
// scratch that the kernels write before they read it.  One block serves every feature call: they block until their rows are
// written, so no two overlap in time.
struct ClipPart {
  enum Kind { kUpload, kZero, kScratch } kind;
  const void* src;           // kUpload: the host bytes
  size_t bytes;
};
// What every pdmp3_hip_clip_<feature> does once its arguments and parameters are accepted: the refusal of a busy slot, the
// empty call's return, the block, the uploads, and a grid per 32768 clips.  launch(dk, nk, k, part): clips [k, k + nk) of the
// launch, whose descriptors lie at dk on the device; part[i]: the device address of parts[i] (of the whole part: what a part
// holds per clip is the callable's to offset by k).
template <class Desc, size_t N, class Launch>
static int clip_run(pdmp3_hip_stream* hs, int slot, const char* name, const Desc* descs, int n_clips, long long n_frames,
                    const ClipPart (&parts)[N], Launch launch) {
  static_assert(sizeof(Desc) == 40, "pdmp3_mel_desc, pdmp3_fbank_desc, pdmp3_tempogram_desc, pdmp3_pyin_desc or pdmp3_beat_desc");
  char what[160];
  const auto at = [&](const char* step) -> const char* { snprintf(what, sizeof what, "%s: %s", name, step); return what; };
  StreamSlot& t = hs->s[slot];
  if (t.busy) return fail(PDMP3_HIP_EINVAL, at("slot still in flight (wait for it first)"), hipSuccess);
  if (!n_clips || !n_frames) return PDMP3_HIP_OK;
  HIP_TRY(hipSetDevice(hs->ctx->device), "hipSetDevice");
  const auto room = [](size_t bytes) { return (bytes + 255) & ~(size_t)255; };
  const size_t desc_bytes = (size_t)n_clips * sizeof(Desc);
  size_t total = room(desc_bytes);
  for (const ClipPart& p : parts) total += room(p.bytes);
  if (const int rc = grow_device(&hs->d_clip_args, &hs->clip_args_cap, total + 16, at("hipMalloc tables")); rc != PDMP3_HIP_OK) return rc;
  uint8_t* const a = static_cast<uint8_t*>(hs->d_clip_args);
  uint8_t* part[N] = {};
  HIP_TRY(hipMemcpyAsync(a, descs, desc_bytes, hipMemcpyHostToDevice, t.stream), at("H2D descriptors"));
  size_t off = room(desc_bytes);
  int i = 0;
  for (const ClipPart& p : parts) {
    part[i++] = a + off;
    if (p.bytes && p.kind == ClipPart::kUpload) HIP_TRY(hipMemcpyAsync(a + off, p.src, p.bytes, hipMemcpyHostToDevice, t.stream), at("H2D tables"));
    if (p.bytes && p.kind == ClipPart::kZero) HIP_TRY(hipMemsetAsync(a + off, 0, p.bytes, t.stream), at("memset"));
    off += room(p.bytes);
  }
  const int kMaxY = 32768;                     // (a grid's y extent ends at 65535)
  for (int k = 0; k < n_clips; k += kMaxY)
    HIP_TRY(launch(reinterpret_cast<const Desc*>(a) + k, n_clips - k < kMaxY ? n_clips - k : kMaxY, k, part), at("launch"));
  HIP_TRY(hipStreamSynchronize(t.stream), "stream sync");
  return PDMP3_HIP_OK;
}
static const float* as_floats(const uint8_t* p) { return reinterpret_cast<const float*>(p); }

// ---- log-mel features (mel.hip) ----
extern "C" int pdmp3_hip_clip_mel(pdmp3_hip_stream* hs, int slot, const pdmp3_mel_desc* descs, int n_clips, const float* dft, const float* fbt,
                                  const pdmp3_mel_params* params) {
  if (!SLOT_OK(hs, slot) || n_clips < 0 || (n_clips && !descs) || !dft || !fbt || !params)
    return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_mel: bad argument", hipSuccess);
  const pdmp3_mel_params& P = *params;
  // what the kernel's indexing relies on
  if (P.n_fft < 16 || P.n_fft > 1024 || (P.n_fft & 1) || P.rows != ((P.n_fft + 3) & ~3) || P.hop < 1 || P.hop > P.n_fft || P.row_pad < 0 ||
      P.bins16 != ((P.n_fft / 2 + 1 + 15) & ~15) || P.n_mels < 1 || P.n_mels > 256 || P.mels16 != ((P.n_mels + 15) & ~15) ||
      (P.tile != 16 && P.tile != 32) || (P.channels != 1 && P.channels != 2) || P.out_mode < 0 || P.out_mode > 3 || P.n_frames < 0 || P.n_in < 0 ||
      !(P.floor > 0.0f) || P.lds_bytes > PDMP3_MEL_LDS_MAX)
    return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_mel: bad parameters", hipSuccess);
  {
    const size_t span = (size_t)(P.tile - 1) * P.hop + P.rows, chunks = (span + P.hop - 1) / P.hop;
    const size_t first = chunks * (size_t)(P.hop + P.row_pad), mt = (size_t)P.mels16 * (P.tile + 1);
    if (P.span_floats < first || P.span_floats < mt || (size_t)P.lds_bytes < ((size_t)P.span_floats + (size_t)P.tile * (P.bins16 + 2)) * sizeof(float))
      return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_mel: a tile's span, powers and mel tile do not fit the LDS asked for", hipSuccess);
    if (((long long)P.n_frames + P.tile - 1) / P.tile * P.channels > 0x7fffffffLL)
      return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_mel: too many frames", hipSuccess);
  }
  // descriptors | row maxima | DFT table | filterbank
  return clip_run(hs, slot, "pdmp3_hip_clip_mel", descs, n_clips, P.n_frames,
                  {{ClipPart::kZero, nullptr, (size_t)n_clips * sizeof(unsigned)},
                   {ClipPart::kUpload, dft, (size_t)P.rows * 2 * (size_t)P.bins16 * sizeof(float)},
                   {ClipPart::kUpload, fbt, (size_t)P.bins16 * (size_t)P.mels16 * sizeof(float)}},
                  [&](const pdmp3_mel_desc* dk, int nk, int k, uint8_t* const* part) {
                    return pdmp3_launch_clip_mel(hs->s[slot].stream, dk, nk, as_floats(part[1]), as_floats(part[2]), reinterpret_cast<unsigned*>(part[0]) + k, &P);
                  });
}
// ---- the short-time Fourier transform (stft.hip) ----
extern "C" int pdmp3_hip_clip_stft(pdmp3_hip_stream* hs, int slot, const pdmp3_mel_desc* descs, int n_clips, const float* table,
                                   const pdmp3_stft_params* params) {
  if (!SLOT_OK(hs, slot) || n_clips < 0 || (n_clips && !descs) || !table || !params)
    return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_stft: bad argument", hipSuccess);
  const pdmp3_stft_params& P = *params;
  // what the kernel's indexing relies on
  if (P.n_fft < 16 || P.n_fft > 1024 || (P.n_fft & 1) || P.rows != ((P.n_fft + 3) & ~3) || P.hop < 1 || P.hop > P.n_fft || P.row_pad < 0 ||
      P.bins != P.n_fft / 2 + 1 || P.bins16 != ((P.bins + 15) & ~15) || (P.tile != 16 && P.tile != 32) || (P.channels != 1 && P.channels != 2) ||
      P.out_mode < 0 || P.out_mode > 4 || P.n_frames < 0 || P.n_in < 0 || (P.out_mode >= 3 && !(P.floor > 0.0f)) || (P.span_floats & 3u) ||
      P.lds_bytes > PDMP3_MEL_LDS_MAX)
    return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_stft: bad parameters", hipSuccess);
  {
    const size_t span = (size_t)(P.tile - 1) * P.hop + P.rows, chunks = (span + P.hop - 1) / P.hop;
    const size_t stage = (size_t)4 * (P.out_mode == 0 ? 2 : 1) * 16 * (size_t)(P.tile + 4);
    if (P.span_floats < chunks * (size_t)(P.hop + P.row_pad) || (size_t)P.lds_bytes < ((size_t)P.span_floats + stage) * sizeof(float))
      return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_stft: a tile's span and staging tiles do not fit the LDS asked for", hipSuccess);
    if (((long long)P.n_frames + P.tile - 1) / P.tile * P.channels > 0x7fffffffLL)
      return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_stft: too many frames", hipSuccess);
  }
  // descriptors | folded table
  return clip_run(hs, slot, "pdmp3_hip_clip_stft", descs, n_clips, P.n_frames,
                  {{ClipPart::kUpload, table, (size_t)P.rows * 2 * (size_t)P.bins16 * sizeof(float)}},
                  [&](const pdmp3_mel_desc* dk, int nk, int, uint8_t* const* part) {
                    return pdmp3_launch_clip_stft(hs->s[slot].stream, dk, nk, as_floats(part[0]), &P);
                  });
}
// ---- the constant-Q transform (cqt.hip) ----
// k_clip_cqt, or with `chroma` k_clip_chroma, whose LDS holds `extra_floats` more behind the partial sums (chroma.hip)
static int clip_cqt_run(pdmp3_hip_stream* hs, int slot, const pdmp3_mel_desc* descs, int n_clips, const float* table, size_t table_rows,
                        const pdmp3_cqt_params* params, const pdmp3_chroma_params* chroma, size_t extra_floats) {
  if (!SLOT_OK(hs, slot) || n_clips < 0 || (n_clips && !descs) || !table || !params)
    return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_cqt: bad argument", hipSuccess);
  const pdmp3_cqt_params& P = *params;
  // what the kernel's indexing relies on
  if (P.n_bins < 1 || P.n_bins > 16 * PDMP3_CQT_MAX_TILES || P.n_tiles != (P.n_bins + 15) / 16 || P.n_split < 0 || P.n_split > P.n_tiles ||
      P.hop < 1 || P.row_pad < 0 || (P.tile != 16 && P.tile != 8 && P.tile != 4) || (P.channels != 1 && P.channels != 2) || P.out_mode < 0 ||
      P.out_mode > 4 || P.n_frames < 0 || P.n_in < 0 || (P.out_mode >= 3 && !(P.floor > 0.0f)) || (P.span_floats & 3u) ||
      P.lds_bytes > PDMP3_MEL_LDS_MAX || P.rows0 < 4 || P.rows0 != P.tile_rows[0] || P.rows0 != ((2 * P.half0 + 4) & ~3) || table_rows > (size_t)1 << 24)
    return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_cqt: bad parameters", hipSuccess);
  for (int t = 0; t < P.n_tiles; t++) {
    // a tile's rows lie inside the table, and what they multiply inside a frame's span but for up to three rows of padding
    if (P.tile_rows[t] < 4 || (P.tile_rows[t] & 3) || (size_t)P.tile_at[t] + (size_t)P.tile_rows[t] > table_rows || P.tile_base[t] < 0 ||
        P.tile_base[t] + P.tile_rows[t] > P.rows0 + 3)
      return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_cqt: a tile of the table lies outside it or outside the span", hipSuccess);
  }
  {
    const size_t span = (size_t)(P.tile - 1) * P.hop + P.rows0, chunks = (span + P.hop - 1) / P.hop;
    if (P.span_floats < chunks * (size_t)(P.hop + P.row_pad) ||
        (size_t)P.lds_bytes < ((size_t)P.span_floats + PDMP3_CQT_PART_FLOATS + extra_floats) * sizeof(float))
      return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_cqt: a tile's span and partial sums do not fit the LDS asked for", hipSuccess);
    if (((long long)P.n_frames + P.tile - 1) / P.tile * P.channels > 0x7fffffffLL)
      return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_cqt: too many frames", hipSuccess);
  }
  // descriptors | table
  return clip_run(hs, slot, "pdmp3_hip_clip_cqt", descs, n_clips, P.n_frames, {{ClipPart::kUpload, table, table_rows * 32 * sizeof(float)}},
                  [&](const pdmp3_mel_desc* dk, int nk, int, uint8_t* const* part) {
                    return chroma ? pdmp3_launch_clip_chroma(hs->s[slot].stream, dk, nk, as_floats(part[0]), chroma)
                                  : pdmp3_launch_clip_cqt(hs->s[slot].stream, dk, nk, as_floats(part[0]), &P);
                  });
}
extern "C" int pdmp3_hip_clip_cqt(pdmp3_hip_stream* hs, int slot, const pdmp3_mel_desc* descs, int n_clips, const float* table, size_t table_rows,
                                  const pdmp3_cqt_params* params) {
  return clip_cqt_run(hs, slot, descs, n_clips, table, table_rows, params, nullptr, 0);
}
// ---- chroma features (chroma.hip): the constant-Q transform's launch with the fold's parameters checked in front of it ----
extern "C" int pdmp3_hip_clip_chroma(pdmp3_hip_stream* hs, int slot, const pdmp3_mel_desc* descs, int n_clips, const float* table, size_t table_rows,
                                     const pdmp3_chroma_params* params) {
  if (!params) return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_chroma: bad argument", hipSuccess);
  const pdmp3_chroma_params& S = *params;
  const pdmp3_cqt_params& P = S.cqt;
  // what the fold's indexing relies on: the planes inside the LDS asked for, the class plane inside the partial sums
  if (P.n_tiles < 1 || P.n_tiles > PDMP3_CQT_MAX_TILES || (P.out_mode != 1 && P.out_mode != 2) || S.n_chroma < 1 || S.n_chroma > 96 || S.r < 1 ||
      S.r > 96 || S.base_class < 0 || S.base_class >= S.n_chroma || S.chroma_norm < 0 || S.chroma_norm > 3 ||
      (S.chroma_norm && !(S.norm_floor > 0.0f)) || S.class_at != P.span_floats || S.q_at != P.span_floats + PDMP3_CQT_PART_FLOATS ||
      (size_t)S.n_chroma * 17 > PDMP3_CQT_PART_FLOATS)
    return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_chroma: bad parameters", hipSuccess);
  return clip_cqt_run(hs, slot, descs, n_clips, table, table_rows, &P, &S, (size_t)P.n_tiles * 16 * 17);
}
// ---- the short-time Fourier transform at n_fft 2048 and 4096 (stft_long.hip) ----
extern "C" int pdmp3_hip_clip_stft_long(pdmp3_hip_stream* hs, int slot, const pdmp3_mel_desc* descs, int n_clips, const float* tables,
                                        const pdmp3_stft_long_params* params) {
  if (!SLOT_OK(hs, slot) || n_clips < 0 || (n_clips && !descs) || !tables || !params)
    return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_stft_long: bad argument", hipSuccess);
  const pdmp3_stft_long_params& P = *params;
  // what the kernel's indexing relies on
  if ((P.n_fft != 2048 && P.n_fft != 4096) || P.n2 != P.n_fft / 64 || P.hop < 1 || P.hop > P.n_fft || P.bins != P.n_fft / 2 + 1 ||
      (P.tile != 16 && P.tile != 8 && P.tile != 4) || (P.n2 == 32 && P.tile == 4) || (P.n2 == 64 && P.tile == 16) ||
      (P.channels != 1 && P.channels != 2) || P.out_mode < 0 || P.out_mode > 4 || P.n_frames < 0 || P.n_in < 0 ||
      (P.out_mode >= 3 && !(P.floor > 0.0f)) || (P.span_floats & 3u) || P.lds_bytes > PDMP3_MEL_LDS_MAX)
    return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_stft_long: bad parameters", hipSuccess);
  {
    const size_t span = (size_t)(P.tile - 1) * P.hop + P.n_fft;
    const size_t stage = (size_t)(P.out_mode == 0 ? 2 : 1) * 16 * (size_t)(P.n2 / 2) * (size_t)(P.tile + 1);
    const size_t z = (size_t)P.tile * P.n2 * 32;
    if (P.span_floats < span || P.span_floats < stage || (size_t)P.lds_bytes < ((size_t)P.span_floats + z) * sizeof(float))
      return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_stft_long: a tile's span, staging tile and Z do not fit the LDS asked for", hipSuccess);
    if (((long long)P.n_frames + P.tile - 1) / P.tile * 4 * P.channels > 0x7fffffffLL)
      return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_stft_long: too many frames", hipSuccess);
  }
  // descriptors | the four tables
  return clip_run(hs, slot, "pdmp3_hip_clip_stft_long", descs, n_clips, P.n_frames,
                  {{ClipPart::kUpload, tables, ((size_t)P.n_fft + 64 * 128 + 2 * (size_t)P.n2 * P.n2 + (size_t)P.n2 * 128) * sizeof(float)}},
                  [&](const pdmp3_mel_desc* dk, int nk, int, uint8_t* const* part) {
                    return pdmp3_launch_clip_stft_long(hs->s[slot].stream, dk, nk, as_floats(part[0]), &P);
                  });
}
// ---- log-mel features at n_fft 2048 and 4096 (mel_long.hip) ----
extern "C" int pdmp3_hip_clip_mel_long(pdmp3_hip_stream* hs, int slot, const pdmp3_mel_desc* descs, int n_clips, const float* tables,
                                       const float* operand, const pdmp3_mel_long_params* params) {
  if (!SLOT_OK(hs, slot) || n_clips < 0 || (n_clips && !descs) || !tables || !operand || !params)
    return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_mel_long: bad argument", hipSuccess);
  const pdmp3_mel_long_params& P = *params;
  // what the kernel's indexing relies on
  if ((P.n_fft != 2048 && P.n_fft != 4096) || P.n2 != P.n_fft / 64 || P.hop < 1 || P.hop > P.n_fft || P.n_mels < 1 || P.n_mels > 256 ||
      P.mels16 != ((P.n_mels + 15) & ~15) || (P.tile != 16 && P.tile != 8 && P.tile != 4) || (P.n2 == 32 && P.tile == 4) ||
      (P.n2 == 64 && P.tile == 16) || (P.channels != 1 && P.channels != 2) || P.out_mode < 0 || P.out_mode > 2 || P.n_frames < 0 || P.n_in < 0 ||
      !(P.floor > 0.0f) || (P.span_floats & 3u) || P.lds_bytes > PDMP3_MEL_LDS_MAX)
    return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_mel_long: bad parameters", hipSuccess);
  {
    const size_t span = (size_t)(P.tile - 1) * P.hop + P.n_fft;
    const size_t z = (size_t)P.tile * P.n2 * 32, pw = (size_t)P.tile * (8 * (size_t)P.n2 + 2);
    if (P.span_floats < span || (size_t)P.lds_bytes < ((size_t)P.span_floats + z + pw) * sizeof(float))
      return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_mel_long: a tile's span, Z and powers do not fit the LDS asked for", hipSuccess);
    if (((long long)P.n_frames + P.tile - 1) / P.tile * P.channels > 0x7fffffffLL)
      return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_mel_long: too many frames", hipSuccess);
  }
  // descriptors | the four tables | the filterbank operand
  return clip_run(hs, slot, "pdmp3_hip_clip_mel_long", descs, n_clips, P.n_frames,
                  {{ClipPart::kUpload, tables, ((size_t)P.n_fft + 64 * 128 + 2 * (size_t)P.n2 * P.n2 + (size_t)P.n2 * 128) * sizeof(float)},
                   {ClipPart::kUpload, operand, (size_t)(P.n_fft / 2) * (size_t)P.mels16 * sizeof(float)}},
                  [&](const pdmp3_mel_desc* dk, int nk, int, uint8_t* const* part) {
                    return pdmp3_launch_clip_mel_long(hs->s[slot].stream, dk, nk, as_floats(part[0]), as_floats(part[1]), &P);
                  });
}
// ---- spectral descriptors at n_fft 2048 and 4096 (spectral.hip) ----
extern "C" int pdmp3_hip_clip_spectral(pdmp3_hip_stream* hs, int slot, const pdmp3_mel_desc* descs, int n_clips, const float* tables,
                                       const pdmp3_spectral_params* params) {
  if (!SLOT_OK(hs, slot) || n_clips < 0 || (n_clips && !descs) || !tables || !params)
    return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_spectral: bad argument", hipSuccess);
  const pdmp3_spectral_params& P = *params;
  // what the kernel's indexing relies on: one of its two (n2, tile) paths, and the four regions inside the LDS asked for
  if ((P.n_fft != 2048 && P.n_fft != 4096) || P.n2 != P.n_fft / 64 || P.hop < 1 || P.hop > P.n_fft || P.tile != (P.n2 == 32 ? 8 : 4) ||
      (P.channels != 1 && P.channels != 2) || P.n_frames < 0 || P.n_in < 0 || !(P.bin_hz > 0.0) || !(P.roll_percent > 0.0 && P.roll_percent < 1.0) ||
      !(P.amin > 0.0f) || !(P.zcr_threshold >= 0.0f) || (P.span_floats & 3u) || P.lds_bytes > PDMP3_MEL_LDS_MAX)
    return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_spectral: bad parameters", hipSuccess);
  {
    const size_t span = (size_t)(P.tile - 1) * P.hop + P.n_fft;
    const size_t z = (size_t)P.tile * P.n2 * 32, plane = (size_t)P.tile * (size_t)(P.n_fft / 2 + 1), res = (size_t)8 * P.tile;
    if (P.span_floats < span || (size_t)P.lds_bytes < ((size_t)P.span_floats + z + plane + res) * sizeof(float))
      return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_spectral: a tile's span, Z, plane and results do not fit the LDS asked for", hipSuccess);
    if (((long long)P.n_frames + P.tile - 1) / P.tile * P.channels > 0x7fffffffLL)
      return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_spectral: too many frames", hipSuccess);
  }
  // descriptors | the four tables
  return clip_run(hs, slot, "pdmp3_hip_clip_spectral", descs, n_clips, P.n_frames,
                  {{ClipPart::kUpload, tables, ((size_t)P.n_fft + 64 * 128 + 2 * (size_t)P.n2 * P.n2 + (size_t)P.n2 * 128) * sizeof(float)}},
                  [&](const pdmp3_mel_desc* dk, int nk, int, uint8_t* const* part) {
                    return pdmp3_launch_clip_spectral(hs->s[slot].stream, dk, nk, as_floats(part[0]), &P);
                  });
}
// ---- harmonic-percussive separation (hpss.hip) ----
extern "C" int pdmp3_hip_clip_hpss(pdmp3_hip_stream* hs, int slot, const pdmp3_mel_desc* descs, int n_clips, const pdmp3_hpss_params* params) {
  if (!SLOT_OK(hs, slot) || n_clips < 0 || (n_clips && !descs) || !params)
    return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_hpss: bad argument", hipSuccess);
  const pdmp3_hpss_params& P = *params;
  const auto kernel_ok = [](int l) { return l >= 3 && l <= pdmp3::kHpssMaxKernel && (l & 1); };
  // what the kernel's indexing relies on: the one tile and layout of hpss_core.h, the stage's frames, rows inside 31 bits
  if ((P.n_fft != 2048 && P.n_fft != 4096) || P.bins != P.n_fft / 2 + 1 || !kernel_ok(P.kernel_harm) || !kernel_ok(P.kernel_perc) || P.n_frames < 0 ||
      P.n_stage != (long long)P.n_frames + P.kernel_harm - 1 || (P.channels != 1 && P.channels != 2) || P.out_mode < 0 || P.out_mode > 3 ||
      (P.power != 0 && P.power != 1 && P.power != 2) || !(P.margin_harm >= 1.0 && P.margin_harm <= 1.7976931348623157e308) ||
      !(P.margin_perc >= 1.0 && P.margin_perc <= 1.7976931348623157e308))
    return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_hpss: bad parameters", hipSuccess);
  if (P.tile_bins != pdmp3::kHpssBins || P.tile_frames != pdmp3::kHpssFrames || P.pitch != pdmp3::kHpssPitch ||
      P.lds_bytes != pdmp3::kHpssLdsFloats * sizeof(float) || P.lds_bytes > PDMP3_MEL_LDS_MAX)
    return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_hpss: not the plan's tile, pitch and LDS", hipSuccess);
  {
    const long long e = P.out_mode == 2 ? 2 : 1, tiles = ((long long)P.n_frames + pdmp3::kHpssFrames - 1) / pdmp3::kHpssFrames;
    if (e * P.bins * (long long)P.n_stage > 0x7fffffffLL || 2 * e * P.bins * (long long)P.n_frames > 0x7fffffffLL ||
        tiles * pdmp3::hpss_bin_tiles(P.bins) * P.channels > 0x7fffffffLL)
      return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_hpss: too many frames", hipSuccess);
  }
  // descriptors alone: the kernel reads no table
  return clip_run(hs, slot, "pdmp3_hip_clip_hpss", descs, n_clips, P.n_frames, {{ClipPart::kScratch, nullptr, 0}},
                  [&](const pdmp3_mel_desc* dk, int nk, int, uint8_t* const*) { return pdmp3_launch_clip_hpss(hs->s[slot].stream, dk, nk, &P); });
}
// ---- MFCC, deltas and dB mel at n_fft 2048 and 4096 (mfcc_long.hip) ----
extern "C" int pdmp3_hip_clip_mfcc_long(pdmp3_hip_stream* hs, int slot, const pdmp3_mel_desc* descs, int n_clips, const float* dct,
                                        const pdmp3_mfcc_long_params* params) {
  if (!SLOT_OK(hs, slot) || n_clips < 0 || (n_clips && !descs) || !params)
    return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_mfcc_long: bad argument", hipSuccess);
  const pdmp3_mfcc_long_params& P = *params;
  // what the kernels' indexing relies on: the bands, the stage's frames, rows inside 31 bits
  if (P.n_mels < 1 || P.n_mels > 256 || P.mels16 != ((P.n_mels + 15) & ~15) || P.n_frames < 0 || (P.channels != 1 && P.channels != 2) ||
      (P.out_mode != 0 && P.out_mode != 1) || (P.use_top != 0 && P.use_top != 1) || (P.use_top && !(P.top_db >= 0.0f)) ||
      P.halo < 0 || P.halo > pdmp3::kMfccLongMaxHalo || P.n_stage != (long long)P.n_frames + 2 * P.halo ||
      (long long)P.n_mels * P.n_stage > 0x7fffffffLL)
    return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_mfcc_long: bad parameters", hipSuccess);
  size_t dct_bytes = 0;
  if (P.out_mode == 1) {
    if (P.halo != 0) return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_mfcc_long: the dB mode has no halo", hipSuccess);
  } else {
    if ((n_clips && !dct) || P.n_mfcc < 1 || P.n_mfcc > P.n_mels || P.n_mfcc > 128 || P.ceps16 != ((P.n_mfcc + 15) & ~15) || P.deltas < 0 ||
        P.deltas > 2 || (P.deltas == 0) != (P.halo == 0) || (long long)(1 + P.deltas) * P.n_mfcc * P.n_frames > 0x7fffffffLL)
      return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_mfcc_long: bad parameters", hipSuccess);
    if (P.tile != pdmp3::kMfccLongFrames || P.d_pitch != pdmp3::kMfccLongDPitch || P.c_pitch != pdmp3::kMfccLongCPitch ||
        P.lds_bytes != pdmp3::mfcc_long_lds_floats(P.mels16, P.ceps16) * sizeof(float) || P.lds_bytes > PDMP3_MEL_LDS_MAX)
      return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_mfcc_long: not the plan's tile, pitches and LDS", hipSuccess);
    dct_bytes = (size_t)P.ceps16 * (size_t)P.mels16 * sizeof(float);
  }
  return clip_run(hs, slot, "pdmp3_hip_clip_mfcc_long", descs, n_clips, P.n_frames, {{ClipPart::kUpload, dct, dct_bytes}},
                  [&](const pdmp3_mel_desc* dk, int nk, int, uint8_t* const* part) {
                    return pdmp3_launch_clip_mfcc_long(hs->s[slot].stream, dk, nk, as_floats(part[0]), &P);
                  });
}
// ---- Kaldi-style filterbank features (fbank.hip) ----
extern "C" int pdmp3_hip_clip_fbank(pdmp3_hip_stream* hs, int slot, const pdmp3_fbank_desc* descs, int n_clips, const float* dft, const float* fbt,
                                    const pdmp3_fbank_params* params) {
  if (!SLOT_OK(hs, slot) || n_clips < 0 || (n_clips && !descs) || !dft || !fbt || !params)
    return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_fbank: bad argument", hipSuccess);
  const pdmp3_fbank_params& P = *params;
  // what the kernel's indexing relies on
  if (P.win < 2 || P.win > 1024 || P.rows != ((P.win + 3) & ~3) || P.n_dft < P.win || P.n_dft > 1024 || (P.n_dft & 1) || P.hop < 1 || P.hop > P.win ||
      P.row_pad < 0 || P.bins16 != ((P.n_dft / 2 + 15) & ~15) || P.n_mels < 1 || P.n_mels > 256 || P.mels16 != ((P.n_mels + 15) & ~15) ||
      (P.tile != 16 && P.tile != 32) || (P.channels != 1 && P.channels != 2) || P.out_mode < 0 || P.out_mode > 1 || P.n_frames < 0 || P.n_in < 0 ||
      (P.use_energy & ~1) || (P.htk_compat & ~1) || (P.subtract_mean & ~1) || (P.remove_dc & ~1) || !(P.eps > 0.0f) || !(P.scale > 0.0f) ||
      P.lds_bytes > PDMP3_MEL_LDS_MAX)
    return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_fbank: bad parameters", hipSuccess);
  const size_t tiles = ((size_t)P.n_frames + P.tile - 1) / P.tile, D = (size_t)(P.n_mels + P.use_energy);
  {
    const size_t span = (size_t)(P.tile - 1) * P.hop + P.rows, chunks = (span + P.hop - 1) / P.hop;
    const size_t first = chunks * (size_t)(P.hop + P.row_pad), mt = (size_t)P.mels16 * (P.tile + 1);
    if (P.span_floats < first || P.span_floats < mt || (size_t)P.lds_bytes < ((size_t)P.span_floats + (size_t)P.tile * (P.bins16 + 2)) * sizeof(float))
      return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_fbank: a tile's span, powers and mel tile do not fit the LDS asked for", hipSuccess);
    if (tiles * P.channels > 0x7fffffffULL)
      return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_fbank: too many frames", hipSuccess);
  }
  for (int k = 0; k < n_clips; k++)
    if ((long long)descs[k].valid > (long long)P.n_frames) return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_fbank: a clip's valid frames exceed its frames", hipSuccess);
  // descriptors | folded table | filterbank | (subtract_mean) column sums [clip][channel][tile][D]
  const size_t clip_sums = (size_t)P.channels * tiles * D;               // (floats)
  return clip_run(hs, slot, "pdmp3_hip_clip_fbank", descs, n_clips, P.n_frames,
                  {{ClipPart::kUpload, dft, (size_t)P.rows * 2 * (size_t)P.bins16 * sizeof(float)},
                   {ClipPart::kUpload, fbt, (size_t)P.bins16 * (size_t)P.mels16 * sizeof(float)},
                   {ClipPart::kScratch, nullptr, P.subtract_mean ? (size_t)n_clips * clip_sums * sizeof(float) : 0}},
                  [&](const pdmp3_fbank_desc* dk, int nk, int k, uint8_t* const* part) {
                    float* const sums = reinterpret_cast<float*>(part[2]);
                    return pdmp3_launch_clip_fbank(hs->s[slot].stream, dk, nk, as_floats(part[0]), as_floats(part[1]),
                                                   P.subtract_mean ? sums + (size_t)k * clip_sums : sums, &P);
                  });
}
// ---- Kaldi-style MFCC features (mfcc.hip) ----
extern "C" int pdmp3_hip_clip_mfcc(pdmp3_hip_stream* hs, int slot, const pdmp3_fbank_desc* descs, int n_clips, const float* dft, const float* fbt,
                                   const float* dct, const pdmp3_mfcc_params* params) {
  if (!SLOT_OK(hs, slot) || n_clips < 0 || (n_clips && !descs) || !dft || !fbt || !dct || !params)
    return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_mfcc: bad argument", hipSuccess);
  const pdmp3_fbank_params& P = params->fb;
  // what the kernel's indexing relies on
  if (P.win < 2 || P.win > 1024 || P.rows != ((P.win + 3) & ~3) || P.n_dft < P.win || P.n_dft > 1024 || (P.n_dft & 1) || P.hop < 1 || P.hop > P.win ||
      P.row_pad < 0 || P.bins16 != ((P.n_dft / 2 + 15) & ~15) || P.n_mels < 1 || P.n_mels > 256 || P.mels16 != ((P.n_mels + 15) & ~15) ||
      (P.tile != 16 && P.tile != 32) || (P.channels != 1 && P.channels != 2) || P.out_mode != 1 || P.n_frames < 0 || P.n_in < 0 ||
      (P.use_energy & ~1) || (P.htk_compat & ~1) || (P.subtract_mean & ~1) || (P.remove_dc & ~1) || !(P.eps > 0.0f) || !(P.scale > 0.0f) ||
      P.lds_bytes > PDMP3_MEL_LDS_MAX || params->n_ceps < 1 || params->n_ceps > P.n_mels || params->ceps16 != ((params->n_ceps + 15) & ~15))
    return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_mfcc: bad parameters", hipSuccess);
  const size_t tiles = ((size_t)P.n_frames + P.tile - 1) / P.tile, D = (size_t)params->n_ceps;
  {
    const size_t span = (size_t)(P.tile - 1) * P.hop + P.rows, chunks = (span + P.hop - 1) / P.hop;
    const size_t first = chunks * (size_t)(P.hop + P.row_pad), mt = (size_t)P.mels16 * (P.tile + 1);
    const size_t pw = (size_t)P.tile * (P.bins16 + 2), ct = (size_t)P.tile * (params->ceps16 + 1);
    if (P.span_floats < first || P.span_floats < mt || (size_t)P.lds_bytes < ((size_t)P.span_floats + (pw > ct ? pw : ct)) * sizeof(float))
      return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_mfcc: a tile's span, powers, mel tile and cepstra do not fit the LDS asked for", hipSuccess);
    if (tiles * P.channels > 0x7fffffffULL)
      return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_mfcc: too many frames", hipSuccess);
  }
  for (int k = 0; k < n_clips; k++)
    if ((long long)descs[k].valid > (long long)P.n_frames) return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_mfcc: a clip's valid frames exceed its frames", hipSuccess);
  // descriptors | folded table | filterbank | folded DCT table | (subtract_mean) column sums [clip][channel][tile][n_ceps]
  const size_t clip_sums = (size_t)P.channels * tiles * D;               // (floats)
  return clip_run(hs, slot, "pdmp3_hip_clip_mfcc", descs, n_clips, P.n_frames,
                  {{ClipPart::kUpload, dft, (size_t)P.rows * 2 * (size_t)P.bins16 * sizeof(float)},
                   {ClipPart::kUpload, fbt, (size_t)P.bins16 * (size_t)P.mels16 * sizeof(float)},
                   {ClipPart::kUpload, dct, (size_t)P.mels16 * (size_t)params->ceps16 * sizeof(float)},
                   {ClipPart::kScratch, nullptr, P.subtract_mean ? (size_t)n_clips * clip_sums * sizeof(float) : 0}},
                  [&](const pdmp3_fbank_desc* dk, int nk, int k, uint8_t* const* part) {
                    float* const sums = reinterpret_cast<float*>(part[3]);
                    return pdmp3_launch_clip_mfcc(hs->s[slot].stream, dk, nk, as_floats(part[0]), as_floats(part[1]), as_floats(part[2]),
                                                  P.subtract_mean ? sums + (size_t)k * clip_sums : sums, params);
                  });
}
// ---- loudness (loudness.hip) ----
extern "C" int pdmp3_hip_clip_loudness(pdmp3_hip_stream* hs, int slot, const pdmp3_mel_desc* descs, int n_clips, const pdmp3_loud_tables* tables,
                                       const uint64_t* stats_dst, const uint64_t* mom_dst, const pdmp3_loud_params* params) {
  if (!SLOT_OK(hs, slot) || n_clips < 0 || (n_clips && (!descs || !stats_dst || !mom_dst)) || !tables || !params)
    return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_loudness: bad argument", hipSuccess);
  const pdmp3_loud_params& P = *params;
  // what the kernels' indexing relies on
  if (P.n_in < 0 || P.n_in > 0x7fffffffLL || (P.channels != 1 && P.channels != 2) || P.q < 800 || P.q > 19200 ||
      P.n_chunks != (P.n_in + PDMP3_LOUD_B * PDMP3_LOUD_CHUNK - 1) / (PDMP3_LOUD_B * PDMP3_LOUD_CHUNK) || P.n_sub != P.n_in / P.q ||
      P.n_mom != (P.n_sub > 3 ? P.n_sub - 3 : 0) || (P.dual_mono != 0 && (P.dual_mono != 1 || P.channels != 1)) || !(P.peak_limit >= 0.0))
    return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_loudness: bad parameters", hipSuccess);
  for (int k = 0; k < n_clips; k++)
    if (!descs[k].src || !descs[k].dst || (descs[k].src & 15u) || (descs[k].src_chan_stride & 3u) || !stats_dst[k] ||
        (P.channels == 2 && (descs[k].src_chan_stride < (uint64_t)P.n_in || descs[k].dst_chan_stride < (uint64_t)P.n_in)))
      return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_loudness: a clip's rows are not where the kernels can take them", hipSuccess);
  // descriptors | tables | destinations of stats, of momentary | states | chunk starts | partial sums | sub-block sums | gains
  const size_t rows = (size_t)n_clips * (size_t)P.channels, chunks = rows * (size_t)P.n_chunks;
  return clip_run(hs, slot, "pdmp3_hip_clip_loudness", descs, n_clips, P.n_in,
                  {{ClipPart::kUpload, tables, sizeof *tables},
                   {ClipPart::kUpload, stats_dst, (size_t)n_clips * sizeof(uint64_t)},
                   {ClipPart::kUpload, mom_dst, (size_t)n_clips * sizeof(uint64_t)},
                   {ClipPart::kScratch, nullptr, chunks * PDMP3_LOUD_CHUNK * 4 * sizeof(double)},
                   {ClipPart::kScratch, nullptr, chunks * 4 * sizeof(double)},
                   {ClipPart::kScratch, nullptr, chunks * 16 * sizeof(float)},
                   {ClipPart::kScratch, nullptr, rows * (size_t)P.n_sub * sizeof(float)},
                   {ClipPart::kScratch, nullptr, (size_t)n_clips * sizeof(float)}},
                  [&](const pdmp3_mel_desc* dk, int nk, int k, uint8_t* const* part) {
                    return pdmp3_launch_clip_loudness(hs->s[slot].stream, dk, nk, k, reinterpret_cast<const pdmp3_loud_tables*>(part[0]),
                                                      reinterpret_cast<const uint64_t*>(part[1]), reinterpret_cast<const uint64_t*>(part[2]),
                                                      reinterpret_cast<double*>(part[3]), reinterpret_cast<double*>(part[4]),
                                                      reinterpret_cast<float*>(part[5]), reinterpret_cast<float*>(part[6]),
                                                      reinterpret_cast<float*>(part[7]), &P);
                  });
}
// ---- true peak, short-term loudness and loudness range (loudness.hip, the second instantiations) ----
extern "C" int pdmp3_hip_clip_r128(pdmp3_hip_stream* hs, int slot, const pdmp3_mel_desc* descs, int n_clips, const pdmp3_loud_tables* tables,
                                   const float* taps, const uint64_t* stats_dst, const uint64_t* mom_dst, const uint64_t* st_dst,
                                   const pdmp3_r128_params* params) {
  if (!SLOT_OK(hs, slot) || n_clips < 0 || (n_clips && (!descs || !stats_dst || !mom_dst || !st_dst)) || !tables || !taps || !params)
    return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_r128: bad argument", hipSuccess);
  const pdmp3_loud_params& P = params->loud;
  // what the kernels' indexing relies on
  const int n_st = P.n_sub > 29 ? P.n_sub - 29 : 0;
  if (P.n_in < 0 || P.n_in > 0x7fffffffLL || (P.channels != 1 && P.channels != 2) || P.q < 800 || P.q > 19200 ||
      P.n_chunks != (P.n_in + PDMP3_LOUD_B * PDMP3_LOUD_CHUNK - 1) / (PDMP3_LOUD_B * PDMP3_LOUD_CHUNK) || P.n_sub != P.n_in / P.q ||
      P.n_mom != (P.n_sub > 3 ? P.n_sub - 3 : 0) || (P.dual_mono != 0 && (P.dual_mono != 1 || P.channels != 1)) || !(P.peak_limit >= 0.0) ||
      params->n_st != n_st || params->n_rng != (n_st + 9) / 10 || params->n_rng > PDMP3_R128_MAX_RANGE || (params->limit_true_peak & ~1))
    return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_r128: bad parameters", hipSuccess);
  for (int k = 0; k < n_clips; k++)
    if (!descs[k].src || !descs[k].dst || (descs[k].src & 15u) || (descs[k].src_chan_stride & 3u) || !stats_dst[k] ||
        (P.channels == 2 && (descs[k].src_chan_stride < (uint64_t)P.n_in || descs[k].dst_chan_stride < (uint64_t)P.n_in)))
      return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_r128: a clip's rows are not where the kernels can take them", hipSuccess);
  // descriptors | tables | taps | destinations of stats, of momentary, of short-term | states | chunk starts | partial results
  // (8 floats a wave) | sub-block sums | gains
  const size_t rows = (size_t)n_clips * (size_t)P.channels, chunks = rows * (size_t)P.n_chunks;
  return clip_run(hs, slot, "pdmp3_hip_clip_r128", descs, n_clips, P.n_in,
                  {{ClipPart::kUpload, tables, sizeof *tables},
                   {ClipPart::kUpload, taps, 3 * PDMP3_R128_TAPS * sizeof(float)},
                   {ClipPart::kUpload, stats_dst, (size_t)n_clips * sizeof(uint64_t)},
                   {ClipPart::kUpload, mom_dst, (size_t)n_clips * sizeof(uint64_t)},
                   {ClipPart::kUpload, st_dst, (size_t)n_clips * sizeof(uint64_t)},
                   {ClipPart::kScratch, nullptr, chunks * PDMP3_LOUD_CHUNK * 4 * sizeof(double)},
                   {ClipPart::kScratch, nullptr, chunks * 4 * sizeof(double)},
                   {ClipPart::kScratch, nullptr, chunks * 32 * sizeof(float)},
                   {ClipPart::kScratch, nullptr, rows * (size_t)P.n_sub * sizeof(float)},
                   {ClipPart::kScratch, nullptr, (size_t)n_clips * sizeof(float)}},
                  [&](const pdmp3_mel_desc* dk, int nk, int k, uint8_t* const* part) {
                    return pdmp3_launch_clip_r128(hs->s[slot].stream, dk, nk, k, reinterpret_cast<const pdmp3_loud_tables*>(part[0]), as_floats(part[1]),
                                                  reinterpret_cast<const uint64_t*>(part[2]), reinterpret_cast<const uint64_t*>(part[3]),
                                                  reinterpret_cast<const uint64_t*>(part[4]), reinterpret_cast<double*>(part[5]),
                                                  reinterpret_cast<double*>(part[6]), reinterpret_cast<float*>(part[7]),
                                                  reinterpret_cast<float*>(part[8]), reinterpret_cast<float*>(part[9]), params);
                  });
}
// ---- pitch (pitch.hip) ----
extern "C" int pdmp3_hip_clip_pitch(pdmp3_hip_stream* hs, int slot, const pdmp3_mel_desc* descs, int n_clips, const pdmp3_pitch_params* params) {
  if (!SLOT_OK(hs, slot) || n_clips < 0 || (n_clips && !descs) || !params)
    return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_pitch: bad argument", hipSuccess);
  const pdmp3_pitch_params& P = *params;
  // what the kernel's indexing relies on
  if (P.n < 64 || P.n > 2048 || (P.n & 1) || P.win < 4 || P.win > P.n - 2 || P.hop < 1 || P.hop > P.n || P.tmin < 1 || P.tmin >= P.tmax ||
      P.tmax > P.n - P.win - 1 || P.tiles != (P.tmax + 256) / 256 || P.tiles > 8 || P.ksteps != (P.win + 18) / 4 ||
      (P.frames_wg != 1 && P.frames_wg != 2 && P.frames_wg != 4 && P.frames_wg != 8) || (P.channels != 1 && P.channels != 2) ||
      (P.out_mode != 0 && P.out_mode != 1) || P.n_frames < 0 || P.n_in < 0 || !(P.sr > 0.0) || !(P.threshold > 0.0) || (P.span_floats & 3u) ||
      P.lds_bytes > PDMP3_MEL_LDS_MAX)
    return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_pitch: bad parameters", hipSuccess);
  {
    // (the A operand of the k-step behind the last, which the kernel reads ahead: row 15 of the last tile)
    const size_t reach = (size_t)4 * (P.ksteps + 1) + 240 + (size_t)256 * (P.tiles - 1), first = (size_t)(P.frames_wg - 1) * P.hop;
    const size_t ext = pdmp3::kPitchFront + first + (reach > (size_t)P.n ? reach : (size_t)P.n);
    if (P.q_doubles != first + P.n + 1 || P.ext < ext || P.ext > 0x100000u || P.span_floats < pdmp3::pitch_at(P.ext) ||
        (size_t)P.lds_bytes < (size_t)pdmp3::pitch_lds(P).total_f * sizeof(float))
      return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_pitch: a workgroup's span, sums and curves do not fit the LDS asked for", hipSuccess);
    if (((long long)P.n_frames + P.frames_wg - 1) / P.frames_wg * P.channels > 0x7fffffffLL)
      return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_pitch: too many frames", hipSuccess);
  }
  // descriptors alone: the kernel reads no table
  return clip_run(hs, slot, "pdmp3_hip_clip_pitch", descs, n_clips, P.n_frames, {{ClipPart::kScratch, nullptr, 0}},
                  [&](const pdmp3_mel_desc* dk, int nk, int, uint8_t* const*) { return pdmp3_launch_clip_pitch(hs->s[slot].stream, dk, nk, &P); });
}
// ---- pYIN (pyin.hip) ----
extern "C" int pdmp3_hip_clip_pyin(pdmp3_hip_stream* hs, int slot, const pdmp3_pyin_desc* descs, int n_clips, const double* tables,
                                   const pdmp3_pyin_params* params) {
  if (!SLOT_OK(hs, slot) || n_clips < 0 || (n_clips && !descs) || !tables || !params)
    return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_pyin: bad argument", hipSuccess);
  const pdmp3_pyin_params& P = *params;
  // what the kernels' indexing relies on
  if (P.tmin < 1 || P.tmin >= P.tmax || P.tmax > 2046 || P.n_thr < 1 || P.n_thr > 256 || P.n_bins < 2 || P.n_bins > 2048 || P.hb < 0 ||
      2 * P.hb > P.n_bins || P.max_troughs != (P.tmax - 1 - P.tmin) / 2 + 1 ||
      (P.frames_wg != 1 && P.frames_wg != 2 && P.frames_wg != 4 && P.frames_wg != 8) || (P.channels != 1 && P.channels != 2) ||
      (P.out_mode != 0 && P.out_mode != 1) || P.n_frames < 0 || (P.use_bin != 0 && P.use_bin != 1) ||
      (unsigned)P.path_threads != pdmp3::pyin_path_threads(P.n_bins) || P.obs_lds_bytes > PDMP3_MEL_LDS_SOFT || P.path_lds_bytes > PDMP3_MEL_LDS_MAX)
    return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_pyin: bad parameters", hipSuccess);
  if (P.obs_lds_bytes < pdmp3::pyin_obs_lds_bytes(P, P.frames_wg) || (size_t)P.path_lds_bytes < (size_t)pdmp3::pyin_path_lds(P).total_d * sizeof(double))
    return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_pyin: a workgroup's curves, rows and states do not fit the LDS asked for", hipSuccess);
  if (((long long)P.n_frames + P.frames_wg - 1) / P.frames_wg * P.channels > 0x7fffffffLL || (long long)P.n_frames * (P.n_bins + 1) > 0x7fffffffLL ||
      (long long)P.n_frames * (P.tmax + 1) > 0x7fffffffLL)
    return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_pyin: too many frames", hipSuccess);
  // descriptors | the tables
  return clip_run(hs, slot, "pdmp3_hip_clip_pyin", descs, n_clips, P.n_frames, {{ClipPart::kUpload, tables, pdmp3::pyin_table_bytes(P)}},
                  [&](const pdmp3_pyin_desc* dk, int nk, int, uint8_t* const* part) {
                    return pdmp3_launch_clip_pyin(hs->s[slot].stream, dk, nk, reinterpret_cast<const double*>(part[0]), &P);
                  });
}
// ---- onset strength, tempogram, tempo (tempogram.hip) ----
extern "C" int pdmp3_hip_clip_tempogram(pdmp3_hip_stream* hs, int slot, const pdmp3_tempogram_desc* descs, int n_clips, const float* window,
                                        const double* prior, const pdmp3_tempogram_params* params) {
  if (!SLOT_OK(hs, slot) || n_clips < 0 || (n_clips && !descs) || !window || !prior || !params)
    return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_tempogram: bad argument", hipSuccess);
  const pdmp3_tempogram_params& P = *params;
  // what the kernels' indexing relies on
  if (P.n_mels < 1 || P.n_mels > 256 || P.lag < 1 || P.lag > 16 || P.half < 0 || P.half > 4 || P.hop < 1 || P.win < 16 || P.win > pdmp3::kTempoMaxWin ||
      (P.win & 1) || P.tiles != (P.win + 255) / 256 || P.ksteps != (P.win + 18) / 4 ||
      (P.frames_wg != 1 && P.frames_wg != 2 && P.frames_wg != 4 && P.frames_wg != 8) || (P.channels != 1 && P.channels != 2) || P.out_mode < 0 ||
      P.out_mode > 2 || P.n_frames < 0 || P.n_env != (P.out_mode == 0 ? (long long)P.n_frames : (long long)P.n_frames + P.win - 1) ||
      P.n_mel_frames != (long long)P.n_env + P.lag || (long long)P.n_mels * P.n_mel_frames > 0x7fffffffLL ||
      (long long)P.win * P.n_frames > 0x7fffffffLL || (P.out_mode != 0 && P.env_stride < (unsigned)P.n_env) || !(P.sr > 0.0) || (P.span_floats & 3u) ||
      P.lds_bytes > PDMP3_MEL_LDS_MAX)
    return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_tempogram: bad parameters", hipSuccess);
  if (P.ext < pdmp3::tempogram_ext(P.win, P.tiles, P.ksteps) || P.ext > 0x10000u || P.span_floats < pdmp3::pitch_at(P.ext) ||
      (size_t)P.lds_bytes < (size_t)pdmp3::tempogram_lds(P).total_f * sizeof(float))
    return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_tempogram: a workgroup's spans and curves do not fit the LDS asked for", hipSuccess);
  if (((long long)P.n_env + pdmp3::kOnsetThreads - 1) / pdmp3::kOnsetThreads * P.channels > 0x7fffffffLL)
    return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_tempogram: too many frames", hipSuccess);
  // descriptors | the window | the prior
  return clip_run(hs, slot, "pdmp3_hip_clip_tempogram", descs, n_clips, P.n_frames,
                  {{ClipPart::kUpload, window, (size_t)P.win * sizeof(float)}, {ClipPart::kUpload, prior, (size_t)P.win * sizeof(double)}},
                  [&](const pdmp3_tempogram_desc* dk, int nk, int, uint8_t* const* part) {
                    return pdmp3_launch_clip_tempogram(hs->s[slot].stream, dk, nk, as_floats(part[0]), reinterpret_cast<const double*>(part[1]), &P);
                  });
}
// ---- beat tracking (beat.hip) ----
extern "C" int pdmp3_hip_clip_beat(pdmp3_hip_stream* hs, int slot, const pdmp3_beat_desc* descs, int n_clips, const double* tables, double* work,
                                   const pdmp3_beat_params* params) {
  if (!SLOT_OK(hs, slot) || n_clips < 0 || (n_clips && !descs) || !tables || !params || (n_clips && params->n_frames > 0 && !work))
    return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_beat: bad argument", hipSuccess);
  const pdmp3_beat_params& P = *params;
  // what the kernels' indexing relies on
  if (P.p_min < 1 || P.p_min > P.p_max || P.p_max > pdmp3::kBeatMaxPeriod || P.period < 0 || (P.period && (P.period != P.p_min || P.period != P.p_max)) ||
      P.n_frames < 0 || P.n_frames > pdmp3::kBeatMaxFrames || (P.channels != 1 && P.channels != 2) || P.out_mode < 0 || P.out_mode > 2 ||
      !(P.tightness > 0.0) || P.work_stride < pdmp3::beat_work_of(P.n_frames).total_d || P.score_lds_bytes > PDMP3_MEL_LDS_SOFT ||
      P.dp_lds_bytes > PDMP3_MEL_LDS_SOFT)
    return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_beat: bad parameters", hipSuccess);
  if ((size_t)P.score_lds_bytes < (size_t)pdmp3::beat_score_lds(P.p_max, P.n_frames).total_d * sizeof(double) ||
      (size_t)P.dp_lds_bytes < (size_t)pdmp3::beat_dp_lds(P.p_max).total_d * sizeof(double))
    return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_clip_beat: the tiles, the ring and the tables do not fit the LDS asked for", hipSuccess);
  // descriptors | the tables
  return clip_run(hs, slot, "pdmp3_hip_clip_beat", descs, n_clips, P.n_frames,
                  {{ClipPart::kUpload, tables, pdmp3::beat_table_doubles(P.p_min, P.p_max) * sizeof(double)}},
                  [&](const pdmp3_beat_desc* dk, int nk, int k, uint8_t* const* part) {
                    return pdmp3_launch_clip_beat(hs->s[slot].stream, dk, nk, k, reinterpret_cast<const double*>(part[0]), work, &P);
                  });
}
extern "C" int pdmp3_hip_copy_from_device(void* host_dst, const void* dev_src, size_t bytes) {
  if (!bytes) return PDMP3_HIP_OK;
  if (!host_dst || !dev_src) return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_copy_from_device: NULL", hipSuccess);
  HIP_TRY(hipMemcpy(host_dst, dev_src, bytes, hipMemcpyDeviceToHost), "copy from the device");
  return PDMP3_HIP_OK;
}

extern "C" int pdmp3_hip_stream_fetch_records(pdmp3_hip_stream* hs, int slot, int n_frames, int16_t* spectra, pdmp3_gc_side* side) {
  if (!SLOT_OK(hs, slot) || n_frames < 0 || n_frames > hs->max_frames || !spectra || !side)
    return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_stream_fetch_records: bad argument", hipSuccess);
  HIP_TRY(hipSetDevice(hs->ctx->device), "hipSetDevice");
  HIP_TRY(hipStreamSynchronize(hs->s[slot].stream), "stream sync");
  HIP_TRY(hipMemcpy(spectra, hs->s[slot].d_spectra, (size_t)n_frames * PDMP3_FRAME_SPECTRA_BYTES, hipMemcpyDeviceToHost), "D2H spectra");
  HIP_TRY(hipMemcpy(side, hs->s[slot].d_side, (size_t)n_frames * PDMP3_FRAME_SIDE_BYTES, hipMemcpyDeviceToHost), "D2H side");
  return PDMP3_HIP_OK;
}

extern "C" int pdmp3_hip_stream_decode(pdmp3_hip_stream* hs, int n_frames) {
  int rc = pdmp3_hip_stream_submit(hs, 0, n_frames);
  if (rc != PDMP3_HIP_OK) return rc;
  return pdmp3_hip_stream_wait(hs, 0);
}
