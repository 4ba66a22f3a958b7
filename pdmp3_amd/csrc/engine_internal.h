// engine_internal.h -- what the translation units of libpdmp3_hip.so share and the C-ABI (include/pdmp3_hip.h) does not
// show.  Host code only.
//   engine.hip      the kernels, the engine context, launch_decode (which kernel, which grid), the device Huffman stage's
//                   launches, the bare decode entry points
//   stream.hip      pdmp3_hip_stream: buffers, events and ordering of the slots' submits; names no kernel
//   engine_lsf.hip  the LSF instantiations of the Huffman stage's kernels
//   clip.hip        k_clip_pack
//   resample.hip    k_clip_audio (its arithmetic: resample_core.h)
//   node.hip        include/pdmp3_node.h over the C-ABI
#ifndef PDMP3_ENGINE_INTERNAL_H
#define PDMP3_ENGINE_INTERNAL_H
#include <hip/hip_runtime.h>

#include <atomic>
#include <mutex>

#include "../../include/pdmp3_hip.h"
#include "decode_core.h"        // TabLds, kNumSfreq: the layout of the tables' allocation below

#define PDMP3_LOCAL __attribute__((visibility("hidden")))

namespace pdmp3 {
struct GcRaw;          // unpack_core.h
struct UnpackTables;
}

// ---- errors (engine.hip): the calling thread's text behind pdmp3_hip_last_error ----
PDMP3_LOCAL int fail(int code, const char* what, hipError_t e);
#define HIP_TRY(call, what)                                   \
  do {                                                        \
    hipError_t e_ = (call);                                   \
    if (e_ != hipSuccess) return fail(PDMP3_HIP_EDEVICE, what, e_); \
  } while (0)
// (for node.hip, which stays on the C-ABI: the calling thread's error text)
extern "C" void pdmp3_hip_set_error_(const char* text);

// ---- the engine context (engine.hip) ----
// Scratch of a chained launch (DecodeArgs::chain_*): launches that are ordered one after the other share a buffer --
// those of one pdmp3_hip_stream (its slots' kernels are chained by the state event), or those of bare calls on one HIP
// stream; launches that may overlap never do.
struct ChainBuf {
  const void* key;          // whose launches share it: a pdmp3_hip_stream's state scratch, or the HIP stream of bare calls
  bool used;
  int cap;                  // frames
  unsigned epoch;           // of the last launch that used it; flags of older launches are smaller, never equal
  float* state;             // cap x 2 kGranFloats floats
  unsigned* flag;           // cap x 4 flags
  unsigned long long last_use;   // launch counter value of its latest use (the least recently used one is evicted)
  // bare calls on this HIP stream (no stream object, which has its own): where the kernel leaves the closing state before it
  // is copied over the caller's, and an LSF launch's regrouped records.  Stream-ordered like the rest: a call's launches are
  // through with them before the next call's on the same stream start.
  float* state_tmp;
  int16_t* pair_sp; pdmp3_gc_side* pair_sd; int pair_cap;   // record-frames
};
constexpr int kChainBufs = 32;

// The decode kernels' tables (decode_core.h GlobalTables) share ONE device allocation, each at a constant 256-byte aligned
// offset: the granule kernel takes the base as its only table parameter and forms the eight pointers from constants; the
// other kernels get a GlobalTables built on the host from the same offsets.  Sizes as host_tables.h builds them (checked
// when the engine is created).
constexpr size_t kTabPow43Bytes = 8207 * sizeof(float);                  // pow43 [8207]
constexpr size_t kTabLinetabBytes = pdmp3::kNumSfreq * 3 * 576 * sizeof(uint16_t);   // linetab [sfreq][kind][576]
constexpr size_t kTabWinBytes = 4 * 36 * sizeof(float);                  // win [4][36]
constexpr int kFragShort = 10 * 64, kFragMat = 20 * 64, kFragTaps = 28 * 64, kFragFloats = 44 * 64;   // frag_long [10][64] | frag_short [10][64] | frag_mat [8][64] | taps [16][64]
constexpr size_t kTabFragBytes = kFragFloats * sizeof(float);
constexpr size_t kTabImageBytes = pdmp3::kNumSfreq * sizeof(pdmp3::TabLds) + sizeof(pdmp3::ScaleTabs);   // [kNumSfreq] TabLds images | the ScaleTabs image
constexpr size_t tab_align(size_t n) { return (n + 255) & ~(size_t)255; }
constexpr size_t kTabOffPow43 = 0;
constexpr size_t kTabOffLinetab = tab_align(kTabOffPow43 + kTabPow43Bytes);
constexpr size_t kTabOffWin = tab_align(kTabOffLinetab + kTabLinetabBytes);
constexpr size_t kTabOffFrag = tab_align(kTabOffWin + kTabWinBytes);
constexpr size_t kTabOffImage = tab_align(kTabOffFrag + kTabFragBytes);
constexpr size_t kTabBytes = tab_align(kTabOffImage + kTabImageBytes);

constexpr int kRareSlots = 4096;      // a flag word per launch, taken round robin: two launches share one only if 4096 others lie between them
struct pdmp3_hip_ctx {
  int device;
  int wave_slots;           // waves of k_decode the device holds at once (CUs x 4 SIMDs x 2)
  pdmp3::UnpackTables* d_unpack;
  int unpack_n16;                // its used part, in 16-byte units
  unsigned long long* d_uprof;   // development only: PDMP3_HIP_UNPACK_PROF=1
  char* d_tables;           // what GlobalTables points into: one allocation, kTabOff* below
  unsigned* d_rare_flags;   // [kRareSlots] epoch numbers (DecodeArgs::rare_flag): "this launch of chunks holds a chunk for k_decode_rare"
  std::atomic<unsigned> rare_epoch;
  int chain_mode;           // PDMP3_HIP_CHAIN=0: independent chunks with halos everywhere; otherwise launches up to
                            // gran_max_frames take the granule kernel (k_decode_g)
  int gran_max_frames;      // launches up to this many frames take the granule kernel (PDMP3_HIP_GRAN_MAX)
  int ring_min_frames;      // launches from this many frames on take the persistent granule kernel (PDMP3_HIP_RING_MIN; 0: never)
  int cus;
  int wave_slots_gran;      // waves of k_decode_g the device holds at once (CUs x 4 SIMDs x 4)
  unsigned debug_flags;     // PDMP3_HIP_DEBUG_FAR_TIMEOUT=1: every wait for another workgroup gives up at once (tests)
  std::atomic<int> last_kind;   // PDMP3_HIP_LAUNCH_* of the latest decode launch, any thread (reports only)
  int direct_max_frames;    // record batches of a stream up to this size run on the pinned host buffers directly (PDMP3_HIP_DIRECT_MAX)
  int gran_w8;              // development: PDMP3_HIP_GRAN_W=8 -- every launch of the granule kernel in workgroups of 8 waves
  int sf_hint;              // sampling-frequency index the granule kernel's line tables are loaded for (PDMP3_HIP_SF_HINT; 0 = 44.1 kHz)
  std::mutex chain_mu;
  unsigned long long chain_clock;
  ChainBuf chain[kChainBufs];
};

// the chain scratch kept under `key` goes back (its launches are complete)
PDMP3_LOCAL void chain_release(pdmp3_hip_ctx* c, const void* key);

// ---- one decode launch (engine.hip launch_decode) ----
// Zero-initialised by default; a call site names the members it sets.
struct DecodeLaunch {
  // input: n_frames records (device memory, or pinned host memory the device reads)
  const int16_t* spectra = nullptr;
  const pdmp3_gc_side* side = nullptr;
  int n_frames = 0;
  bool lsf = false;                     // LSF frames, pdmp3_hip_decode_lsf_frames' layout
  int16_t* pair_sp = nullptr;           // LSF: the caller's buffers for the regrouped records, (n_frames + 1) / 2 frames
  pdmp3_gc_side* pair_sd = nullptr;     //      (NULL: the ones the engine keeps for bare calls on `stream`)
  // output
  void* pcm = nullptr;                  // int16, or float if f32: one destination, never both
  bool f32 = false;
  float* stages = nullptr;              // stage dumps (pdmp3_hip_decode_frames_stages)
  unsigned long long* prof = nullptr;   // shader-clock stamps (pdmp3_hip_debug_profile_phases)
  // synthesis state
  void* state = nullptr;                // carried from launch to launch; NULL: starts from silence, closing state dropped
  float* state_tmp = nullptr;           // where the kernel leaves the new state (NULL: the one kept for bare calls on `stream`)
  bool leave_state_in_tmp = false;      // the caller swaps its state buffers instead of having the new state copied back
  // policy / ordering
  int chunk_frames = 0;                 // include/pdmp3_hip.h pdmp3_hip_decode_frames; 0 = the engine's choice
  hipStream_t stream = nullptr;
  const void* owner = nullptr;          // the stream object whose launches these are (they are ordered: one chain scratch for
                                        // all of them); NULL: a bare call, ordered by its HIP stream
};
PDMP3_LOCAL int launch_decode(pdmp3_hip_ctx* c, const DecodeLaunch& q);

// ---- the device Huffman stage of one window (engine.hip; pdmp3_hip_stream_submit_bits and its kin) ----
struct UnpackWindow {
  hipStream_t stream;
  int n_frames;
  bool lsf;
  const pdmp3_row_desc* desc; const uint8_t* pool;   // compact input (desc != NULL): the reservoir rows are rebuilt from the pool first
  const pdmp3_frame_bits* bits; uint8_t* res;        // side info, reservoir rows
  int16_t* spectra; pdmp3::GcRaw* raw;               // out: the records' spectra, what the merge needs of every granule
  uint32_t* outc; unsigned* mcnt;                    // merge scratch: rows of outcomes (blocks, then super-blocks), the super-blocks' counters
  const uint16_t* sf_in; uint16_t* sf_out;           // scalefactor / count1 carry: the window before's, this window's
  pdmp3_gc_side* side;                               // out: the records' side part
};
// the part that needs nothing of the window before: k_rows (compact input), k_unpack, k_merge_outcome
PDMP3_LOCAL int unpack_window_head(pdmp3_hip_ctx* c, const UnpackWindow& w);
// ... and the part that continues it, to be ordered behind the previous window's state event: k_merge_apply
PDMP3_LOCAL int unpack_window_carry(const UnpackWindow& w);

// ---- engine_lsf.hip ----
hipError_t pdmp3_launch_unpack_lsf(dim3 grid, hipStream_t s, const pdmp3::UnpackTables* tabs, const pdmp3_frame_bits* bits, const uint8_t* res,
                                   int n_frames, int16_t* spectra, pdmp3::GcRaw* raw, int tab_n16, unsigned long long* prof);
hipError_t pdmp3_launch_merge_apply_lsf(dim3 grid, hipStream_t s, const pdmp3::GcRaw* raw, const pdmp3_frame_bits* bits, int n_frames, const uint32_t* outc,
                                        const uint32_t* sup, const uint16_t* state_in, uint16_t* state_out, pdmp3_gc_side* side);
// ---- clip.hip ----
hipError_t pdmp3_launch_clip_pack(hipStream_t s, const pdmp3_clip_piece* pieces, int n_pieces, const void* src);
// ---- resample.hip ----
hipError_t pdmp3_launch_clip_audio(hipStream_t s, const pdmp3_audio_desc* descs, int n_clips, const uint32_t* frames, const float* tables,
                                   long long n_samples, int channels, unsigned lds_bytes);
// ---- mel.hip ----
hipError_t pdmp3_launch_clip_mel(hipStream_t s, const pdmp3_mel_desc* descs, int n_clips, const float* dft, const float* fbt, unsigned* row_max,
                                 const pdmp3_mel_params* params);
// ---- fbank.hip ----
hipError_t pdmp3_launch_clip_fbank(hipStream_t s, const pdmp3_fbank_desc* descs, int n_clips, const float* dft, const float* fbt, float* sums,
                                   const pdmp3_fbank_params* params);
// ---- mfcc.hip ----
hipError_t pdmp3_launch_clip_mfcc(hipStream_t s, const pdmp3_fbank_desc* descs, int n_clips, const float* dft, const float* fbt, const float* dct,
                                  float* sums, const pdmp3_mfcc_params* params);
// ---- stft.hip ----
hipError_t pdmp3_launch_clip_stft(hipStream_t s, const pdmp3_mel_desc* descs, int n_clips, const float* table, const pdmp3_stft_params* params);
// ---- cqt.hip ----
hipError_t pdmp3_launch_clip_cqt(hipStream_t s, const pdmp3_mel_desc* descs, int n_clips, const float* table, const pdmp3_cqt_params* params);
// ---- chroma.hip ----
hipError_t pdmp3_launch_clip_chroma(hipStream_t s, const pdmp3_mel_desc* descs, int n_clips, const float* table, const pdmp3_chroma_params* params);
// ---- loudness.hip ----
// clips [clip0, clip0 + n_clips) of the launch, whose descriptors lie at descs; every other pointer is the whole launch's
hipError_t pdmp3_launch_clip_loudness(hipStream_t s, const pdmp3_mel_desc* descs, int n_clips, int clip0, const pdmp3_loud_tables* tab,
                                      const uint64_t* stats_dst, const uint64_t* mom_dst, double* states, double* starts, float* part, float* sub,
                                      float* gains, const pdmp3_loud_params* params);
hipError_t pdmp3_launch_clip_r128(hipStream_t s, const pdmp3_mel_desc* descs, int n_clips, int clip0, const pdmp3_loud_tables* tab, const float* taps,
                                  const uint64_t* stats_dst, const uint64_t* mom_dst, const uint64_t* st_dst, double* states, double* starts,
                                  float* part, float* sub, float* gains, const pdmp3_r128_params* params);
// ---- pitch.hip ----
hipError_t pdmp3_launch_clip_pitch(hipStream_t s, const pdmp3_mel_desc* descs, int n_clips, const pdmp3_pitch_params* params);
// ---- pyin.hip ----
hipError_t pdmp3_launch_clip_pyin(hipStream_t s, const pdmp3_pyin_desc* descs, int n_clips, const double* tables, const pdmp3_pyin_params* params);
// ---- beat.hip ----
hipError_t pdmp3_launch_clip_beat(hipStream_t s, const pdmp3_beat_desc* descs, int n_clips, int first, const double* tables, double* work,
                                  const pdmp3_beat_params* params);
// ---- tempogram.hip ----
hipError_t pdmp3_launch_clip_tempogram(hipStream_t s, const pdmp3_tempogram_desc* descs, int n_clips, const float* window, const double* prior,
                                       const pdmp3_tempogram_params* params);
// ---- stft_long.hip ----
hipError_t pdmp3_launch_clip_stft_long(hipStream_t s, const pdmp3_mel_desc* descs, int n_clips, const float* tables,
                                       const pdmp3_stft_long_params* params);
// ---- mel_long.hip ----
hipError_t pdmp3_launch_clip_mel_long(hipStream_t s, const pdmp3_mel_desc* descs, int n_clips, const float* tables, const float* operand,
                                      const pdmp3_mel_long_params* params);
// ---- spectral.hip ----
hipError_t pdmp3_launch_clip_spectral(hipStream_t s, const pdmp3_mel_desc* descs, int n_clips, const float* tables,
                                      const pdmp3_spectral_params* params);
// ---- hpss.hip ----
hipError_t pdmp3_launch_clip_hpss(hipStream_t s, const pdmp3_mel_desc* descs, int n_clips, const pdmp3_hpss_params* params);
// ---- mfcc_long.hip ----
hipError_t pdmp3_launch_clip_mfcc_long(hipStream_t s, const pdmp3_mel_desc* descs, int n_clips, const float* dct,
                                       const pdmp3_mfcc_long_params* params);

#endif
