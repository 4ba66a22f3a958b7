/*
 * pdmp3_bulk.h -- whole-stream decoding on top of include/pdmp3.h
 * (pdmp3_amd/libpdmp3.so).
 *
 * NOT part of the reference's API: the reference decodes one frame per
 * pdmp3_read() iteration on one core.  This is the throughput form of the same
 * contract for callers that hold a whole file in memory (first
 * "next" row: the host Huffman stage that feeds the transforms).  The OUTPUT
 * is defined by the reference: byte for byte what its CLI driver pdmp3()
 * (pdmp3.c:2540-2589: 4096-byte feeds, 16 KiB reads, raw int16 sink) writes
 * for the same bytes, including the dropped tail and the stop at
 * the first frame error.
 *
 * Inside: the reference's read loop runs sequentially but only as far as the
 * bit reservoir (everything that depends on the previous frame); scalefactor +
 * Huffman decoding of each frame, a pure function of its reservoir snapshot,
 * runs on a pool of host threads straight into pinned staging memory; windows
 * of frames go through pdmp3_hip_stream_submit() (include/pdmp3_hip.h) three
 * deep, so upload, transforms, download and host decoding overlap.
 */
#ifndef PDMP3_BULK_H
#define PDMP3_BULK_H

#include <stddef.h>
#include <stdint.h>
#include "pdmp3_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bulk pdmp3_amd_bulk;

/* Returned by the scan / decode / parse entry points when the stream drives the reference into replaying its
 * 16 KiB input ring: pdmp3_feed leaves the write index AT the end of the ring when a feed ends exactly there
 * (pdmp3.c:2410-2417), and a frame that then ends exactly there too -- only 1152-byte frames can: 32 kHz at
 * 256 kbps, the limit of SURVEY H10 -- wraps the read index past it (pdmp3.c:1464-1474), after which the ring
 * looks full of its own stale bytes.  The reference's CLI then writes the same audio again, usually forever
 * (libpdmp3.so's pdmp3_read / pdmp3() keep that behaviour, as a drop-in must).  There is no finite reference
 * output to reproduce, so the whole-stream entry points stop and say so. */
#define PDMP3_BULK_REPLAY (-2)

/* threads <= 0: one worker per usable CPU (affinity and cgroup quota; at most 64; 4 with device Huffman, where the
 * pool only copies PCM out).  window_frames <= 0: with device Huffman the engine's slots hold 8192 frames -- the split scan
 * (below) fills them as far as its scanners have got when a slot is free, the one-thread scan closes its windows at 4096 --,
 * with host Huffman 2048; a size given explicitly is both (at most 32768).  Returns NULL when there is no transform
 * engine (no CPU fallback). */
pdmp3_amd_bulk* pdmp3_amd_bulk_new(int threads, int window_frames);
/* Environment: PDMP3_BULK_HOST_HUFFMAN=1 (below), PDMP3_BULK_SNAPSHOT_ROWS=1 (upload 2064-byte reservoir snapshots per frame
 * instead of the compact pool + row descriptors: tests), PDMP3_BULK_TRACE=1 (one summary of the pipeline's waits per decode on
 * stderr; 2: a line per window as well), PDMP3_BULK_SCAN_THREADS=n (0 .. 16: scanner threads of the split scan -- a pre-pass
 * hops from header to header and n threads run the scan from every 256th frame into private windows that the calling
 * thread puts into the engine's slots in stream order, results identical to the one-thread scan; by default 12 / 8 / 4 / 2 with
 * 32 / 16 / 12 / 6 usable CPUs when the PCM stays in device memory, where the scan is the bound, four of them at most for
 * destinations in host memory (there with the engine's windows closed at 4096 frames; decoders made with windows shorter than
 * 1024 frames, and hosts with fewer than 12 usable CPUs, keep the one-thread scan); given explicitly: that many for every destination and for streams from 4 private
 * windows on instead of 12; 0: never; decoders of one process that scan
 * at the same time share: the second takes half the scanners, the third a third ...), PDMP3_BULK_PREPASS_THREADS=n (1 .. 8
 * parts of the pre-pass, all but the first with a thread of their own that hops from a guessed header; 6 / 3 / 1 by default
 * with 16 / 12 / fewer usable CPUs; no part shorter than 256 KB), PDMP3_BULK_SUB_FRAMES=n (frames of a private window; 256 by
 * default), PDMP3_BULK_SCAN_SPIN=0 / 1 (a scanner whose snapshot is the next or the one after yields / spins while it waits; by
 * default it spins where the process has 2 x scanners + 8 CPUs),
 * PDMP3_BULK_GATHER_THREADS=n (0 .. 8 helper threads for the copies of the windows' main data into the pinned upload
 * buffers; 6 by default with 8 scanners, 3 with fewer, 0 without), PDMP3_BULK_GATHER_NT=0 (those copies with memcpy instead
 * of non-temporal stores).
 * Thread footprint of ONE decoder with a device destination on a host with 16 usable CPUs or more, for its lifetime
 * (the threads are started when a stream first needs them and then sleep on a job queue between streams): 8 scanners,
 * 5 hop threads + the pre-pass, 6 gather helpers, the submitter and the copy-out pool (`threads`) -- about 25.  Only
 * the scanners are shared out between decoders of one process that scan at the same time (above); gather helpers,
 * hop threads and the pre-pass are per decoder, and their waits yield the CPU (sched_yield) or nap 20 us at a time rather
 * than sleep on a condition (the scanners' wait for their snapshots: a broadcast per snapshot to a dozen sleepers was
 * the split scan's bottleneck until round 5).  A
 * process that keeps many decoders (one per GPU and more) should size them with the variables above --
 * PDMP3_BULK_SCAN_THREADS=2 PDMP3_BULK_PREPASS_THREADS=1 PDMP3_BULK_GATHER_THREADS=1 is 6 threads per decoder. */
/* host_huffman = 0 (what pdmp3_amd_bulk_new gives unless PDMP3_BULK_HOST_HUFFMAN=1 is set): the host only runs
 * the sequential scan and ships side info + reservoir snapshots; scalefactors, Huffman and the frame-to-frame
 * merge run on the device (pdmp3_hip_stream_submit_bits) and the pool just copies PCM out.  host_huffman = 1:
 * they run on the pool and the engine is given decoded records (pdmp3_hip_stream_submit). */
pdmp3_amd_bulk* pdmp3_amd_bulk_new_ex(int threads, int window_frames, int host_huffman);
/* the same on HIP device `device` (the others use $PDMP3_DEVICE, default 0).  Decoders are independent: a corpus of
 * files is dealt over the GPUs of a node by giving each host thread its own decoder (whole files per GPU,
 * largest first; pdmp3_amd/sharding.py assign_files) -- there is nothing to exchange between them. */
pdmp3_amd_bulk* pdmp3_amd_bulk_new_on(int threads, int window_frames, int host_huffman, int device);
void pdmp3_amd_bulk_delete(pdmp3_amd_bulk* b);
int pdmp3_amd_bulk_threads(const pdmp3_amd_bulk* b);
/* Streams the decoder's split scan (several scanner threads; taken for device destinations, or with
 * PDMP3_BULK_SCAN_THREADS) decoded to their end, and streams it gave up half way -- irregular ones: resync, tags, a
 * truncation the ring's feed cadence shows -- and decoded again with the one-thread scan.  Same PCM either way. */
void pdmp3_amd_bulk_split_scans(const pdmp3_amd_bulk* b, long long* taken, long long* given_up);
/* Frames whose scalefactors + Huffman data the device stage (*device) and the host pool (*host) decoded over the decoder's
 * life: the frames of every stream it decoded to its end, by the stage that decoded them (a stream the split scan gave up
 * counts once).  Either pointer may be NULL. */
void pdmp3_amd_bulk_huffman_frames(const pdmp3_amd_bulk* b, long long* device, long long* host);
/* ISO-correct switches (include/pdmp3.h: PDMP3_ISO_*, pdmp3_amd_set_quirks) for the streams decoded from now on;
 * 0 (the default) = the reference's behaviour, bit for bit.  The CLI driver reads the mask from $PDMP3_CLI_ISO. */
int pdmp3_amd_bulk_set_quirks(pdmp3_amd_bulk* b, unsigned iso_mask);
/* PDMP3_ISO_LSF (MPEG-2 LSF / MPEG-2.5 streams, which the reference rejects): both Huffman stages take LSF frames.  A
 * window closes where the version, or an LSF stream's channel count, changes, and goes to the engine as an LSF window
 * (pdmp3_hip_stream_set_lsf): a device-Huffman decoder hands the LSF form of pdmp3_frame_bits to the device, which builds
 * the host stage's records from it, byte for byte; a host_huffman decoder decodes them on its pool.  LSF, MPEG-1 and
 * mixed-version streams go through either kind of decoder in their own calls, asynchronously where the call is.  The split
 * scan (several scanner threads) is MPEG-1 only: a stream in which it meets an LSF frame anywhere, its last bytes included,
 * is given up and decoded from its first byte by the one-thread scan -- what counts as a frame never depends on which
 * scan or stage reads it. */

/* PCM bytes (return value) and frames pdmp3() would produce for this stream;
 * header / side-info / reservoir pass only, no Huffman, no GPU.  Use it to
 * size the output of pdmp3_amd_bulk_decode. */
long long pdmp3_amd_scan_buffer(const unsigned char* mp3, size_t n, long long* frames);
/* ... with a decoder's switches (pdmp3_amd_bulk_set_quirks): PDMP3_ISO_LSF makes MPEG-2 LSF / 2.5 frames count */
long long pdmp3_amd_scan_buffer_iso(const unsigned char* mp3, size_t n, unsigned iso_mask, long long* frames);

/* Decode one whole stream with a fresh decoder state.  Returns the PCM byte
 * count pdmp3() writes for it; pcm[0 .. min(return, pcm_cap)) holds them
 * (interleaved int16; bytes of `pcm` past the return value are unspecified).
 * -1 on an engine failure.  rate / channels (may be NULL): format of the last
 * header seen, as pdmp3_getformat reports it. */
long long pdmp3_amd_bulk_decode(pdmp3_amd_bulk* b, const unsigned char* mp3, size_t n,
                                unsigned char* pcm, size_t pcm_cap, long* rate, int* channels);

/* Optional: PCM buffers in pinned host memory.  When the `pcm` given to the decode calls lies in such a buffer the
 * GPU downloads every window straight into it (mono frames packed on the way) and the host never touches the
 * samples; any other memory works too, through a staging buffer and a copy by the pool.  A DEVICE pointer (hipMalloc,
 * a torch tensor) is accepted as `pcm` as well: the PCM then never leaves the GPU -- the decode kernel stores it there
 * itself when the destination is memory of the decoder's device and takes whole frames (copies otherwise).  The decoder
 * works on HIP streams of its own, which do NOT wait for the caller's: whatever the caller still has in flight on the
 * buffer (a fill, an earlier consumer) must be complete before the decode call, and a consumer on another stream starts
 * after pdmp3_amd_bulk_decode / pdmp3_amd_bulk_wait has returned. */
void* pdmp3_amd_pcm_alloc(size_t bytes);
void pdmp3_amd_pcm_free(void* p);

/* The same without waiting for the tail: returns as soon as the stream is scanned and its windows are queued on
 * the device (`mp3` may be released then, `pcm` must stay); the PCM of every stream given so far is complete after
 * pdmp3_amd_bulk_wait() returns 0.  The next stream's scan overlaps the previous one's GPU work and copy-out, so a
 * corpus of medium-sized files runs at the long-stream rate instead of paying a pipeline fill and drain per file.
 * Each stream starts from a fresh decoder state, exactly as with pdmp3_amd_bulk_decode (PDMP3_FR_RESET /
 * PDMP3_FR_NEWSTREAM on its first frame; nothing is reset from the host).  Host-Huffman decoders simply wait. */
long long pdmp3_amd_bulk_decode_async(pdmp3_amd_bulk* b, const unsigned char* mp3, size_t n,
                                      unsigned char* pcm, size_t pcm_cap, long* rate, int* channels);
int pdmp3_amd_bulk_wait(pdmp3_amd_bulk* b);

/* Host stages only, for tests on machines without a GPU: a decoder made by
 * pdmp3_amd_bulk_new_parse_only() writes the gc records the engine would be
 * given into caller memory (cap_frames frames of 2304 int16 / 4 records).
 * Returns the frame count, -1 if they do not fit. */
pdmp3_amd_bulk* pdmp3_amd_bulk_new_parse_only(int threads, int window_frames);
long long pdmp3_amd_bulk_parse(pdmp3_amd_bulk* b, const unsigned char* mp3, size_t n,
                               int16_t* spectra, pdmp3_gc_side* side, size_t cap_frames, long long* pcm_bytes);

/* The scan alone, in the device-Huffman form: per frame the pdmp3_frame_bits and PDMP3_RESERVOIR_BYTES of
 * reservoir that the engine would be given (host tests). */
pdmp3_amd_bulk* pdmp3_amd_bulk_new_parse_bits(void);
/* ... and the scan a device-Huffman decoder runs: with PDMP3_ISO_LSF (pdmp3_amd_bulk_set_quirks) it takes MPEG-2 LSF / 2.5
 * frames, in the LSF form of pdmp3_frame_bits, where the one above ends at the first of them.  For both parse entries. */
pdmp3_amd_bulk* pdmp3_amd_bulk_new_parse_bits_lsf(void);
long long pdmp3_amd_bulk_parse_bits(pdmp3_amd_bulk* b, const unsigned char* mp3, size_t n, pdmp3_frame_bits* bits,
                                    uint8_t* reservoir, size_t cap_frames, long long* pcm_bytes);

/* The same in the compact form the engine is actually given (include/pdmp3_hip.h, pdmp3_row_desc): side info, row
 * descriptors and the pool, as ONE window holding the whole stream (host tests: the rows rebuilt from it must be the
 * snapshots of pdmp3_amd_bulk_parse_bits).  pool_cap: capacity of `pool`; *pool_bytes: what was used. */
long long pdmp3_amd_bulk_parse_pool(pdmp3_amd_bulk* b, const unsigned char* mp3, size_t n, pdmp3_frame_bits* bits,
                                    pdmp3_row_desc* desc, uint8_t* pool, size_t pool_cap, size_t cap_frames, size_t* pool_bytes);

/* The streaming API (include/pdmp3.h) driven from a memory buffer by a C loop: pdmp3_new, pdmp3_open_feed, then
 * pdmp3_read(read_bytes) until PDMP3_ERR, with a pdmp3_feed of feed_bytes on every PDMP3_NEED_MORE -- the
 * reference driver's loop (pdmp3.c:2564-2584; 4096 and 16384 there) with its two sizes as parameters.  eager != 0:
 * the caller keeps the ring as full as feed_bytes-sized feeds allow instead of waiting for PDMP3_NEED_MORE, but never
 * to the last byte (a ring filled exactly looks EMPTY to the reference, pdmp3.c:1062-1068, and so to this library).  At most
 * `cap` bytes go to `out` (may be NULL); returns the PCM bytes the reads delivered, -1 without an engine.  For
 * measuring the drop-in path without an interpreter in the loop (bench.py: streaming_api). */
long long pdmp3_amd_stream_loop(const unsigned char* mp3, size_t n, unsigned char* out, size_t cap,
                                size_t feed_bytes, size_t read_bytes, int eager);

/* A PCM buffer as a RIFF/WAVE file: interleaved int16 (float32 = 0) or 32-bit float (float32 != 0; the output of
 * pdmp3_amd_set_encoding(PDMP3_ENC_FLOAT_32)).  The reference's only sink is the raw writer (pdmp3.c:2236-2257); the
 * CLI driver writes "<first name>.wav" instead of ".raw" when PDMP3_CLI_WAV=1 is set.  PDMP3_OK or PDMP3_ERR. */
int pdmp3_amd_write_wav(const char* path, const void* pcm, size_t bytes, long rate, int channels, int float32);

/* ---- Frame ranges and batches of clips ----
 * A range's PCM is DEFINED as a byte slice of what pdmp3() writes for the whole stream: frames [a, b) are the bytes
 * [pcm_offset(a), pcm_offset(b)) of the whole-stream decode, bit for bit.  Nothing else changes; no entry point above
 * returns anything other than it did.
 *
 * A stream index is built once per stream: the one-thread scan in its count-only form (what counts as a frame and each
 * frame's PCM size are exactly pdmp3_amd_scan_buffer_iso's, whichever form the index takes -- a mono frame of a stereo
 * stream is 2304 bytes, an LSF frame half of an MPEG-1 one), and, where the split scan's pre-pass takes the stream (MPEG-1,
 * no resync, H9, H16 / H18 or tags; the same verdict as for the whole-stream decoder), the pre-pass's snapshots every
 * `spacing` frames (256 by default), from which a scan can start in the middle of the stream.  A stream the pre-pass does
 * not take (every LSF stream among them) keeps no snapshot: its clips are scanned from frame 0 (pdmp3_amd_index_split says
 * which).  Memory: 13 bytes per frame (PCM offset, flag byte, the side-info bits of the halo rule), 24 more per frame with
 * snapshots (the pre-pass's frame records, which a scan started from a snapshot reads); per `spacing` frames 128 bytes of
 * halo checkpoint and, with snapshots, 128 bytes + 4 per frame whose main data is still visible in the reservoir.  About
 * 5.3 MB for an hour at 44.1 kHz (137 812 frames), next to the 57 MB of a 128 kbps stream; built in 0.2-0.3 ms per MB of
 * stream on one core.  The index does not keep the
 * stream: the clip calls are given the same bytes again (n is checked).
 * iso_mask: only PDMP3_ISO_LSF matters (it changes what counts as a frame); a decoder's switches must agree with it.
 * A stream whose scan ends in a ring replay gives an index whose frame count is PDMP3_BULK_REPLAY. */
typedef struct pdmp3_amd_index pdmp3_amd_index;
pdmp3_amd_index* pdmp3_amd_index_new(const unsigned char* mp3, size_t n, unsigned iso_mask);
/* ... with snapshots every `spacing` frames (<= 0: the default).  No result depends on it (tests build with two). */
pdmp3_amd_index* pdmp3_amd_index_new_spacing(const unsigned char* mp3, size_t n, unsigned iso_mask, int spacing);
void pdmp3_amd_index_delete(pdmp3_amd_index* ix);
long long pdmp3_amd_index_frames(const pdmp3_amd_index* ix);   /* == pdmp3_amd_scan_buffer_iso's frames, or PDMP3_BULK_REPLAY */
/* bytes of pdmp3()'s output before `frame`; frame == frames gives the total; -1 outside [0, frames] */
long long pdmp3_amd_index_pcm_offset(const pdmp3_amd_index* ix, long long frame);
/* all frames + 1 of them into out[0 .. min(cap, frames + 1)); returns frames + 1 (or the index's negative frame count) */
long long pdmp3_amd_index_pcm_offsets(const pdmp3_amd_index* ix, long long* out, size_t cap);
/* 1: the pre-pass took the stream (snapshots); 0: the one-thread scan built the index (scans start at frame 0) */
int pdmp3_amd_index_split(const pdmp3_amd_index* ix);

/* A clip: frames [first_frame, first_frame + n_frames) of a stream, both clamped to the index's frames.  dst is pageable,
 * pinned (pdmp3_amd_pcm_alloc) or device memory of the decoder's GPU, as for pdmp3_amd_bulk_decode. */
typedef struct {
  const unsigned char* mp3; size_t n; const pdmp3_amd_index* index;
  long long first_frame, n_frames;
  void* dst; size_t dst_cap;
} pdmp3_amd_clip;
/* Decodes a batch of clips, of one stream or of many.  pcm_bytes[k] = pcm_offset(b) - pcm_offset(a) of clip k's clamped
 * range [a, b); dst[0 .. min(that, dst_cap)) receives exactly those bytes of the whole-stream output (interleaved int16 as
 * pdmp3_amd_bulk_decode writes it); nothing past them is written.  Each clip is decoded from a frame `first` <= a that the
 * halo rule picks so that the result is exact -- two frames, further back past mono runs, and as far
 * back as the frames that last set a scalefactor or count1 value the range reads -- and is scanned from the index's nearest
 * snapshot at or before `first`; the PCM of [first, a) is thrown away on the GPU (k_clip_pack places the kept frames: on
 * the device for device destinations, mono / stereo / LSF mixed or not; through the slot's pinned buffer, kept bytes only,
 * for host ones).  The clips' frames share the engine's windows (a window costs the GPU about 150 us whatever its size);
 * a clip's first frame carries PDMP3_FR_RESET and PDMP3_FR_NEWSTREAM; windows split where the version changes, as for a
 * whole stream; a clip longer than a window goes on in the next with its state carried.
 * Synchronous: every clip is in place on return; earlier asynchronous decodes are waited for first.  Returns 0; -1 on a
 * bad argument, an engine failure, a decoder with host Huffman or parse only (not supported), or a decoder whose
 * PDMP3_ISO_LSF switch differs from an index's; PDMP3_BULK_REPLAY when a clip's index says so (those clips' pcm_bytes
 * are PDMP3_BULK_REPLAY too and nothing of them is written; the others are decoded). */
int pdmp3_amd_bulk_decode_clips(pdmp3_amd_bulk* b, const pdmp3_amd_clip* clips, int n_clips, long long* pcm_bytes);
/* frames the decoder's clips kept (the sum of their clamped n_frames) and frames it decoded in front of them and threw
 * away (the sum of a - first) over its life: a stream that forces long halos shows here.  Either pointer may be NULL. */
void pdmp3_amd_bulk_clip_stats(const pdmp3_amd_bulk* b, long long* clip_frames, long long* halo_frames);
/* Host tests (a decoder of pdmp3_amd_bulk_new_parse_only): the host stage on ONE range, with the same index and the same
 * halo rule as the clip decode: the records of frames [first, b) into spectra / side (cap_frames frames), *decoded_from =
 * first.  lookback = 0 leaves out the scalefactor / count1 part of the rule (the synthesis halo alone: tests show that
 * it matters).  Returns b - first, or -1 / PDMP3_BULK_REPLAY. */
long long pdmp3_amd_bulk_parse_range(pdmp3_amd_bulk* b, const unsigned char* mp3, size_t n, const pdmp3_amd_index* ix,
                                     long long first_frame, long long n_frames, int lookback, int16_t* spectra, pdmp3_gc_side* side,
                                     size_t cap_frames, long long* decoded_from);

/* ---- Clips by sample position as float batches ----
 * What a loader feeds to a model: K clips addressed in samples, as one dense planar float32 batch [K][C][T] at ONE sampling
 * frequency and channel count, made on the GPU from the clips' int16 PCM while it is still in device memory.  Every value is
 * defined from the whole-stream int16 output above; nothing any entry point above returns changes.
 *
 * Time line.  A stream has ONE FORMAT when all its frames have the same sampling frequency and the same samples per frame
 * spf (1152 MPEG-1, 576 LSF); channel counts may change.  It then has N = frames * spf samples per channel, sample n lies in
 * frame n / spf, and x_c[n] is the whole-stream int16 output / 32768 for 0 <= n < N and 0 outside; a mono frame inside a stereo
 * stream gives its samples to both channels.  A stream whose frames differ in rate or spf has no time line.
 * Channels.  Cs = 2 if any frame is stereo, else 1.  Asked for C = 1 from Cs = 2: x[n] = (l + r) / 65536 with l, r the int16
 * values (exact in binary32); C = 2 from Cs = 1: both channels equal.  The downmix comes before the filter.
 * Rate.  in = the stream's, out = the requested one, g = gcd, M = in / g, L = out / g, Z = width, and
 *     u(n, j) = rolloff * (n L - j M) / max(L, M)
 *     h(n, j) = rolloff * min(L, M) / M * sinc(u) * cos^2(pi u / (2 Z))   for |u| < Z, else 0;   sinc(u) = sin(pi u) / (pi u)
 *     y_c[j]  = sum over n of h(n, j) * x_c[n]          for 0 <= j < J = ceil(N L / M), 0.0 from J on
 * (a Hann-windowed sinc with its cut-off at rolloff * min(in, out) / 2: torchaudio's sinc_interp_hann with the same two
 * parameters).  h depends on j through (j M) mod L alone: the table of L rows is computed on the host in binary64, rounded
 * once to binary32 and kept by the decoder per (in, out, Z, rolloff); the GPU multiplies and adds in binary32.  out == in: no
 * filter at all, y_c[j] = x_c[j] exactly. */
/* 1: the stream has one format (*rate, *channels = Cs, *frame_samples = spf), 0: its frames differ in rate or spf (only
 * *channels is set), -1: a replay index or NULL.  An index without frames has one format with rate 0.  Pointers may be NULL. */
int pdmp3_amd_index_format(const pdmp3_amd_index* ix, long* rate, int* channels, int* frame_samples);
/* N = frames * spf of a stream with one format, else -1 */
long long pdmp3_amd_index_samples(const pdmp3_amd_index* ix);

/* Planning, plain C (host tests reach both).  The input samples [*first_in, *first_in + *n_in) that output samples [start,
 * start + n) at rate `out` read from a stream at rate `in`, before any clamping to [0, N): every n with |u(n, j)| < Z for
 * one of those j, and at most one sample more on either side.  width 0 = 6 (1 .. 64), rolloff 0 = 0.99 (in (0, 1]); out == in:
 * [start, start + n).  0, or -1 on a bad argument. */
int pdmp3_amd_audio_span(long in, long out, int width, double rolloff, long long start, long long n, long long* first_in, long long* n_in);
/* The filter table of the pair: *rows = L rows of *taps coefficients, row r = (j M) mod L, whose tap k multiplies input sample
 * floor(j M / L) + *first_tap + k.  Returns the coefficient count rows * taps and writes them to table[0 .. min(that, cap));
 * -1 on a bad argument, out == in (no table) or a table of more than 2^22 coefficients. */
long long pdmp3_amd_audio_table(long in, long out, int width, double rolloff, float* table, size_t cap, long* rows, int* taps, int* first_tap);
/* What a workgroup of k_clip_audio keeps in LDS for a clip of the pair in a call with `channels` (1 or 2) channels, as the
 * decode call itself decides it (the same function): *flags = PDMP3_AUDIO_LDS_X (1: the input span of a tile of 1024 output
 * samples, *span_cap samples a channel, a multiple of 4) | PDMP3_AUDIO_LDS_TABLE (2: the table behind it) of
 * include/pdmp3_hip.h pdmp3_audio_desc; 0, 0: every output sample straight from memory, and at out == in (no filter).  0, or
 * -1 on a bad argument or another channel count.  Either pointer may be NULL. */
int pdmp3_amd_audio_lds_plan(long in, long out, int width, double rolloff, int channels, unsigned* flags, unsigned* span_cap);

/* A clip of the batch: output samples [start, start + n_samples) of the stream at the requested rate.  dst: device memory of
 * the decoder's GPU (written by the kernel itself) or host memory (kernel into a device stage, copied out); channel c's
 * n_samples floats at dst + c * chan_stride. */
typedef struct {
  const unsigned char* mp3; size_t n; const pdmp3_amd_index* index;
  long long start; float* dst; size_t chan_stride;
} pdmp3_amd_audio_clip;
/* 0 = default: the stream's own rate, the clips' common Cs (their Cs must agree then), width 6, rolloff 0.99 */
typedef struct { long rate; int channels; long long n_samples; int width; double rolloff; } pdmp3_amd_audio_spec;
#define PDMP3_BULK_MIXED_FORMAT (-3)
/* Row k receives y_c[start + t] for 0 <= t < n_samples, 0.0 where start + t >= J (the batch is dense), and valid[k] =
 * clamp(J - start, 0, n_samples).  The frames a clip's input span touches go through the clip path above unchanged -- halo
 * rule, snapshots, windows, k_clip_pack -- into a device stage the decoder owns; k_clip_audio then writes the rows.
 * Synchronous; device-Huffman decoders only; the decoder's PDMP3_ISO_LSF must match every index.  Returns 0; -1 on a bad
 * argument (start < 0, n_samples < 0, width outside 1 .. 64, rolloff outside (0, 1], channels 0 with clips whose Cs differ, a
 * filter table of more than 2^22 coefficients) and as pdmp3_amd_bulk_decode_clips.  A clip whose index is a replay: valid[k]
 * = PDMP3_BULK_REPLAY and the call returns that; one whose stream has no one format: valid[k] = PDMP3_BULK_MIXED_FORMAT and the
 * call returns that unless a replay does; nothing of such a row is written and the other clips are decoded.
 * pdmp3_amd_bulk_clip_stats counts these clips' frames and halos too. */
int pdmp3_amd_bulk_decode_clips_audio(pdmp3_amd_bulk* b, const pdmp3_amd_audio_clip* clips, int n_clips,
                                      const pdmp3_amd_audio_spec* spec, long long* valid);

/* ---- Log-mel features of clips ----
 * What speech and audio models consume, made on the GPU behind k_clip_audio while the resampled signal is in device memory:
 * K clips as one planar float32 batch [K][C][n_mels][F], frames innermost.  Nothing any entry point above returns changes.
 *
 * Signal.  y_c[j] is the resampled signal above at the requested rate sr and channel count for 0 <= j < J, and 0.0 outside.
 * The input of the feature stage is the binary32 value pdmp3_amd_bulk_decode_clips_audio produces for y_c[j].
 * Window.  Periodic Hann, w[n] = 0.5 - 0.5 cos(2 pi n / N), N = n_fft (even, 16 .. 1024).
 * Frame.  A clip is (stream, index, start), start >= 0 a sample position at sr.  Frame f is centred on sample start + f H
 * (H = hop, 1 .. N); with K = N / 2 + 1 bins
 *     X[f, k] = sum over n < N of w[n] y[start + f H - N / 2 + n] e^(-2 pi i k n / N),      P[f, k] = Re^2 + Im^2.
 * Samples in front of 0 and from J on are zeros; NO reflection is used, and inside a stream the window sees the stream's real
 * neighbours, not padding.  So the first and the last N / (2 H) frames of a STREAM differ from a transform that reflects its
 * input at the ends (torch.stft center=True, librosa), and every other frame -- a clip's first and last ones included -- is
 * the usual definition on the stream's own samples.
 * Filterbank.  n_mels + 2 points equally spaced in mel between f_min and f_max (0 = sr / 2; 0 <= f_min < f_max <= sr / 2),
 * mapped back to Hz as f_0 .. f_(n_mels + 1); the frequency of bin k is k sr / N;
 *     W[m, k] = max(0, min((k sr / N - f_m) / (f_(m+1) - f_m), (f_(m+2) - k sr / N) / (f_(m+2) - f_(m+1)))),
 * norm = 1 multiplies row m by 2 / (f_(m+2) - f_m).  scale = 1 (HTK): mel = 2595 log10(1 + f / 700); scale = 0 (Slaney):
 * mel = 3 f / 200 below 1000 Hz, 15 + 27 ln(f / 1000) / ln 6.4 from there on.  M[f, m] = sum over k of W[m, k] P[f, k].
 * Output.  out_mode 0: M; 1: ln max(M, floor); 2: log10 max(M, floor); 3 ("whisper"): with g = log10 max(the largest M of the
 * row -- all its frames, bands and channels --, floor):  (max(log10 max(M, floor), g - 8) + 4) / 4.  floor > 0 is rounded to
 * binary32 first.  valid[k] = clamp(ceil((J - start) / H), 0, F) counts the frames whose centre lies inside the stream;
 * frames behind the stream's end are the transform of zeros: M = 0, or the floor's logarithm.
 * The DFT coefficients (window folded in) and the filterbank are computed on the host in binary64 and rounded once to
 * binary32; the GPU multiplies and adds in binary32 (v_mfma_f32_16x16x4_f32: fused multiply-add chains). */
typedef struct {
  long rate; int channels; int width; double rolloff;   /* as pdmp3_amd_audio_spec (rate 0: the clips' common own rate) */
  int n_fft, hop, n_mels;
  double f_min, f_max;                                  /* f_max 0 = rate / 2 */
  int scale, norm;                                      /* 0 Slaney / 1 HTK; 0 none / 1 Slaney's area normalisation */
  long long n_frames;
  int out_mode;                                         /* 0 power, 1 ln, 2 log10, 3 whisper */
  double floor;                                         /* > 0 */
} pdmp3_amd_mel_spec;
/* Planning, plain C (host tests reach all of it).  0 when the spec's numbers are acceptable at sampling frequency sr, else -1:
 * n_fft odd or outside 16 .. 1024, hop outside 1 .. n_fft, n_mels outside 1 .. 256, f_min < 0, f_max > sr / 2, f_min >= f_max,
 * scale / norm / out_mode unknown, n_frames < 0, floor not > 0 (or smaller than binary32's least normal number). */
int pdmp3_amd_mel_check(const pdmp3_amd_mel_spec* spec, long sr);
/* The samples [*first, *first + *count) that frames 0 .. n_frames - 1 of a clip at `start` read, before any clamping:
 * [start - N / 2, start + (n_frames - 1) H + N / 2); count 0 for no frame.  0, or -1 on a bad argument. */
int pdmp3_amd_mel_span(int n_fft, int hop, long long start, long long n_frames, long long* first, long long* count);
/* The DFT table as k_clip_mel's B operand: *rows = n_fft rounded up to 4 rows of *cols = 2 Kp floats, Kp = K rounded up to
 * 16; row n holds w[n] cos(2 pi k n / N) at column k and -w[n] sin(2 pi k n / N) at column Kp + k for k < K; the padding rows
 * and columns are 0.  The angle is reduced as the integer k n mod N.  Returns rows * cols and writes min(that, cap) floats;
 * -1 on a bad n_fft. */
long long pdmp3_amd_mel_dft_table(int n_fft, float* table, size_t cap, int* rows, int* cols);
/* The filterbank, dense [n_mels][K].  Returns n_mels * K and writes min(that, cap) floats; -1 on a bad argument. */
long long pdmp3_amd_mel_filterbank(long sr, int n_fft, int n_mels, double f_min, double f_max, int scale, int norm, float* w, size_t cap);
/* What a workgroup of k_clip_mel takes: *tile frames (32, or 16 where 32 need more than 64 KB of LDS), the LDS floats between
 * two hops' worth of the signal (*row_pad: hop + row_pad = 2 mod 32, no bank conflicts between the rows of a tile) and the
 * LDS of a workgroup in bytes.  0, or -1 on a bad argument.  Pointers may be NULL. */
int pdmp3_amd_mel_tile(int n_fft, int hop, int n_mels, int* tile, int* row_pad, unsigned* lds_bytes);
/* Row k receives channel c's [n_mels][n_frames] floats at dst + c * chan_stride (pdmp3_amd_audio_clip; chan_stride >= n_mels *
 * n_frames).  The call decodes the samples the frames read with pdmp3_amd_bulk_decode_clips_audio itself into a device stage
 * the decoder owns, and k_clip_mel (csrc/mel.hip) writes the rows; host destinations go through a second stage.  Synchronous.
 * Returns, refuses (PDMP3_BULK_REPLAY / PDMP3_BULK_MIXED_FORMAT per clip in valid[k], the other clips decoded) and counts
 * (pdmp3_amd_bulk_clip_stats) as pdmp3_amd_bulk_decode_clips_audio; -1 also where pdmp3_amd_mel_check says so and for rate 0
 * with clips of different rates. */
int pdmp3_amd_bulk_decode_clips_mel(pdmp3_amd_bulk* b, const pdmp3_amd_audio_clip* clips, int n_clips, const pdmp3_amd_mel_spec* spec,
                                    long long* valid);

/* ---- Kaldi-style filterbank features of clips ----
 * Kaldi's `fbank` front end (torchaudio.compliance.kaldi.fbank's options, by their names there) on the same resampled signal:
 * K clips as one planar float32 batch [K][C][F][D], frames by coefficients, coefficients innermost.  New entry points only;
 * nothing any entry point above returns changes.
 *
 * Signal.  y_c[j] as for the log-mel call: the resampled signal at the requested rate sr and channel count for 0 <= j < J,
 * 0.0 outside; its binary32 value is what pdmp3_amd_bulk_decode_clips_audio produces.
 * Framing.  Nw = win_length samples (2 .. 1024), H = hop (1 .. Nw).  The DFT length N is the least power of two >= Nw with
 * round_to_power_of_two, else N = Nw (an odd Nw is then refused).  A clip is (stream, index, start), start >= 0.  Frame f is
 *     s[n] = scale * y[start + f H + n],   0 <= n < Nw:
 * left-aligned; samples outside [0, J) are zeros, nothing is reflected.
 * Steps.
 *  1. remove_dc_offset:  a[n] = s[n] - (1 / Nw) sum s      (off: a = s)
 *  2. raw energy:        E = sum a[n]^2                    (behind step 1, in front of step 3)
 *  3. pre-emphasis, rho = preemphasis_coefficient in [0, 1]:  p[n] = a[n] - rho a[n - 1] for n >= 1, p[0] = a[0] - rho a[0]
 *  4. window w[n], t = 2 pi n / (Nw - 1):  0 povey (0.5 - 0.5 cos t)^0.85;  1 hanning 0.5 - 0.5 cos t;  2 hamming
 *     0.54 - 0.46 cos t;  3 rectangular 1;  4 blackman b - 0.5 cos t + (0.5 - b) cos 2t, b = blackman_coeff
 *  5. X[k] = sum over n < Nw of w[n] p[n] e^(-2 pi i k n / N) for k = 0 .. N / 2 - 1 (the Nyquist bin is not used);
 *     P[k] = Re^2 + Im^2
 *  6. mel(f) = 1127 ln(1 + f / 700), lo = low_freq, hi = high_freq (<= 0: that offset from sr / 2), 0 <= lo < hi <= sr / 2;
 *     d = (mel(hi) - mel(lo)) / (n_mels + 1), l_m = mel(lo) + m d, c_m = l_m + d, r_m = l_m + 2 d,
 *     W[m, k] = max(0, min((mel(k sr / N) - l_m) / (c_m - l_m), (r_m - mel(k sr / N)) / (r_m - c_m))),  M[m] = sum_k W[m, k] P[k]
 *  7. out_mode 0: M;  1 (use_log_fbank): ln max(M, eps), eps = 2^-23 (binary32's epsilon, as Kaldi and torchaudio)
 *  8. use_energy: one column more, ln max(E, eps) -- where energy_floor > 0 the larger of that and ln energy_floor --, in
 *     front of the mel columns, behind them with htk_compat; out_mode 0: E itself.  D = n_mels + use_energy.
 *  9. subtract_mean: from every column of a (clip, channel) its mean over the frames f < valid[k] is subtracted, from the
 *     frames at and behind valid[k] too; nothing where valid[k] = 0.
 * scale must be finite and > 0: 1.0 gives what kaldi.fbank gives on the audio call's [-1, 1) batch, 32768.0 Kaldi's int16
 * convention.  Not offered, and refused by pdmp3_amd_fbank_check when asked for: dither (random), use_power = false,
 * raw_energy = false, VTLN (vtln_warp other than 1), snip_edges = false (Kaldi reflects at the edges then; a clip here has the
 * stream's real neighbours, so a caller moves `start` instead).
 * valid[k] = the frames wholly inside [0, J): 0 if J - start < Nw, else min(F, (J - start - Nw) / H + 1).  Frames behind it
 * are the transform of whatever real samples they cover, and zeros.  With start = 0 and F = valid the rows are Kaldi's
 * snip_edges = true output of the whole stream.
 * Steps 1, 3, 4 and the zero padding to N are linear maps on a frame: they are folded into the DFT table on the host in
 * binary64 and rounded once to binary32 (pdmp3_amd_fbank_table); the filterbank likewise.  The GPU multiplies and adds in
 * binary32 (v_mfma_f32_16x16x4_f32); the energy is a two-pass mean / sum of squares in binary32. */
typedef struct {
  long rate; int channels; int width; double rolloff;   /* as pdmp3_amd_audio_spec (rate 0: the clips' common own rate) */
  int win_length, hop, n_mels;
  int round_to_power_of_two, remove_dc_offset;          /* 0 / 1 */
  double preemphasis;                                   /* rho */
  int window;                                           /* 0 povey, 1 hanning, 2 hamming, 3 rectangular, 4 blackman */
  double blackman_coeff;
  double low_freq, high_freq;
  int out_mode;                                         /* 0 power, 1 ln */
  int use_energy, htk_compat;                           /* 0 / 1 */
  double energy_floor;                                  /* >= 0; 0: none */
  int subtract_mean;                                    /* 0 / 1 */
  double scale;                                         /* > 0 */
  long long n_frames;
  /* what is not offered: each must be 0 (vtln_warp: 0 or 1.0) */
  double dither, vtln_warp;
  int no_power, no_raw_energy, no_snip_edges;
} pdmp3_amd_fbank_spec;
/* Planning, plain C (host tests reach all of it).  0 when the spec's numbers are acceptable at sampling frequency sr, else -1:
 * win_length outside 2 .. 1024 (or odd without round_to_power_of_two), hop outside 1 .. win_length, n_mels outside 1 .. 256,
 * preemphasis outside [0, 1], an unknown window / out_mode / flag, blackman_coeff not finite, low_freq < 0, hi > sr / 2,
 * low_freq >= hi, energy_floor < 0 or not finite, scale not finite or not > 0 (or one whose table leaves binary32),
 * n_frames < 0, and every option that is not offered. */
int pdmp3_amd_fbank_check(const pdmp3_amd_fbank_spec* spec, long sr);
/* N of (win_length, round_to_power_of_two), or -1 */
int pdmp3_amd_fbank_dft_length(int win_length, int round_to_power_of_two);
/* The folded table in k_clip_mel's B-operand layout: *rows = Nw rounded up to 4 rows of *cols = 2 Kp floats, Kp = N / 2
 * rounded up to 16; Re at column k, Im at Kp + k for k < N / 2, 0 in the padding.  With c[n] = w[n] cos(2 pi (k n mod N) / N)
 * (Im: -w[n] sin) and c[Nw] = 0:  d[n] = c[n] - rho c[n + 1], d[0] loses rho c[0] besides, T[n] = scale (d[n] - (sum d) / Nw)
 * (no sum term without remove_dc_offset); binary64, rounded once.  Only the spec's framing, window, rho, DC and scale fields
 * are read.  Returns rows * cols and writes min(that, cap) floats; -1 on a bad argument. */
long long pdmp3_amd_fbank_table(const pdmp3_amd_fbank_spec* spec, float* table, size_t cap, int* rows, int* cols);
/* The filterbank, dense [n_mels][N / 2], binary64 rounded once (n_dft even, 2 .. 1024).  Returns n_mels * N / 2 and writes
 * min(that, cap) floats; -1 on a bad argument. */
long long pdmp3_amd_fbank_filterbank(long sr, int n_dft, int n_mels, double low_freq, double high_freq, float* w, size_t cap);
/* valid[k] of a clip at `start` of a stream of J samples; -1 on a bad argument */
long long pdmp3_amd_fbank_valid(long long J, long long start, int win_length, int hop, long long n_frames);
/* What a workgroup of k_clip_fbank takes, as the call itself decides it: *tile frames (32, or 16 where 32 need more than 64 KB
 * of LDS), *row_pad (hop + row_pad = 2 mod 32) and the LDS bytes: the span in chunks of hop + row_pad floats or the mel tile
 * [mels16][tile + 1] where that is larger, then the powers [tile][Kp + 2] (a row's first spare float holds the frame's
 * energy).  More than 64 KB at a tile of 16: the static-array kernel.  0, or -1 on a bad argument.  Pointers may be NULL. */
int pdmp3_amd_fbank_tile(int win_length, int n_dft, int hop, int n_mels, int* tile, int* row_pad, unsigned* lds_bytes);
/* Row k receives channel c's [n_frames][D] floats at dst + c * chan_stride (pdmp3_amd_audio_clip; chan_stride >= n_frames * D).
 * The call decodes the span from `start` on, (F - 1) H + Nw samples, with pdmp3_amd_bulk_decode_clips_audio itself into a
 * device stage the decoder owns, and k_clip_fbank (csrc/fbank.hip) writes the rows; host destinations go through a second
 * stage.  Synchronous.  Returns, refuses (per clip in valid[k]) and counts as pdmp3_amd_bulk_decode_clips_mel; -1 also where
 * pdmp3_amd_fbank_check says so. */
int pdmp3_amd_bulk_decode_clips_fbank(pdmp3_amd_bulk* b, const pdmp3_amd_audio_clip* clips, int n_clips, const pdmp3_amd_fbank_spec* spec,
                                      long long* valid);

/* ---- Kaldi-style MFCC features of clips ----
 * Kaldi's `mfcc` front end (torchaudio.compliance.kaldi.mfcc's options, by their names there) on the same resampled signal:
 * K clips as one planar float32 batch [K][C][F][num_ceps], frames by cepstra, cepstra innermost.  New entry points only;
 * nothing any entry point above returns changes.
 *
 * Signal, framing and steps 1 .. 6 and 8 are the filterbank call's above (framing, DC removal, raw energy, pre-emphasis,
 * window, DFT without the Nyquist bin, the mel triangles, the energy column's value), with the same options, the same scale
 * and the same valid[k].  Then, with Nm = n_mels (num_mel_bins), Q = cepstral_lifter:
 *     L[m]   = ln max(M[m], eps),  eps = 2^-23                  (always the logarithm: there is no power mode)
 *     B[c,m] = sqrt(1 / Nm) for c = 0;  sqrt(2 / Nm) cos(pi (m + 1/2) c / Nm) for 1 <= c < num_ceps
 *     l[c]   = 1 + (Q / 2) sin(pi c / Q);  Q = 0: l[c] = 1
 *     C[c]   = l[c] * sum_m B[c,m] L[m]
 *     use_energy:    C[0] = max(ln max(E, eps), ln energy_floor)  (step 8; it replaces C0, a frame keeps num_ceps columns)
 *     htk_compat:    C[0] moves behind C[num_ceps - 1]; without use_energy it is multiplied by sqrt(2) on the way
 *     subtract_mean: every column minus its mean over the frames f < valid[k]   (as step 9)
 * Conditions: 1 <= num_ceps <= n_mels; cepstral_lifter finite and >= 0; out_mode must be 1; everything pdmp3_amd_fbank_check
 * refuses is refused here too (dither, use_power = false, raw_energy = false, VTLN, snip_edges = false).  torchaudio's defaults
 * for kaldi.mfcc: num_ceps 13, num_mel_bins 23, cepstral_lifter 22.0, use_energy false, energy_floor 1.0, low_freq 20,
 * high_freq 0.
 * The lifter, the sqrt(2) and the column order are linear: they are folded into the DCT table on the host in binary64 and
 * rounded once to binary32 (pdmp3_amd_mfcc_dct_table).  The GPU takes the logarithm of the mel tile where the filterbank left
 * it and multiplies it by the table in binary32 (v_mfma_f32_16x16x4_f32); the log-mel values never leave the compute unit. */
typedef struct {
  pdmp3_amd_fbank_spec fbank;                           /* out_mode must be 1 */
  int num_ceps;                                         /* 1 .. fbank.n_mels */
  double cepstral_lifter;                               /* Q >= 0; 0: no lifter */
} pdmp3_amd_mfcc_spec;
/* 0 when pdmp3_amd_fbank_check accepts spec->fbank at sr, its out_mode is 1, 1 <= num_ceps <= n_mels and cepstral_lifter is
 * finite and >= 0; else -1. */
int pdmp3_amd_mfcc_check(const pdmp3_amd_mfcc_spec* spec, long sr);
/* The folded DCT table as k_clip_mfcc reads it: *rows = mels16 (n_mels rounded up to 16) rows of *cols = ceps16 (num_ceps
 * rounded up to 16) floats, Bt[m][col] = l[c] s B[c,m] where c is the cepstral index output column col holds (col itself;
 * with htk_compat columns 0 .. num_ceps - 2 hold c = 1 .. num_ceps - 1 and the last holds c = 0) and s = sqrt(2) only for
 * c = 0 with htk_compat and without use_energy; binary64, rounded once.  The column that holds the energy (use_energy) is
 * all zeros, and so is the padding.  Only n_mels, use_energy, htk_compat, num_ceps and cepstral_lifter are read.  Returns
 * rows * cols and writes min(that, cap) floats; -1 on a bad argument. */
long long pdmp3_amd_mfcc_dct_table(const pdmp3_amd_mfcc_spec* spec, float* table, size_t cap, int* rows, int* cols);
/* What a workgroup of k_clip_mfcc takes, as the call itself decides it: as pdmp3_amd_fbank_tile, but behind the first region
 * lie max(Kp + 2, ceps16 + 1) floats a frame: the cepstra [tile][ceps16 + 1] take the place of the powers [tile][Kp + 2]
 * (a row's spare float holds the frame's energy in both) and can be the larger of the two.  0, or -1 on a bad argument. */
int pdmp3_amd_mfcc_tile(int win_length, int n_dft, int hop, int n_mels, int num_ceps, int* tile, int* row_pad, unsigned* lds_bytes);
/* Row k receives channel c's [n_frames][num_ceps] floats at dst + c * chan_stride (chan_stride >= n_frames * num_ceps).
 * Everything else -- the audio call in front, the stages, host destinations, the per-clip refusals in valid[k], rate 0 /
 * channels 0, width, rolloff, the counts, n_clips = 0 and n_frames = 0 -- as pdmp3_amd_bulk_decode_clips_fbank; k_clip_mfcc
 * (csrc/mfcc.hip) writes the rows.  -1 also where pdmp3_amd_mfcc_check says so. */
int pdmp3_amd_bulk_decode_clips_mfcc(pdmp3_amd_bulk* b, const pdmp3_amd_audio_clip* clips, int n_clips, const pdmp3_amd_mfcc_spec* spec,
                                     long long* valid);

/* ---- The short-time Fourier transform of clips ----
 * What the three feature calls above compute first and discard: K clips as one planar float32 batch [K][C][bins][F], frames
 * innermost, complex or as magnitude, power or its logarithm.  New entry points only; nothing above returns anything else.
 *
 * Signal, clip, frame position, valid.  As the log-mel call: y_c[j] is the binary32 output of
 * pdmp3_amd_bulk_decode_clips_audio at the requested rate and channel count for 0 <= j < J and 0.0 outside; frame f of a clip
 * at `start` is centred on sample start + f H and reads y[start + f H - N / 2 + n], 0 <= n < N; NO reflection, real
 * neighbours inside the stream; valid[k] = clamp(ceil((J - start) / H), 0, F).  This is torch.stft(center=False) applied to
 * the span from start - N / 2 on, and center=True with pad_mode="constant" at a stream's two ends only.
 * Window.  N = n_fft is even, 16 .. 1024; win_length Nw, 1 <= Nw <= N (0: N); `window` points to Nw binary32 values of the
 * caller's (finite), NULL: the periodic Hann window of Nw, 0.5 - 0.5 cos(2 pi i / Nw).  The frame's window w[n] is `window`
 * at n = (N - Nw) / 2 + i (integer division, as torch.stft) and 0 elsewhere.
 * Transform.  bins = N / 2 + 1;  X[f, k] = s sum over n < N of w[n] y[start + f H - N / 2 + n] e^(-2 pi i k n / N),
 * s = N^(-1/2) with `normalized`, else 1.
 * Output.  out_mode 0 complex: [K][C][bins][F][2], Re and Im interleaved -- the memory of a [K, C, bins, F] complex64
 * tensor; 1 magnitude sqrt(Re^2 + Im^2); 2 power Re^2 + Im^2; 3 ln max(power, floor); 4 log10 max(power, floor); modes 1 .. 4
 * are [K][C][bins][F].  floor > 0 is rounded to binary32 first and is read in modes 3 and 4 only.  Frames behind the
 * stream's end are the transform of zeros.
 * The coefficients s w[n] cos and -s w[n] sin are computed on the host in binary64 from the binary32 window values and
 * rounded once; the GPU multiplies and adds in binary32 (v_mfma_f32_16x16x4_f32), the square root is correctly rounded.
 * Not offered here: n_fft above 1024 (the transform is a matrix product, N^2 a frame; n_fft 2048 and 4096 are served by the
 * two-stage calls below, pdmp3_amd_stft_long_*), the inverse transform, reflection at a stream's ends, a frames-major
 * layout. */
typedef struct {
  long rate; int channels; int width; double rolloff;   /* as pdmp3_amd_mel_spec */
  int n_fft, hop, win_length;                           /* win_length 0 = n_fft */
  const float* window;                                  /* win_length values, NULL = periodic Hann */
  int normalized;                                       /* 0, or 1: scaled by n_fft^(-1/2) */
  long long n_frames;
  int out_mode;                                         /* 0 complex, 1 magnitude, 2 power, 3 ln, 4 log10 */
  double floor;                                         /* modes 3 and 4: > 0 */
} pdmp3_amd_stft_spec;
/* 0 when the spec's numbers are acceptable at sampling frequency sr, else -1: n_fft odd or outside 16 .. 1024, hop outside
 * 1 .. n_fft, win_length outside 0 .. n_fft, a window value that is not finite, normalized not 0 or 1, out_mode unknown,
 * n_frames < 0, and in modes 3 and 4 a floor not > 0 (or smaller than binary32's least normal number). */
int pdmp3_amd_stft_check(const pdmp3_amd_stft_spec* spec, long sr);
/* The folded table in pdmp3_amd_mel_dft_table's layout: *rows = n_fft rounded up to 4 rows of *cols = 2 Kp floats, Kp = bins
 * rounded up to 16; row n holds s w[n] cos(2 pi k n / N) at column k and -s w[n] sin(2 pi k n / N) at column Kp + k, the
 * angle reduced as the integer k n mod N; the rows outside the window's support and all padding are exactly 0.  With a NULL
 * window, win_length = n_fft and normalized = 0 it is pdmp3_amd_mel_dft_table(n_fft) bit for bit.  Only n_fft, win_length,
 * window and normalized are read.  Returns rows * cols and writes min(that, cap) floats; -1 on a bad argument. */
long long pdmp3_amd_stft_table(const pdmp3_amd_stft_spec* spec, float* table, size_t cap, int* rows, int* cols);
/* What a workgroup of k_clip_stft takes, the function the call itself uses: *tile frames (32 where the LDS below fits 64 KB,
 * else 16), *row_pad (hop + row_pad = 2 mod 32) and the LDS bytes: the tile's span in chunks of hop + row_pad floats, rounded
 * up to 4 floats, then four staging tiles of (out_mode 0 ? 2 : 1) x 16 x (tile + 4) floats.  A tile of 16 frames that needs
 * more than 64 KB runs in a kernel with a static array (k_clip_stft_big).  0, or -1 on a bad argument.  Pointers may be NULL. */
int pdmp3_amd_stft_tile(int n_fft, int hop, int out_mode, int* tile, int* row_pad, unsigned* lds_bytes);
/* Row k receives channel c's [bins][n_frames] floats (mode 0: [bins][n_frames][2]) at dst + c * chan_stride
 * (pdmp3_amd_audio_clip; chan_stride >= that many floats).  Everything else -- the
 * audio call in front, the stages, host destinations, the per-clip refusals in valid[k], rate 0 / channels 0, width, rolloff,
 * the counts, n_clips = 0 and n_frames = 0 -- as pdmp3_amd_bulk_decode_clips_mel; k_clip_stft (csrc/stft.hip) writes the
 * rows.  The decoder keeps the folded tables of the last PDMP3_STFT_TABLES distinct (n_fft, win_length, normalized, window
 * contents) and drops the least recently used one for a new one.  -1 also where pdmp3_amd_stft_check says so. */
#define PDMP3_STFT_TABLES 4
int pdmp3_amd_bulk_decode_clips_stft(pdmp3_amd_bulk* b, const pdmp3_amd_audio_clip* clips, int n_clips, const pdmp3_amd_stft_spec* spec,
                                     long long* valid);

/* ---- The short-time Fourier transform of clips at n_fft 2048 and 4096 ----
 * The definition of the section above, unchanged, on a wider domain: the same spec struct, signal, clip, framing, valid[k],
 * window rules (win_length 0 .. N, the caller's binary32 window or periodic Hann, centred as torch.stft centres it),
 * `normalized`, the five output modes with their floor rules and the same layouts, bins = N / 2 + 1.  What differs: n_fft is
 * 2048 or 4096 only (hop 1 .. n_fft); a window length that is no power of two -- 1764, 1920 -- is a shorter window inside
 * the next power of two.  New entry points only: the calls above keep refusing n_fft = 2048.
 * The arithmetic.  N = 64 N2 (N2 = 32 or 64), n = N2 n1 + n2, k = k1 + 64 k2; all tables are computed on the host in
 * binary64, every angle reduced as an integer modulo its period, and rounded once to binary32.
 *   0. wt[n] = fl32(s w[n]), 0 outside the window's support; xw[n] = wt[n] y[n], one binary32 product a sample.
 *   1. Y[n2][k1] = sum over n1 < 64 of xw[N2 n1 + n2] e^(-2 pi i n1 k1 / 64), k1 < 64: real by complex on
 *      v_mfma_f32_16x16x4_f32, one fused multiply-add chain for Re and one for Im, n1 ascending.
 *   2. Z = Y T, T[n2][k1] = fl32(e^(-2 pi i n2 k1 / N)):  Zr = fma(Yr, Tr, -(Yi Ti)),  Zi = fma(Yr, Ti, Yi Tr).
 *   3. X[k1 + 64 k2] = sum over n2 < N2 of Z[n2][k1] e^(-2 pi i n2 k2 / N2), k2 < N2 / 2: Re and Im are each ONE fused
 *      multiply-add chain over the 2 N2 real terms in the order n2 ascending, Zr's term before Zi's: with a = 2 pi n2 k2 / N2,
 *      Re takes Zr cos a, then Zi sin a; Im takes Zr (-sin a), then Zi cos a.  The Nyquist bin N / 2 is the same chain at
 *      k1 = 0, k2 = N2 / 2, whose coefficients are exact: (-1)^n2 for the cosine, 0 for the sine.
 *   4. What is stored is section 13's: the pair, the correctly rounded square root, the power fma(Im, Im, Re Re), logf, log10f.
 * Every frame's values come from the same chains whatever its place in a tile or clip, and Im of bins 0 and N / 2 is exactly
 * zero (the sine coefficients there are exact zeros). */
/* 0 when the spec's numbers are acceptable at sampling frequency sr, else -1: as pdmp3_amd_stft_check, with n_fft 2048 or
 * 4096 only. */
int pdmp3_amd_stft_long_check(const pdmp3_amd_stft_spec* spec, long sr);
/* The four tables of the spec's frame, one behind the other as the kernel reads them, with their shapes in shapes[8] (rows,
 * columns of each; may be NULL): wt [1][N]; the 64-point DFT [64][128], cos(2 pi n1 k1 / 64) at column k1 and -sin at column
 * 64 + k1; the N2-point half DFT [2 N2][N2], row 2 n2 + part, columns k2 < N2 / 2 Re's coefficients (cos a for part 0, sin a
 * for part 1) and columns N2 / 2 + k2 Im's (-sin a, cos a); the twiddles [N2][128], cos(2 pi n2 k1 / N) at column k1 and
 * -sin at column 64 + k1.  Only n_fft, win_length, window and normalized are read.  Returns the floats of all four and
 * writes min(that, cap) of them; -1 on a bad argument. */
long long pdmp3_amd_stft_long_tables(const pdmp3_amd_stft_spec* spec, float* tables, size_t cap, int* shapes);
/* What a workgroup of k_clip_stft_long takes, the function the call itself uses.  A workgroup of eight waves takes *tile
 * frames and 16 of the 64 values of k1: 16 frames where the LDS below fits PDMP3_MEL_LDS_MAX (include/pdmp3_hip.h), else 8,
 * else 4.  The LDS bytes: a first region of max((tile - 1) hop + n_fft, (out_mode 0 ? 2 : 1) x 16 x N2 / 2 x (tile + 1))
 * floats rounded up to 4 -- the tile's span, later the staging tile -- then Z, tile x N2 x 32 floats.  *row_pad is 0: the
 * span lies plain in LDS.  Every plan is above 64 KB and runs on a static array.  0, or -1 on a bad argument.  Pointers may
 * be NULL. */
int pdmp3_amd_stft_long_plan(int n_fft, int hop, int out_mode, int* tile, int* row_pad, unsigned* lds_bytes);
/* pdmp3_amd_bulk_decode_clips_stft in everything -- rows, destinations, the audio call in front, the stages, the per-clip
 * refusals in valid[k], rate 0 / channels 0, the counts, n_clips = 0 and n_frames = 0 -- with the check above and
 * k_clip_stft_long (csrc/stft_long.hip) writing the rows.  The decoder makes the three tables that depend on n_fft alone
 * once per n_fft and keeps them for its life (two sets at most); wt is filled on every call.  -1 also where
 * pdmp3_amd_stft_long_check says so. */
int pdmp3_amd_bulk_decode_clips_stft_long(pdmp3_amd_bulk* b, const pdmp3_amd_audio_clip* clips, int n_clips, const pdmp3_amd_stft_spec* spec,
                                          long long* valid);

/* ---- log-mel features of clips at n_fft 2048 and 4096 ----
 * The mel spectrogram of the spectrum above without the spectrum leaving the device's compute units: librosa's 2048 / 512
 * with 128 bands and its like.  Signal, clip, framing, valid[k] and layout are pdmp3_amd_bulk_decode_clips_mel's: frame f of a
 * clip at `start` reads y[start + f hop - N / 2 + n], no reflection, zeros outside the stream; planar float32
 * [K, C, n_mels, F], frames innermost, rows of K and C may be strided.  The window is the transform's wt above with s = 1
 * (there is no `normalized`); P[f][k] = Re^2 + Im^2 of its X, as fma(Im, Im, Re Re); W is pdmp3_amd_mel_filterbank's at
 * N / 2 + 1 bins; M = W P, each M[f][m] one fused multiply-add chain in one fixed order of the bins, the same for every frame.
 * out_mode 0 (power), 1 (ln max(M, floor)) and 2 (log10 max(M, floor)).  out_mode 3 (Whisper's normalisation) is refused:
 * its front end is 400 / 160, and it would bring the row-maximum atomics and the finishing launch for no user at these
 * lengths.  The Nyquist bin is never computed: f_max <= sr / 2 and the last band's upper edge is f_max itself, so its weight
 * is exactly 0 in every filterbank the check accepts. */
typedef struct pdmp3_amd_mel_long_spec {
  pdmp3_amd_mel_spec mel;     /* pdmp3_amd_mel_spec's fields and meanings; mel.n_fft is 2048 or 4096, mel.hop 1 .. n_fft */
  int win_length;             /* 0 = n_fft, else 1 .. n_fft, centred as torch.stft centres it */
  const float* window;        /* NULL: periodic Hann of win_length; else win_length binary32 values of the caller's */
} pdmp3_amd_mel_long_spec;
/* 0 when the spec's numbers are acceptable at sampling frequency sr, else -1: pdmp3_amd_mel_check's limits on n_mels, f_min,
 * f_max, scale, norm, floor and n_frames, n_fft 2048 or 4096, hop 1 .. n_fft, out_mode 0 .. 2, win_length and the window's
 * values as pdmp3_amd_stft_long_check takes them. */
int pdmp3_amd_mel_long_check(const pdmp3_amd_mel_long_spec* spec, long sr);
/* pdmp3_amd_mel_filterbank on this domain: dense [n_mels][n_fft / 2 + 1], binary64 rounded once.  Returns the floats and
 * writes min(that, cap); -1 on a bad argument, nothing written. */
long long pdmp3_amd_mel_long_filterbank(long sr, int n_fft, int n_mels, double f_min, double f_max, int scale, int norm, float* w, size_t cap);
/* The same weights as the kernel reads them: [n_fft / 2][n_mels rounded up to 16] (*rows, *cols; may be NULL), the row of bin
 * k = 16 kt + k1l + 64 k2 at 8 N2 kt + slot(k1l, k2) (csrc/mel_long_core.h), zeros in the bands' padding, bin n_fft / 2 left
 * out.  Returns the floats and writes min(that, cap); -1 on a bad argument, nothing written. */
long long pdmp3_amd_mel_long_operand(long sr, int n_fft, int n_mels, double f_min, double f_max, int scale, int norm, float* op, size_t cap,
                                     int* rows, int* cols);
/* What a workgroup of k_clip_mel_long takes, the function the call itself uses: *tile frames -- 16 where the LDS below fits
 * PDMP3_MEL_LDS_MAX (include/pdmp3_hip.h), else 8, else 4 -- and all bins.  The LDS bytes: the tile's span,
 * (tile - 1) hop + n_fft floats rounded up to 4, which stays; Z, tile x N2 x 32 floats; the powers of one tile of k1,
 * tile x (8 N2 + 2) floats.  *row_pad is 0.  Every plan is above 64 KB and runs on a static array.  0, or -1 on a bad
 * argument.  Pointers may be NULL. */
int pdmp3_amd_mel_long_plan(int n_fft, int hop, int n_mels, int* tile, int* row_pad, unsigned* lds_bytes);
/* pdmp3_amd_bulk_decode_clips_stft_long's course -- rows through the audio call, destinations, the stages, the per-clip
 * refusals in valid[k], rate 0 / channels 0, the counts, n_clips = 0 and n_frames = 0 -- with the check above and
 * k_clip_mel_long (csrc/mel_long.hip) writing the rows.  The transform's tables are that call's; the filterbank operand is
 * made once per (sr, n_fft, n_mels, f_min, f_max, scale, norm) and kept for the decoder's life.  -1 also where
 * pdmp3_amd_mel_long_check says so. */
int pdmp3_amd_bulk_decode_clips_mel_long(pdmp3_amd_bulk* b, const pdmp3_amd_audio_clip* clips, int n_clips, const pdmp3_amd_mel_long_spec* spec,
                                         long long* valid);

/* ---- The constant-Q transform of clips ----
 * What music models take besides the mel spectrogram: K clips as one planar float32 batch [K][C][n_bins][F], frames
 * innermost, complex or as magnitude, power or its logarithm.  New entry points only; nothing above returns anything else.
 *
 * Signal, clip, frame position, valid, destinations.  Section 13's: y_c[j] is the binary32 output of
 * pdmp3_amd_bulk_decode_clips_audio at the requested rate sr and channel count for 0 <= j < J and 0.0 outside; frame f of a
 * clip at `start` is centred on sample start + f H; NO reflection, samples outside the stream are zeros;
 * valid[k] = clamp(ceil((J - start) / H), 0, F).  Rows of K and C may be strided.
 * Bins.  With B = bins_per_octave and k = 0 .. n_bins - 1:
 *   f_k = fmin 2^(k / B);  Q = filter_scale / (2^(1 / B) - 1);  L_k = Q sr / f_k (real);  h_k = floor(L_k / 2);
 *   N_k = 2 h_k + 1 (odd: the filter is centred on the frame's centre sample);
 *   g_k[m] = 0.5 - 0.5 cos(2 pi (m + h_k) / N_k), m = -h_k .. h_k (the periodic Hann window of N_k);
 *   s_k = n_k a_k;  n_k: norm 0: 1, norm 1: 1 / sum_m g_k[m], norm 2: 1 / sqrt(sum_m g_k[m]^2);
 *                   a_k: scale 0: 1, scale 1: sqrt(L_k), scale 2: L_k;
 *   C[f, k] = s_k sum over m = -h_k .. h_k of g_k[m] y[start + f H + m] e^(-2 pi i f_k m / sr).
 * The phase is referred to the frame's centre.  norm 1, scale 1 is the convention of librosa's cqt(norm=1, scale=True) -- L1
 * filters times sqrt(length); norm 1, scale 0 gives |C| = a / 2 for a sinusoid of amplitude a at f_k.  The definition is the
 * formula above, evaluated in full at the one rate sr -- not librosa's multirate approximation of it: no agreement with
 * librosa is promised beyond the convention.
 * Output.  out_mode 0 complex: [K][C][n_bins][F][2], Re and Im interleaved -- the memory of a complex64 tensor; 1 magnitude,
 * the correctly rounded sqrt(Re^2 + Im^2); 2 power fma(Im, Im, Re Re); 3 ln max(power, floor); 4 log10 max(power, floor).
 * The floor rules are section 13's.
 * The coefficients s_k g_k[m] cos(2 pi f_k m / sr) and -s_k g_k[m] sin(..) are computed on the host in binary64 and rounded
 * once to binary32; the angle is reduced first: x = m f_k / sr in binary64 (one product, one quotient), x - floor(x) in
 * [0, 1), then times 2 pi.  The GPU multiplies and adds in binary32 (v_mfma_f32_16x16x4_f32).
 * Not offered: windows other than Hann, variable-Q (gamma), fmin per clip, the inverse transform, the multirate form,
 * reflection at a stream's ends. */
#define PDMP3_CQT_MAX_LEN 32767       /* N_0, the longest filter, at most */
#define PDMP3_CQT_SPLIT_ROWS 512      /* a tile of 16 bins with this many rows or more is cut into PDMP3_CQT_SEGMENTS */
#define PDMP3_CQT_SEGMENTS 8
#define PDMP3_CQT_TABLES 4
typedef struct {
  long rate; int channels; int width; double rolloff;   /* as pdmp3_amd_mel_spec */
  int hop;
  double fmin;
  int n_bins, bins_per_octave;
  double filter_scale;
  int norm, scale;                                      /* 0 .. 2 each, above */
  long long n_frames;
  int out_mode;                                         /* 0 complex, 1 magnitude, 2 power, 3 ln, 4 log10 */
  double floor;                                         /* modes 3 and 4: > 0 */
} pdmp3_amd_cqt_spec;
/* 0 when the spec's numbers are acceptable at sampling frequency sr, else -1: n_bins outside 1 .. 512, bins_per_octave
 * outside 1 .. 96, fmin or filter_scale not finite or not > 0, f_(n_bins - 1) >= sr / 2, N_0 > PDMP3_CQT_MAX_LEN, a shortest
 * filter of fewer than 3 taps (its Hann window is 0), a table of more than 2^22 floats, hop outside 1 .. 8192, norm or scale
 * outside 0 .. 2, out_mode unknown, a floor section 13 refuses, n_frames < 0, a spec whose plan finds no tile that fits the LDS. */
int pdmp3_amd_cqt_check(const pdmp3_amd_cqt_spec* spec, long sr);
/* f_k into f[] and h_k into half[] (either may be NULL), k < n_bins <= cap.  Returns n_bins; -1 where the check refuses the
 * spec or cap < n_bins, nothing written. */
int pdmp3_amd_cqt_lengths(const pdmp3_amd_cqt_spec* spec, long sr, double* f, int* half, size_t cap);
/* The ragged table.  Bins are taken in tiles of 16, ascending k; tile t has tile_rows[t] = N_(16 t) rounded up to 4 rows --
 * the support of its lowest, longest bin -- of 32 floats: Re's coefficient of bin 16 t + j at column j, Im's at column
 * 16 + j.  Row r of tile t stands for m = r - h_(16 t): a shorter bin is centred in its tile, and exact zeros lie outside its
 * own support, in the padding rows and in the padding bins.  The tiles lie one behind the other; tile_offset[t] is tile t's
 * first row.  tile_rows / tile_offset hold (n_bins + 15) / 16 entries (either may be NULL).  Returns the floats of the table
 * and, where table != NULL, writes them all; -1 where the check refuses the spec or table != NULL and cap is short of them,
 * nothing written. */
long long pdmp3_amd_cqt_table(const pdmp3_amd_cqt_spec* spec, long sr, float* table, size_t cap, int* tile_rows, int* tile_offset);
/* What a workgroup of k_clip_cqt takes, the function the call itself uses.  One workgroup of eight waves per (*tile frames,
 * channel, clip): 16 frames where the LDS below fits PDMP3_MEL_LDS_MAX (include/pdmp3_hip.h), else 8, else 4.  The LDS bytes:
 * the tile's span, (*tile - 1) hop + tile_rows[0] samples in chunks of hop + *row_pad floats (hop + row_pad = 2 mod 32),
 * rounded up to 4 floats, then the partial sums, 8 x 2 x 16 x 17 floats.  Up to 64 KB the launch asks for it dynamically,
 * above that the kernel with a static array runs.  The first *n_split tiles -- those of *split_rows = PDMP3_CQT_SPLIT_ROWS
 * rows or more -- are cut into *segments = 8 runs of rows, segment s being rows [s q, min((s + 1) q, R)) with q =
 * ceil(R / 8) rounded up to 4, one a wave, each a chain from +0, the partial sums added as ((p0 + p1) + p2) + ...; every other
 * tile is one chain from +0 over its rows.  0, or -1 where the check refuses the spec.  Pointers may be NULL. */
int pdmp3_amd_cqt_plan(const pdmp3_amd_cqt_spec* spec, long sr, int* tile, int* row_pad, unsigned* lds_bytes, int* split_rows, int* segments,
                       int* n_split);
/* Row k receives channel c's [n_bins][n_frames] floats (mode 0: [n_bins][n_frames][2]) at dst + c * chan_stride.  Everything
 * else -- the audio call in front, the stages, host destinations, the per-clip refusals in valid[k], rate 0 / channels 0,
 * width, rolloff, the counts, n_clips = 0 and n_frames = 0, synchronous -- as pdmp3_amd_bulk_decode_clips_stft; k_clip_cqt
 * (csrc/cqt.hip) writes the rows.  The decoder keeps the tables of the last PDMP3_CQT_TABLES distinct (sr, fmin, n_bins,
 * bins_per_octave, filter_scale, norm, scale) and drops the least recently used one for a new one.  -1 also where
 * pdmp3_amd_cqt_check says so. */
int pdmp3_amd_bulk_decode_clips_cqt(pdmp3_amd_bulk* b, const pdmp3_amd_audio_clip* clips, int n_clips, const pdmp3_amd_cqt_spec* spec,
                                    long long* valid);

/* ---- Chroma features of clips ----
 * Pitch-class profiles, what transcription, chord and key models start from: K clips as one planar float32 batch
 * [K][C][n_chroma][F], frames innermost, straight from MP3 bytes.  New entry points only; nothing above returns anything else.
 *
 * Signal, clip, frame position, valid, destinations and strides are section 16's: real neighbours inside the stream, zeros
 * outside, no reflection.  The bins f_k, the filters g_k, norm, scale and C[f, k] are section 16's, computed by section 16's
 * table and section 16's chains.
 *   q_k[f] is what pdmp3_amd_bulk_decode_clips_cqt stores for bin k at out_mode 1 (or 2): the same binary32 value, bit for
 *     bit, from the same chains.
 *   class(k) = ((k + r / 2) / r + base_class) mod n_chroma in integer division, r = bins_per_octave / n_chroma.  For r = 3
 *     class p collects bins 3 p - 1, 3 p, 3 p + 1 of every octave -- the centring of librosa's cq_to_chroma; for r = 1 it is
 *     k mod n_chroma rotated.
 *   c_p[f] is the binary32 sum of q_k[f] over the bins of class p, k ascending: it starts from the first term and uses plain
 *     additions in this order and no other.  A class without a bin is +0.
 *   The norm d[f] over p = 0 .. n_chroma - 1 ascending: L1 ((c_0 + c_1) + c_2) + ... (no absolute value: every c_p >= 0);
 *     L2 sqrtf, correctly rounded, of the chain s = c_0 c_0, s = fma(c_p, c_p, s); max the exact maximum.
 *   The output is c_p / max(d, (float)norm_floor), one correctly rounded binary32 division, or c_p itself at chroma_norm 0.
 *     A silent frame is exactly +0 in every mode.  There is no threshold and no branch on d other than the max: the result
 *     is a continuous function of the signal.
 * As in section 16 the definition is the formula, not librosa's multirate chroma_cqt: no agreement with librosa is promised
 * beyond the convention.  36 bins an octave from C1 at 22 050 Hz are refused: N_0 = 34 683 > PDMP3_CQT_MAX_LEN, which
 * pdmp3_amd_cqt_check says already; 36 an octave from C2 (N_0 = 17 341) and 24 an octave from C1 (N_0 = 23 011) fit.
 * Not offered: octave weighting windows and a caller's fold matrix, thresholds, chroma_stft, harmonic stacks, tuning
 * estimation. */
typedef struct {
  pdmp3_amd_cqt_spec cqt;   /* out_mode: 1 = magnitudes are folded, 2 = powers; cqt.floor is not used */
  int n_chroma;             /* 1 .. 96, divides cqt.bins_per_octave; r = bins_per_octave / n_chroma */
  int base_class;           /* 0 .. n_chroma - 1: the class of fmin (0 where fmin is a C) */
  int chroma_norm;          /* 0 none, 1 L1, 2 L2, 3 max */
  double norm_floor;        /* > 0, a normal binary32 number; used where chroma_norm != 0 */
} pdmp3_amd_chroma_spec;
/* 0 when the spec's numbers are acceptable at sampling frequency sr, else -1: whatever pdmp3_amd_cqt_check refuses, cqt.out_mode
 * outside {1, 2}, n_chroma outside 1 .. 96 or not a divisor of bins_per_octave, base_class or chroma_norm out of range, where
 * chroma_norm != 0 a norm_floor that is not a positive normal binary32 number once rounded, a spec for which the plan below
 * finds no tile. */
int pdmp3_amd_chroma_check(const pdmp3_amd_chroma_spec* spec, long sr);
/* class(k) into cls[k], k < n_bins <= cap, and the bins of each class into count[p], p < n_chroma (either may be NULL).
 * Returns n_bins; -1 where the check refuses the spec or cls != NULL and cap < n_bins, nothing written. */
int pdmp3_amd_chroma_map(const pdmp3_amd_chroma_spec* spec, long sr, int* cls, size_t cap, int* count);
/* What a workgroup of k_clip_chroma takes, the function the call itself uses: pdmp3_amd_cqt_plan's plan -- table, tile rows,
 * *row_pad, *split_rows, *segments and *n_split are that function's -- with more LDS.  The LDS floats: the tile's span as
 * there; from *class_at on the eight waves' partial sums, 8 x 2 x 16 x 17; from *q_at = *class_at + 4352 on the plane of the
 * frame tile's values q, [n_bins rounded up to 16][17].  The folded classes, [n_chroma][17] floats, lie OVER the partial sums,
 * from *class_at on: they are written behind the workgroup barrier that follows every wave's last read of the sums, and 96 x
 * 17 <= 4352.  *tile is 16 frames where all of this fits PDMP3_MEL_LDS_MAX, else 8, else 4 -- so it may be smaller than the
 * constant-Q call's at the same spec; up to 64 KB the launch asks for the LDS dynamically, above that the kernel with a
 * static array runs.  0, or -1 where the check refuses the spec.  Pointers may be NULL. */
int pdmp3_amd_chroma_plan(const pdmp3_amd_chroma_spec* spec, long sr, int* tile, int* row_pad, unsigned* lds_bytes, int* split_rows, int* segments,
                          int* n_split, unsigned* q_at, unsigned* class_at);
/* Row k receives channel c's [n_chroma][n_frames] floats at dst + c * chan_stride.  Everything else as
 * pdmp3_amd_bulk_decode_clips_cqt, whose cache of tables this call shares (a chroma call and a constant-Q call of the same
 * geometry use one table); k_clip_chroma (csrc/chroma.hip) writes the rows.  -1 also where pdmp3_amd_chroma_check says so. */
int pdmp3_amd_bulk_decode_clips_chroma(pdmp3_amd_bulk* b, const pdmp3_amd_audio_clip* clips, int n_clips, const pdmp3_amd_chroma_spec* spec,
                                       long long* valid);

/* ---- Loudness of clips (ITU-R BS.1770 / EBU R128) ----
 * The integrated loudness of each clip and its normalisation to a target level, on the GPU while the resampled signal is in
 * device memory: audio [K][C][T] float32, stats [K][8] float32 and optionally momentary [K][Jmax] float32.  New entry points
 * only; nothing above returns anything else.  With `target` unset the audio is pdmp3_amd_bulk_decode_clips_audio's bit for bit.
 * What ffmpeg's ebur128 / loudnorm, libebur128, pyloudnorm and torchaudio.functional.loudness compute.  The definition, to be
 * evaluated in binary64:
 *
 * 1. Signal.  x_c[t], c < C, t < T = n_samples, is the row pdmp3_amd_bulk_decode_clips_audio returns for the same clip, rate,
 *    channels, width and rolloff: binary32 values with zeros behind the stream's end.  The zeros are measured as the silence
 *    they are.
 * 2. K-weighting.  y = H2(H1(x)), two biquads, both from rest at t = 0 of the row: a clip is measured as a file holding just
 *    that clip would be.  The coefficients at rate fs follow libebur128's parametrisation, with K = tan(pi f0 / fs) and
 *    a0 = 1 + K/Q + K^2.
 *    Shelf H1: f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196, Vh = 10^(G/20),
 *      Vb = Vh^0.4996667741545416; b = [(Vh + Vb K/Q + K^2), 2 (K^2 - Vh), (Vh - Vb K/Q + K^2)] / a0,
 *      a = [1, 2 (K^2 - 1) / a0, (1 - K/Q + K^2) / a0].
 *    High-pass H2: f0 = 38.13547087602444, Q = 0.5003270373238773; b = [1, -2, 1], a as above.
 *    At 48 kHz these give the standard's table to 1e-15 (1.53512485958697, -2.69169618940638, 1.19839281085285,
 *    -1.69065929318241, 0.73248077421585 and -1.99004745483398, 0.99007225036621), and a full-scale 997 Hz sine on one channel
 *    measures -3.0103 LUFS.  torchaudio's own coefficient formulas (RBJ shelf and high-pass) differ from the table in the
 *    third decimal of a dB; they are not offered.
 * 3. Blocks.  q = (fs + 5) / 10 (integer division) samples per 100 ms.  Sub-block sums s_c[i] = sum over i q <= t < (i + 1) q
 *    of y_c[t]^2 for i < I = T / q: only whole sub-blocks count.  Blocks of 400 ms every 100 ms:
 *    z_j = (1 / 4q) sum_c G_c (s_c[j] + .. + s_c[j + 3]) for j < J = max(0, I - 3); G_c = 1, and G_0 = 2 when C = 1 and
 *    dual_mono.  Block loudness l_j = -0.691 + 10 log10 z_j, and -inf at z_j = 0.
 * 4. Gates.  Absolute gate A = {j : l_j > -70}.  Relative threshold Gamma = -0.691 + 10 log10(mean_A z_j) - 10.  Gated set
 *    Gt = {j in A : l_j > Gamma}.  Integrated loudness L = -0.691 + 10 log10(mean_Gt z_j), and L = -inf when A is empty.
 *    Maximum momentary loudness M = max_j l_j, and -inf when J = 0.  Sample peak P = max_{c,t} |x_c[t]|, exact in binary32.
 * 5. Gain.  g = 1 when target is unset (NaN) or L = -inf.  Otherwise g = 10^((target - L) / 20); if peak_limit > 0 and
 *    g P > peak_limit, then g = peak_limit / P.  g is rounded once to binary32; audio = fl32(x g).  With g = 1 the row is the
 *    audio call's bit for bit.
 * 6. Outputs.  stats[k] = [L, M, P, g, Gamma, J, |A|, |Gt|]; the counts are exact as floats; Gamma = -inf when A is empty.
 *    momentary[k][j] = l_j for j < J, and -inf from J to Jmax = max(0, T / q - 3).  valid is the audio call's.
 * 7. Refusals (-1, nothing written): fs < 8000 or fs > 192000; target finite outside [-70, 0] (or infinite); peak_limit
 *    negative or not finite; dual_mono outside {0, 1}, or set with C = 2; whatever the audio call refuses.
 * A clip of a replay or mixed-format stream is reported as in the other calls, and its rows of audio, stats and momentary stay
 * untouched.  A clip wholly behind the end gives [-inf, -inf, 0, 1, -inf, J, 0, 0], audio exactly +0.
 *
 * Not offered: more than two channels, measuring across clip boundaries with the stream's real history, torchaudio's
 * coefficient variant.  True peak, short-term loudness and loudness range: pdmp3_amd_bulk_decode_clips_r128 below. */
typedef struct {
  long rate; int channels; long long n_samples; int width; double rolloff;      /* pdmp3_amd_audio_spec's */
  double target;            /* LUFS in [-70, 0]; NaN: no gain */
  double peak_limit;        /* > 0: g P <= peak_limit; 0: no limit */
  int dual_mono;            /* 1: a mono clip counts as two channels (G_0 = 2) */
} pdmp3_amd_loudness_spec;
/* 0 when the call would accept these numbers at sampling frequency fs and `channels` (1 or 2) channels, else -1 (item 7) */
int pdmp3_amd_loudness_check(const pdmp3_amd_loudness_spec* spec, long fs, int channels);
/* The two biquads at fs: coef[12] = H1's b[3], a[3], then H2's b[3], a[3] (a[0] = 1).  0, or -1 (fs outside 8000 .. 192000). */
int pdmp3_amd_loudness_coefficients(long fs, double* coef);
/* The tables of the device's filter at fs as the kernels read them (csrc/loudness.hip), for blocks of B = 64 samples and the
 * state s = (z1, z2 of H1, z1, z2 of H2) of the transposed direct form II:  y_block = Hm u_block + O s_in,
 * s_out = Phi s_in + R u_block.  Hm [64][64] binary32, lower-triangular Toeplitz of the impulse response (the kernel reads
 * its column 0); O [64][4] binary32; Phi [4][4] and R [4][64] binary64; pows [70][16] binary64: Phi^k for k = 0 .. 64, then
 * Phi^(64 2^k), k = 1 .. 5.  All made in binary64, Hm and O rounded once.  Pointers may be NULL.  0, or -1. */
int pdmp3_amd_loudness_tables(long fs, float* Hm, float* O, double* Phi, double* R, double* pows);
/* The launch's geometry for rows of n_samples at fs: B (samples of a block), chunk (blocks of a scan chunk), the LDS bytes
 * of a workgroup of k_loud_blocks, q, the chunks of a row, I and J.  Pointers may be NULL.  0, or -1 (fs as above, n_samples
 * outside 0 .. 2^31 - 4). */
int pdmp3_amd_loudness_plan(long fs, long long n_samples, int* B, int* chunk, unsigned* lds_bytes, int* q, long long* n_chunks, long long* I,
                            long long* J);
/* Row k receives channel c's n_samples floats x g at dst + c * chan_stride (pdmp3_amd_audio_clip).  stats: [n_clips][8]
 * floats; momentary: NULL, or [n_clips][Jmax] floats; each host memory or device memory of the decoder's GPU.  Everything else
 * as pdmp3_amd_bulk_decode_clips_audio; the kernels are csrc/loudness.hip's.  -1 also where pdmp3_amd_loudness_check says so. */
int pdmp3_amd_bulk_decode_clips_loudness(pdmp3_amd_bulk* b, const pdmp3_amd_audio_clip* clips, int n_clips, const pdmp3_amd_loudness_spec* spec,
                                         float* stats, float* momentary, long long* valid);

/* ---- True peak, short-term loudness and loudness range of clips (EBU R128, Tech 3341 / 3342) ----
 * The other three descriptors of R128 beside the loudness call's, and the gain held to the true peak: audio [K][C][T] float32,
 * stats [K][16] float32, optionally momentary [K][Jmax] and short_term [K][Jsmax] float32.  New entry points only; the loudness
 * call and everything above return what they return without them.  The definition, to be evaluated in binary64 on the binary32
 * row x_c[t] that pdmp3_amd_bulk_decode_clips_audio returns; everything of the loudness call's items 1-4 holds unchanged: q,
 * s_c[i], I, z_j, l_j, A, Gamma, Gt, L, M, P.
 *
 * 1. Interpolator.  49 taps, factor 4 -- libebur128's own formula, the library whose K-weighting parametrisation the loudness
 *    call follows.  For j = 0 .. 48, m = j - 24: h[j] = sinc4(m) 0.5 (1 - cos(2 pi j / 48)), sinc4(0) = 1, otherwise
 *    sinc4(m) = sin(m pi / 4) / (m pi / 4).  A coefficient with |h[j]| < 1e-6 is exactly 0.  That leaves 37 coefficients: phase 0
 *    is h[24] = 1 alone, a pure delay of 6 samples; phases 1-3 have 12 taps each, c_p[d] = h[4 d + p], d = 0 .. 11.  The sums of
 *    |c_p| are 1, 1.63118, 1.86418, 1.63118; the DC gains 1, 1.00048, 1.00090, 1.00048.  The table of BS.1770-4 Annex 2 is a
 *    different 48-tap design; it is not offered.  The factor is 4 at every accepted rate: libebur128 drops to 2 from 96 kHz up,
 *    this call does not.
 * 2. True peak.  y_c[4 t + p] = sum_d c_p[d] x_c[t - d] for t < T, from rest (x_c[t] = 0 for t < 0), with no flush behind T: a
 *    clip is measured as a file holding just that clip.  TP = max_{c,t,p} |y_c[4 t + p]|.  Phase 0 only reproduces the samples,
 *    so the device forms TP = max(P, peak of phases 1-3); TP >= P holds exactly.
 * 3. Short-term loudness.  w_j = (1 / 30 q) sum_c G_c (s_c[j] + .. + s_c[j + 29]) for j < Js = max(0, I - 29);
 *    S_j = -0.691 + 10 log10 w_j, and -inf at w_j = 0.  Smax = max_j S_j, and -inf when Js = 0.
 * 4. Loudness range (Tech 3342, blocks every 1 s as libebur128 takes them).  R = {j = 10 m : j < Js}, Jr = |R| = ceil(Js / 10).
 *    Ar = {j in R : S_j > -70}.  Gamma_r = -0.691 + 10 log10(mean_Ar w_j) - 20.  Gr = {j in Ar : S_j > Gamma_r}, n = |Gr|.  Sort S_j
 *    over Gr ascending into v[0 .. n - 1]: LRA = v[(19 (n - 1) + 10) / 20] - v[(n + 4) / 10] with integer divisions, and LRA = 0
 *    when n = 0.  The indices equal libebur128's (size_t)((n - 1) 0.95 + 0.5) and (size_t)((n - 1) 0.1 + 0.5) for every
 *    n <= 200 000; the integer forms are used so that no product in binary64 decides an index.
 * 5. Gain.  The loudness call's item 5 with P replaced by PM: PM = TP when limit_true_peak = 1, else P.
 * 6. Outputs.  stats[k][16]: fields 0-7 are the loudness call's [L, M, P, g, Gamma, J, |A|, |Gt|], fields 8-15 are
 *    [TP, Smax, LRA, Gamma_r, Js, Jr, |Ar|, |Gr|].  momentary[k][Jmax] as there.  short_term[k][Jsmax] = S_j, -inf from Js on,
 *    Jsmax = max(0, T / q - 29).  audio = fl32(x g).  With limit_true_peak = 0, fields 0-7, momentary and audio are the
 *    loudness call's bit for bit: the same arithmetic in the same order.
 * 7. Refusals (-1, nothing written): whatever pdmp3_amd_loudness_check refuses; limit_true_peak outside {0, 1}; an n_samples
 *    whose Jr > 4096 (about 68 minutes: the order statistic is taken inside one workgroup).  Refused, replayed and
 *    mixed-format clips in a batch as in the loudness call.  A clip wholly behind the end gives that call's eight numbers, then
 *    [0, -inf, 0, -inf, Js, Jr, 0, 0]. */
typedef struct {
  pdmp3_amd_loudness_spec loudness;
  int limit_true_peak;      /* 1: g PM <= peak_limit with PM the true peak; 0: the sample peak */
} pdmp3_amd_r128_spec;
/* 0 when the call would accept these numbers (n_samples among them) at fs and `channels` (1 or 2) channels, else -1 (item 7) */
int pdmp3_amd_r128_check(const pdmp3_amd_r128_spec* spec, long fs, int channels);
/* The interpolator: h[49] in binary64, and phases [3][12] binary32, c_p[d] of phases 1 .. 3 as the kernel reads them, rounded
 * once.  Pointers may be NULL.  0. */
int pdmp3_amd_r128_taps(double* h, float* phases);
/* pdmp3_amd_loudness_plan's numbers, then Js, Jr and Jsmax.  Pointers may be NULL.  0, or -1 (there, and where Jr > 4096). */
int pdmp3_amd_r128_plan(long fs, long long n_samples, int* B, int* chunk, unsigned* lds_bytes, int* q, long long* n_chunks, long long* I,
                        long long* J, long long* Js, long long* Jr, long long* Jsmax);
/* As pdmp3_amd_bulk_decode_clips_loudness with stats [n_clips][16] floats and short_term: NULL, or [n_clips][Jsmax] floats, host
 * memory or device memory of the decoder's GPU.  The kernels are csrc/loudness.hip's, k_loud_blocks and k_loud_gate in their
 * second instantiation.  -1 also where pdmp3_amd_r128_check says so. */
int pdmp3_amd_bulk_decode_clips_r128(pdmp3_amd_bulk* b, const pdmp3_amd_audio_clip* clips, int n_clips, const pdmp3_amd_r128_spec* spec,
                                     float* stats, float* momentary, float* short_term, long long* valid);

/* ---- Pitch of clips (YIN, de Cheveigne and Kawahara 2002, with librosa.yin's parameters) ----
 * K clips as one planar float32 batch, frames innermost: f0, aperiodicity and lag [K][C][3][F], or the cumulative-mean-normalised
 * difference curve [K][C][tmax + 1][F] that pYIN-style trackers start from.  New entry points only.  The definition is
 * evaluated in binary64 on the binary32 row x_c[t] that pdmp3_amd_bulk_decode_clips_audio returns at the call's rate and
 * channels (sections 13-19's convention).  N = frame_length, W = win_length (0: N / 2), H = hop (0: N / 4).
 * 1. Framing, centred as the transform's: frame f of clip k is z[j] = x[start + f H - N / 2 + j], j = 0 .. N - 1; real
 *    neighbours inside the stream, zeros outside, no reflection; valid[k] = clamp(ceil((J - start) / H), 0, F).
 * 2. Lags.  tmin = max(1, floor(sr / fmax)), tmax = min(ceil(sr / fmin), N - W - 1), from integer arithmetic on the binary64
 *    quotient q: where |q - round(q)| < 1e-9 the quotient must be that integer exactly (the divisor times it is sr without a
 *    rounding error), else the spec is refused.
 * 3. Difference function, tau = 0 .. tmax: r(tau) = sum over j < W of z[j] z[j + tau], e(tau) = sum over j < W of
 *    z[j + tau]^2, d(tau) = e(0) + e(tau) - 2 r(tau) = sum over j < W of (z[j] - z[j + tau])^2  (r(0) = e(0)).
 * 4. S(tau) = d(1) + .. + d(tau); d'(0) = 1; d'(tau) = d(tau) tau / S(tau) where S(tau) > 0, else 1.
 * 5. Decision (librosa's) on [tmin, tmax]: tau is a trough when d'(tau) < d'(tau - 1) and d'(tau) <= d'(tau + 1); at tmin:
 *    d'(tmin) < d'(tmin + 1); tmax is never one.  tau* = the smallest trough with d'(tau*) < threshold; if there is none, the
 *    smallest tau of [tmin, tmax] that attains the minimum of d'.
 * 6. With a = d'(tau* - 1), b = d'(tau*), c = d'(tau* + 1), D = a - 2 b + c: delta = (a - c) / (2 D) when tmin < tau* < tmax
 *    and D > 0, else 0; f0 = sr / (tau* + delta).  A frame whose N samples are all zero gives f0 = 0, aperiodicity 1,
 *    tau* = 0 exactly; its curve is 1 everywhere.
 * 7. out_mode 0: [K][C][3][F], plane 0 f0, plane 1 d'(tau*), plane 2 tau*.  out_mode 1: [K][C][tmax + 1][F], d'(tau).  The
 *    device takes decision and refinement on the binary32 curve values it stores in mode 1: plane 2 is rule 5 applied to the
 *    mode-1 output of the same arguments, plane 1 is that curve at tau* bit for bit, plane 0 is rule 6 in binary64 on those
 *    three binary32 values, rounded once (a frame of zeros excepted: rule 6's last sentence).
 * Arithmetic.  r^ is a binary32 fused multiply-add chain over j ascending (v_mfma_f32_16x16x4_f32); e is a difference of two
 * binary64 prefix sums of the exact squares; d, S (one fixed order) and d tau / S are binary64, d' is rounded once.  With
 * u = 2^-24 and n = 4 ceil((W + 15) / 4): |r^ - r| <= (n u / (1 - n u)) sum |z[j] z[j + tau]|; section 20 derives the bounds
 * of d, S, d' and f0 from it and says when a frame's decision is undecided against the binary64 definition.
 * 8. Refusals (-1, nothing written): N odd or outside 64 .. 2048, W outside 4 .. N - 2, H outside 1 .. N, fmin <= 0,
 *    fmax <= fmin, fmax > sr / 2, tmin >= tmax, threshold outside (0, 1], out_mode not 0 or 1, rule 2's, n_frames < 0, and
 *    whatever the audio call refuses.  N = 4096 is left to a follow-up. */
typedef struct {
  long rate; int channels; int width; double rolloff;   /* as pdmp3_amd_mel_spec */
  long long n_frames;
  int frame_length, win_length, hop;                    /* N (2048); W, 0 = N / 2; H, 0 = N / 4 */
  double fmin, fmax;                                    /* Hz */
  double threshold;                                     /* 0.1 */
  int out_mode;                                         /* 0: f0, aperiodicity, lag; 1: the curve */
} pdmp3_amd_pitch_spec;
/* 0 when the spec's numbers are acceptable at sampling frequency sr, else -1 (item 8) */
int pdmp3_amd_pitch_check(const pdmp3_amd_pitch_spec* spec, long sr);
/* *tmin, *tmax (item 2) and *tiles = ceil((tmax + 1) / 256), the lag tiles of a frame.  Pointers may be NULL.  0, or -1 where
 * the check refuses the spec. */
int pdmp3_amd_pitch_lags(const pdmp3_amd_pitch_spec* spec, long sr, int* tmin, int* tmax, int* tiles);
/* What a workgroup of k_clip_pitch takes, the function the call itself uses: *frames (one a wave: 8, or 4, 2, 1 where the LDS
 * below would pass 160 KB - 64), *span_floats (the span with its zeros around it, skewed by 2 floats every 16), *lds_bytes
 * (the span, (frames - 1) H + N + 1 binary64 prefix sums, 64 frames + 64 binary64 scratch values, 256 tiles + 8 floats a
 * frame for its curve, 4 a frame for its result) and *ksteps = ceil((W + 15) / 4), the matrix instructions a lag tile.  More
 * than 64 KB runs in a kernel with a static array (k_clip_pitch_big).  Pointers may be NULL.  0, or -1 as the check. */
int pdmp3_amd_pitch_plan(const pdmp3_amd_pitch_spec* spec, long sr, int* frames, unsigned* span_floats, unsigned* lds_bytes, int* ksteps);
/* Row k receives channel c's [3][n_frames] (out_mode 1: [tmax + 1][n_frames]) floats at dst + c * chan_stride.  Everything
 * else -- the audio call in front, the stages, host destinations, the per-clip refusals in valid[k], rate 0 / channels 0,
 * width, rolloff, the counts, n_clips = 0 and n_frames = 0, synchronous -- as pdmp3_amd_bulk_decode_clips_stft; k_clip_pitch
 * (csrc/pitch.hip) writes the rows and reads no table.  -1 also where pdmp3_amd_pitch_check says so. */
int pdmp3_amd_bulk_decode_clips_pitch(pdmp3_amd_bulk* b, const pdmp3_amd_audio_clip* clips, int n_clips, const pdmp3_amd_pitch_spec* spec,
                                      long long* valid);

/* ---- Onset strength, tempogram and tempo of clips (librosa.onset.onset_strength, librosa.feature.tempogram and
 * librosa.feature.tempo with their parameters) ----
 * K clips as one planar float32 batch: the onset envelope [K][C][F], the autocorrelation tempogram [K][C][Wt][F], frames
 * innermost, or the tempo estimate [K][C][4].  New entry points only.  The definition is evaluated in binary64 on binary32
 * values that the product itself can return, so every stage can be held against its predecessor.  N = n_fft, H = hop,
 * Wt = win_length of the tempogram (even), Wh = Wt / 2, F = n_frames.
 * 1. Log-mel.  l[m][f] is the binary32 value that pdmp3_amd_bulk_decode_clips_mel_long stores at out_mode 2 (log10 max(M,
 *    floor)) for band m of the frame centred on sample start + f H, with the same mel fields (spec.mel; its out_mode is not
 *    read).  f runs from -(lag + Wh) to F - 1 + Wh - 1 in modes 1 and 2, from -lag to F - 1 in mode 0.  Frames in front of the
 *    clip and behind it see the stream's real neighbours, zeros outside the stream, no reflection.  The value is that call's bit
 *    for bit: the kernel is the same.
 * 2. Reference spectrum (librosa's max_size; SuperFlux at 3): ref[m][f] = max of l[m'][f] over |m' - m| <= (max_size - 1) / 2,
 *    m' clamped to 0 .. n_mels - 1 (scipy's reflecting maximum filter gives the same).
 * 3. Onset strength: o[f] = (10 / n_mels) * sum over m ascending of max(0, l[m][f] - ref[m][f - lag]), rounded once to
 *    binary32: the mean over the bands of the half-wave rectified dB difference, librosa.onset.onset_strength(lag, max_size,
 *    aggregate=mean) on power_to_db(S, top_db=None), without librosa's shift by n_fft // (2 hop) frames and with the real
 *    history in place of its zero padding.  top_db is not offered: it makes every value depend on the clip's loudest frame, so
 *    a clip would no longer be the slice of a longer one; a caller who wants a fixed range sets `floor`.
 * 4. Windowed frame: x_f[n] = fl32(w[n] * o[f - Wh + n]), n = 0 .. Wt - 1, w[n] = 0.5 - 0.5 cos(2 pi n / Wt) in binary64
 *    rounded once (scipy's get_window("hann", fftbins=True)).
 * 5. Autocorrelation: r_f(tau) = sum over n < Wt - tau of x_f[n] x_f[n + tau], tau = 0 .. Wt - 1; T[tau][f] = r_f(tau) / r_f(0)
 *    where r_f(0) > 0, else exactly 0 (librosa's norm=inf: |r(tau)| <= r(0)).
 * 6. Tempo (librosa.feature.tempo, static, aggregate=mean): A[tau] = (sum over f < F ascending of T[tau][f]) / F on the
 *    binary32 T of mode 1; bpm(tau) = 60 sr / (H tau); prior[tau] = -0.5 ((log2 bpm(tau) - log2 start_bpm) / std_bpm)^2, and
 *    -inf for tau = 0 and wherever bpm(tau) >= max_tempo; s[tau] = log1p(1e6 A[tau]) + prior[tau]; tau* = the smallest argmax.
 * 7. out_mode 0 "onset": [K][C][F], o.  1 "tempogram": [K][C][Wt][F], T.  2 "tempo": [K][C][4] = bpm(tau*), tau*, s[tau*], and
 *    the margin s[tau*] minus the largest s at any other lag (+inf where no other lag is admissible).  The o that mode 1 windows
 *    is mode 0's output bit for bit, for the clip widened by Wh frames on both sides (start - Wh H, F + Wt - 1 frames); the T
 *    that mode 2 averages is mode 1's output bit for bit.
 * Arithmetic.  o is a binary64 sum rounded once; r^ is a binary32 fused multiply-add chain over n ascending
 * (v_mfma_f32_16x16x4_f32), T = r^(tau) / r^(0) in binary64 rounded once; A, log1p and s are binary64.  Section 21 derives
 * the bounds and says when a clip's tempo is decided against the binary64 definition.
 * 8. valid[k] is the centred calls': clamp(ceil((J - start) / H), 0, F).
 * 9. Refusals (-1, nothing written): whatever pdmp3_amd_mel_long_check refuses with out_mode 2; lag outside 1 .. 16; max_size
 *    even or outside 1 .. 9; win_length odd or outside 16 .. 1024; start_bpm, std_bpm, max_tempo not finite and positive; a prior
 *    that is -inf at every lag; out_mode not 0, 1 or 2; n_frames < 0; a row of a clip (the output's, the log-mel's) beyond
 *    2^31 - 1 floats; and whatever the audio call refuses. */
typedef struct {
  pdmp3_amd_mel_long_spec mel;                          /* the log-mel of item 1; mel.n_frames = F; mel.out_mode is not read */
  int lag, max_size;                                    /* 1; 1 */
  int win_length;                                       /* Wt (384) */
  double start_bpm, std_bpm, max_tempo;                 /* 120, 1, 320 */
  int out_mode;                                         /* 0 onset, 1 tempogram, 2 tempo */
} pdmp3_amd_tempogram_spec;
/* 0 when the spec's numbers are acceptable at sampling frequency sr, else -1 (item 9) */
int pdmp3_amd_tempogram_check(const pdmp3_amd_tempogram_spec* spec, long sr);
/* w[0 .. Wt - 1] of item 4 as the kernel reads it.  Returns Wt, or -1 (win_length refused, or cap < Wt); w may be NULL with
 * cap 0 to ask for the count. */
int pdmp3_amd_tempogram_window(int win_length, float* w, size_t cap);
/* prior[0 .. Wt - 1] of item 6 in binary64 and *first, the smallest admissible lag.  Pointers may be NULL.  0, or -1 as the
 * check. */
int pdmp3_amd_tempogram_prior(const pdmp3_amd_tempogram_spec* spec, long sr, double* prior, size_t cap, int* first);
/* What the call launches, the function the call itself uses: *front and *back, the log-mel frames in front of frame 0 and
 * behind frame F - 1 (lag + Wh and Wh - 1; mode 0: lag and 0), *tiles = ceil(Wt / 256), *ksteps = ceil((Wt + 15) / 4), the
 * matrix instructions a lag tile, *frames (one a wave: 8, or 4, 2, 1 where the LDS would pass 160 KB - 64) and *lds_bytes of a
 * workgroup of k_clip_tempogram: per frame the skewed span (16 zeros, Wt values, zeros as far as the operands reach) and
 * 256 tiles + 8 floats for its curve.  Pointers may be NULL.  0, or -1 as the check. */
int pdmp3_amd_tempogram_plan(const pdmp3_amd_tempogram_spec* spec, long sr, int* front, int* back, int* tiles, int* ksteps, int* frames,
                             unsigned* lds_bytes);
/* Row k receives channel c's [F] (mode 0), [Wt][F] (mode 1) or [4] (mode 2) floats at dst + c * chan_stride.  The log-mel
 * batch, (modes 1, 2) the envelope and (mode 2) the tempogram go to a stage of the decoder, not to the caller.  Everything else
 * -- the audio call in front, host destinations, the per-clip refusals in valid[k], rate 0 / channels 0, width, rolloff, the
 * counts, n_clips = 0 and n_frames = 0, synchronous -- as pdmp3_amd_bulk_decode_clips_stft.  k_clip_mel_long writes the
 * log-mel; k_clip_onset, k_clip_tempogram and k_clip_tempo (csrc/tempogram.hip) the rest. */
int pdmp3_amd_bulk_decode_clips_tempogram(pdmp3_amd_bulk* b, const pdmp3_amd_audio_clip* clips, int n_clips, const pdmp3_amd_tempogram_spec* spec,
                                          long long* valid);

/* ---- Spectral descriptors of clips at n_fft 2048 and 4096 ----
 * The per-frame scalars of librosa.feature -- RMS energy, zero-crossing rate, spectral centroid, bandwidth, roll-off and
 * flatness -- of K clips as one planar float32 batch [K][C][6][F], frames innermost, rows of K and C may be strided; the
 * spectrum they are made of never leaves the device's compute units.  New entry points only.
 * Frame and signal are the two-stage transform's above: n_fft = N is 2048 or 4096, hop 1 .. N, win_length 0 (= N) or 1 .. N
 * centred as torch.stft centres it, window NULL (periodic Hann of win_length) or the caller's binary32 values; there is no
 * `normalized`.  x[n] = y[start + f hop - N / 2 + n], n < N: real neighbours inside the stream, zeros outside, no reflection;
 * valid[k], rate 0 and channels 0 as pdmp3_amd_bulk_decode_clips_mel.
 * X is that transform's spectrum bit for bit (the same chains), P_k = fma(Im, Im, Re Re), S_k = sqrtf(P_k) -- what its modes 2
 * and 1 store -- for all k = 0 .. N / 2, the Nyquist bin included; f_k = k sr / N.  The rows:
 *   0 rms        sqrt((1 / N) sum_n x[n]^2) over the unwindowed frame (librosa.feature.rms, frame_length = N)
 *   1 zcr        (1 / N) #{n = 1 .. N - 1: neg(x[n]) != neg(x[n - 1])}, neg(v) = v < -t, t = zcr_threshold rounded to binary32
 *                (librosa's zero_pos = True, pad = False): exact
 *   2 centroid   sum f_k S_k / sum S_k
 *   3 bandwidth  sqrt(sum S_k (f_k - centroid)^2 / sum S_k)                  (librosa's p = 2, norm = True)
 *   4 rolloff    the least f_k with S_0 + .. + S_k >= roll_percent sum S
 *   5 flatness   exp(mean_k ln max(amin, P_k)) / mean_k max(amin, P_k)       (librosa's power = 2)
 * A frame whose samples are all zero gives rows 0 .. 4 exactly 0; row 5 is what its formula gives.
 * Arithmetic.  The sums of rows 0 and 2 .. 5 are binary64 sums in one fixed order (csrc/spectral_core.h) that does not depend on
 * the frame's place in a tile, clip or batch, each value rounded once to binary32; x^2 is exact in binary64; ln is binary32 logf
 * of fmaxf(P, amin).  The cumulative sum of row 4 runs in ascending k: each of 64 lanes sums its run of N / 128 consecutive
 * bins (the last one's ends with bin N / 2), a scan adds the lanes' totals in ascending order -- its last value is the one
 * sum S that rows 2 .. 4 use -- and a lane's bins are compared as prefix + (the run's sum so far).  No atomics: two runs are
 * bit-equal.
 * Not offered: spectral contrast (its per-band quantiles are a ranking of their own), p != 2, subsets of the rows,
 * n_fft <= 1024. */
typedef struct pdmp3_amd_spectral_spec {
  long rate; int channels; int width; double rolloff;   /* as pdmp3_amd_mel_spec (rolloff: the resampling filter's) */
  int n_fft, hop, win_length;                           /* N: 2048 or 4096; 1 .. N; 0 = N, else 1 .. N */
  const float* window;                                  /* win_length values, NULL = periodic Hann */
  long long n_frames;
  double roll_percent;                                  /* inside (0, 1); librosa's default is 0.85 */
  double amin;                                          /* > 0 as binary32; librosa's default is 1e-10 */
  double zcr_threshold;                                 /* >= 0; librosa's default is 1e-10 */
} pdmp3_amd_spectral_spec;
#define PDMP3_SPECTRAL_ROWS 6
/* 0 when the spec's numbers are acceptable at sampling frequency sr, else -1: any other n_fft, hop outside 1 .. n_fft, a bad
 * win_length or window value (pdmp3_amd_stft_long_check's rules), roll_percent outside (0, 1), amin that is not positive and
 * finite as binary32, a negative or non-finite zcr_threshold, n_frames < 0, sr <= 0. */
int pdmp3_amd_spectral_check(const pdmp3_amd_spectral_spec* spec, long sr);
/* What a workgroup of k_clip_spectral takes, the function the call itself uses: *tile frames -- 8 at n_fft 2048, 4 at 4096, at
 * every hop -- and all bins.  The LDS bytes: the tile's span, (tile - 1) hop + n_fft floats rounded up to 4, which stays; Z,
 * tile x N2 x 32 floats; the plane, tile x (n_fft / 2 + 1) floats; 8 x tile floats of results; rounded up to 16 bytes.
 * *row_pad is 0.  Every plan is above 64 KB and runs on a static array.  0, or -1 on a bad argument.  Pointers may be NULL. */
int pdmp3_amd_spectral_plan(int n_fft, int hop, int* tile, int* row_pad, unsigned* lds_bytes);
/* pdmp3_amd_bulk_decode_clips_stft_long's course -- rows through the audio call, destinations, the stages, the per-clip
 * refusals in valid[k], rate 0 / channels 0, the counts, n_clips = 0 and n_frames = 0 -- with the check above and
 * k_clip_spectral (csrc/spectral.hip) writing the rows: row k receives channel c's [6][n_frames] floats at
 * dst + c * chan_stride.  The transform's tables are that call's.  -1 also where pdmp3_amd_spectral_check says so. */
int pdmp3_amd_bulk_decode_clips_spectral(pdmp3_amd_bulk* b, const pdmp3_amd_audio_clip* clips, int n_clips, const pdmp3_amd_spectral_spec* spec,
                                         long long* valid);

/* ---- Harmonic-percussive separation of clips at n_fft 2048 and 4096 ----
 * Median-filter separation of the magnitude spectrogram (librosa.decompose.hpss, librosa.effects.harmonic / percussive) of K
 * clips as one planar float32 batch, frames innermost, rows of K and C may be strided.  New entry points only.
 * Frame and signal are the two-stage transform's above: n_fft = N is 2048 or 4096, hop = H 1 .. N, win_length 0 (= N) or 1 .. N
 * centred as torch.stft centres it, window NULL (periodic Hann of win_length) or the caller's binary32 values; there is no
 * `normalized`; real neighbours inside the stream, zeros outside, no reflection; rate, channels, width, rolloff, valid[k], rate 0
 * and channels 0 as pdmp3_amd_bulk_decode_clips_stft_long.
 * K = N / 2 + 1 bins, F = n_frames; Lh = kernel_harm (frames) and Lp = kernel_perc (bins) are odd, 3 .. 31 (librosa: 31 / 31);
 * rh = (Lh - 1) / 2, rp = (Lp - 1) / 2.
 *   1. S[k][f] is the binary32 value pdmp3_amd_bulk_decode_clips_stft_long stores at out_mode 1 for bin k of the frame centred
 *      on sample start + f H, bit for bit (the same kernel), f = -rh .. F - 1 + rh.  In mode 2 Re and Im are that call's
 *      out_mode 0 values and S = sqrtf(fma(Im, Im, Re Re)), that kernel's expression.
 *   2. Hm[k][f] is the (rh + 1)-th smallest of S[k][f - rh .. f + rh]: along time over the stream's real frames (librosa
 *      reflects at a clip's edge; here a clip stays the slice of a longer one).
 *   3. Pm[k][f] is the (rp + 1)-th smallest of S[rho(i)][f], i = k - rp .. k + rp; rho(i) = -1 - i for i < 0, 2 K - 1 - i for
 *      i >= K, else i: scipy.ndimage.median_filter(mode = "reflect"), numpy's "symmetric", as librosa along frequency.
 *      A median of an odd count is one of its elements and every S is +0 or positive and finite: Hm and Pm are exact.
 *   4. Masks (librosa.util.softmask): (X, R) = (Hm, margin_harm Pm) for the harmonic mask, (Pm, margin_perc Hm) for the
 *      percussive one, the product one binary64 multiplication.  power is exactly 1, 2 or +inf.  Finite power: where
 *      max(X, R) < 2^-126 the mask is 0.5 if both margins are 1, else 0; otherwise m = X^p / (X^p + R^p) in binary64, rounded
 *      once to binary32.  power = +inf: m = 1 if X > R, else 0.
 *   5. out_mode, component 0 harmonic, 1 percussive:
 *        0 mask       [K][C][2][bins][F]     m
 *        1 magnitude  [K][C][2][bins][F]     fl32(S m), one binary32 multiplication with mode 0's m
 *        2 complex    [K][C][2][bins][F][2]  (fl32(Re m), fl32(Im m)): what torch.istft takes
 *        3 median     [K][C][2][bins][F]     Hm and Pm themselves
 *      The modes agree bit for bit: mode 1 is mode 0 times the spectrum call's magnitude, mode 2 mode 0 times its complex
 *      output, mode 0 the stated function of mode 3.
 * Every element comes from the same operations whatever its tile, clip or batch; no atomics: two runs are bit-equal.
 * Not offered: any other power, kernels above 31, reflection along time, n_fft <= 1024. */
typedef struct pdmp3_amd_hpss_spec {
  long rate; int channels; int width; double rolloff;   /* as pdmp3_amd_mel_spec (rolloff: the resampling filter's) */
  int n_fft, hop, win_length;                           /* N: 2048 or 4096; 1 .. N; 0 = N, else 1 .. N */
  const float* window;                                  /* win_length values, NULL = periodic Hann */
  long long n_frames;
  int kernel_harm, kernel_perc;                         /* odd, 3 .. 31: frames; bins */
  double margin_harm, margin_perc;                      /* >= 1, finite; librosa's default is 1 */
  double power;                                         /* 1, 2 or +inf; librosa's default is 2 */
  int out_mode;                                         /* 0 mask, 1 magnitude, 2 complex, 3 median */
} pdmp3_amd_hpss_spec;
#define PDMP3_HPSS_MAX_KERNEL 31
/* 0 when the spec's numbers are acceptable at sampling frequency sr, else -1: whatever pdmp3_amd_stft_long_check refuses (any
 * other n_fft, hop outside 1 .. n_fft, a bad win_length or window value, sr <= 0), a kernel size that is even or outside
 * 3 .. 31, a margin below 1 or not finite, a power other than 1, 2 and +inf, out_mode outside 0 .. 3, n_frames < 0, a channel's
 * row of the output (2 bins n_frames floats, twice that in mode 2) or of the stage (bins (n_frames + kernel_harm - 1)) beyond
 * 2^31 - 1 floats. */
int pdmp3_amd_hpss_check(const pdmp3_amd_hpss_spec* spec, long sr);
/* What the call launches, the function the call itself uses: *front and *back, the frames of the spectrum in front of frame 0
 * and behind frame F - 1 (both kernel_harm / 2); *tile_bins x *tile_frames, the elements of a workgroup of k_clip_hpss
 * (64 x 64 for every pair of sizes); *pitch, the floats between two rows of its tile in LDS (64 + 30), and *lds_bytes
 * ((64 + 30) x pitch x 4: the layout has room for 15 bins and 15 frames around the tile, of which kernel_perc / 2 and
 * kernel_harm / 2 are loaded).  Pointers may be NULL.  0, or -1 on a bad kernel size. */
int pdmp3_amd_hpss_plan(int kernel_harm, int kernel_perc, int* front, int* back, int* tile_bins, int* tile_frames, int* pitch,
                        unsigned* lds_bytes);
/* Row k receives channel c's [2][bins][F] floats (mode 2: [2][bins][F][2]) at dst + c * chan_stride.  Three steps: the audio
 * call for the clips widened to start - rh H and F + 2 rh frames; k_clip_stft_long, unchanged, into a stage of the decoder
 * (magnitudes; mode 2: complex values); k_clip_hpss (csrc/hpss.hip) writes the rows.  Everything else -- host destinations, the
 * per-clip refusals in valid[k], rate 0 / channels 0, width, rolloff, the counts, n_clips = 0 and n_frames = 0, synchronous --
 * as pdmp3_amd_bulk_decode_clips_stft_long.  -1, nothing written, also where pdmp3_amd_hpss_check says so. */
int pdmp3_amd_bulk_decode_clips_hpss(pdmp3_amd_bulk* b, const pdmp3_amd_audio_clip* clips, int n_clips, const pdmp3_amd_hpss_spec* spec,
                                     long long* valid);

/* ---- MFCC, deltas and dB mel of clips at n_fft 2048 and 4096 ----
 * librosa.feature.mfcc with librosa.feature.delta stacked under it, and librosa.power_to_db(melspectrogram) with top_db, of K
 * clips as one planar float32 batch, frames innermost, rows of K and C may be strided.  New entry points only; the Kaldi
 * call above (section 12) is a different definition.  The log-mel's parameters are pdmp3_amd_mel_long_spec's (mel.mel.floor is
 * librosa's amin; mel.mel.out_mode is not read); F = mel.mel.n_frames.
 * h = (delta_width - 1) / 2 if deltas > 0 and out_mode is 0, else 0.
 *   1. Log-mel.  l[m][t], t = -h .. F - 1 + h, is the binary32 value pdmp3_amd_bulk_decode_clips_mel_long stores at out_mode 2
 *      (log10 max(M, floor)) for the clip (start - h hop, F + 2 h), bit for bit (the same kernel): real neighbours inside the
 *      stream, zeros outside it, no reflection.  valid[k] is that call's count for the clip (start, F).
 *   2. dB.  d0[m][t] = fl32(10 l[m][t]), one binary32 product.  top_db >= 0: Mx = max d0[m][t] over all m and the clip's own
 *      frames t = 0 .. F - 1 -- the halo does not count --, per clip AND channel; thr = fl32(Mx - fl32(top_db));
 *      d = max(d0, thr).  top_db < 0: d = d0.  Mono is librosa.power_to_db(S, ref = 1.0, amin, top_db); for a stereo clip
 *      librosa takes one maximum over both channels, this call one per channel.  Every operation is one binary32 rounding and
 *      max is exact: d is reproducible bit for bit in binary32 from the log-mel call's values.
 *   3. Cepstra.  c[q][t] = sum_m T[q][m] d[m][t], q < n_mfcc <= n_mels;
 *      T[q][m] = s_q cos(pi q (2 m + 1) / (2 n_mels)) (1 + (lifter / 2) sin(pi (q + 1) / lifter)), s_0 = sqrt(1 / n_mels),
 *      s_q = sqrt(2 / n_mels) for q > 0, the lifter's factor 1 at lifter = 0: scipy.fft.dct(type = 2, norm = "ortho") and
 *      librosa's lifter.  T is formed in binary64 and rounded once; a cepstrum is one chain of binary32 fused multiply-adds
 *      over the bands in ascending order, the same for every frame wherever its tile starts.
 *   4. Deltas.  j = -h .. h, w = delta_width, S2 = sum j^2, S4 = sum j^4:
 *        D1[q][t] = sum_j (j / S2) c[q][t + j]
 *        D2[q][t] = sum_j 2 (j^2 - S2 / w) / (S4 - S2^2 / w) c[q][t + j]
 *      both on c (librosa.feature.delta(order = 2) is not the delta of the delta); at w = 9 the taps are j / 60 and
 *      (3 j^2 - 20) / 462.  These are the interior coefficients of scipy.signal.savgol_coeffs(w, order, deriv = order).  The
 *      formula holds at EVERY frame of the clip because the neighbours exist: librosa.feature.delta fits polynomials at a
 *      batch's edges (mode = "interp"), this call has no edges.  Each value is a chain of binary64 fused multiply-adds, j
 *      ascending, on the binary32 c, rounded once to binary32.
 *   5. Output.  out_mode 0 ("mfcc"): [K][C][(1 + deltas) n_mfcc][F], rows 0 .. n_mfcc - 1 c, then D1, then D2: the memory of
 *      np.concatenate([mfcc, delta, delta2], axis = -2).  out_mode 1 ("db"): [K][C][n_mels][F] = d; n_mfcc, lifter and the
 *      delta fields are not read.  F = 0 writes nothing but valid.
 * No atomics, one fixed order: two runs are bit-equal, and at top_db < 0 a clip is the slice of a longer one bit for bit.
 * Not offered: DCT types 1 and 3, norm = None, one maximum over the channels, delta's edge modes. */
typedef struct pdmp3_amd_mfcc_long_spec {
  pdmp3_amd_mel_long_spec mel;  /* the log-mel of item 1 */
  double top_db;                /* librosa's default is 80; negative: no clamp */
  int n_mfcc;                   /* 1 .. min(n_mels, 128); librosa's default is 20 */
  double lifter;                /* >= 0, finite; 0: none */
  int deltas, delta_width;      /* 0, 1 or 2; odd, 3 .. 17 (librosa: 9), read when deltas > 0 */
  int out_mode;                 /* 0 mfcc, 1 db */
} pdmp3_amd_mfcc_long_spec;
#define PDMP3_MFCC_LONG_MAX_WIDTH 17
#define PDMP3_MFCC_LONG_MAX_CEPS 128
/* 0 when the spec's numbers are acceptable at sampling frequency sr, else -1: whatever pdmp3_amd_mel_long_check refuses at
 * out_mode 2, top_db NaN or +inf, an out_mode other than 0 and 1; at out_mode 0 also n_mfcc outside 1 .. min(n_mels, 128), a
 * lifter that is negative or not finite, deltas outside 0 .. 2, with deltas > 0 a delta_width that is even or outside 3 .. 17;
 * a channel's row of the output ((1 + deltas) n_mfcc F, or n_mels F) or of the stage (n_mels (F + 2 h)) beyond 2^31 - 1 floats. */
int pdmp3_amd_mfcc_long_check(const pdmp3_amd_mfcc_long_spec* spec, long sr);
/* T of item 3 as k_clip_mfcc_long reads it: [n_mfcc rounded up to 16][n_mels rounded up to 16] (*rows, *cols; may be NULL),
 * zeros in the padding.  Returns the floats and writes min(that, cap); -1 on a bad argument (n_mels outside 1 .. 256, n_mfcc
 * outside 1 .. min(n_mels, 128), a bad lifter), nothing written. */
long long pdmp3_amd_mfcc_long_dct_table(int n_mels, int n_mfcc, double lifter, float* table, size_t cap, int* rows, int* cols);
/* Item 4's taps in binary64: taps[j + h] for D1, taps[w + j + h] for D2.  Returns w = delta_width; -1, nothing written, on a
 * width that is even or outside 3 .. 17 or where cap < 2 w.  taps NULL with cap 0: the count alone. */
int pdmp3_amd_mfcc_long_delta_taps(int delta_width, double* taps, size_t cap);
/* What the call launches, the function the call itself uses: *front and *back, the frames of the log-mel in front of frame 0
 * and behind frame F - 1 (both h); *tile, the frames of a workgroup of k_clip_mfcc_long (64); *d_pitch and *c_pitch, the
 * floats between two rows of its two LDS planes (80: the tile with the widest halo; 84); *lds_bytes = (mels16 d_pitch +
 * ceps16 c_pitch) x 4, at most 124 928: every shape fits PDMP3_MEL_LDS_MAX at 64 frames, so there is one tile.  out_mode 1:
 * no halo, *tile the 1024 elements of a workgroup of k_clip_db, no LDS.  Pointers may be NULL.  0, or -1 on a bad argument. */
int pdmp3_amd_mfcc_long_plan(int n_mels, int n_mfcc, int deltas, int delta_width, int out_mode, int* front, int* back, int* tile,
                             int* d_pitch, int* c_pitch, unsigned* lds_bytes);
/* Row k receives channel c's [(1 + deltas) n_mfcc][F] (out_mode 1: [n_mels][F]) floats at dst + c * chan_stride.  The audio
 * call for the clips widened to start - h hop and F + 2 h frames; k_clip_mel_long, unchanged, into a stage of the decoder;
 * k_clip_db_max (top_db >= 0: a plane's threshold, behind the clip's log-mel in the stage); k_clip_mfcc_long or k_clip_db
 * (csrc/mfcc_long.hip) write the rows.  T is made once per (n_mels, n_mfcc, lifter) and kept for the decoder's life.
 * Everything else -- host destinations, the per-clip refusals in valid[k], rate 0 / channels 0, width, rolloff, the counts,
 * n_clips = 0 and n_frames = 0, synchronous -- as pdmp3_amd_bulk_decode_clips_mel_long.  -1, nothing written, also where
 * pdmp3_amd_mfcc_long_check says so. */
int pdmp3_amd_bulk_decode_clips_mfcc_long(pdmp3_amd_bulk* b, const pdmp3_amd_audio_clip* clips, int n_clips,
                                          const pdmp3_amd_mfcc_long_spec* spec, long long* valid);

/* ---- pYIN pitch tracking of clips (Mauch and Dixon 2014, with librosa.pyin's parameters) ----
 * K clips as one planar float32 batch, frames innermost: f0, voiced flag, voiced probability and pitch bin [K][C][4][F], or the
 * observation probabilities with the voiced probability in the last row [K][C][n_b + 1][F].  New entry points only.  Framing,
 * the lags tmin .. tmax, valid[k], rate 0, channels 0, replay, mixed-format clips, destinations and strides are the pitch
 * call's (section 20); spec.pitch carries them, its threshold and out_mode are not read.  nt = n_thresholds, sr the call's rate.
 * 1. Curve.  c[tau][f] is the binary32 value that pdmp3_amd_bulk_decode_clips_pitch stores at out_mode 1 for the same frame
 *    arguments, bit for bit: the kernel is k_clip_pitch, unchanged, its destination a stage of the stream object.
 * 2. Troughs.  Section 20's rule 5 on [tmin, tmax]: tau is a trough when c(tau) < c(tau - 1) and c(tau) <= c(tau + 1); at tmin:
 *    c(tmin) < c(tmin + 1); tmax is never one.  In ascending lag they are t_1 < .. < t_n with heights h_j.  A frame without a
 *    trough has O = 0 everywhere; silence is such a frame (its curve is 1).
 * 3. Threshold weights.  theta_i = i / nt, i = 1 .. nt, in binary64.  w_i = I(theta_i; a, b) - I(theta_(i-1); a, b), the
 *    regularised incomplete beta function, a host table in binary64; for integer a, b in 1 .. 64 it is the finite binomial sum.
 *    Any other beta is refused unless threshold_weights gives nt finite non-negative doubles, which are then used as given.
 * 4. Candidate probabilities.  i_j = the least i with h_j < theta_i (the binary32 value against the binary64 entry, exactly),
 *    none if h_j >= 1.  For threshold i: B_i = {j : i_j <= i}, n_i = |B_i|, p_ij = #{j' < j : j' in B_i}.  Prior:
 *    pi(p, n) = fl(G[p] cN[n]), G[p] = exp(-lambda p), cN[n] = (1 - exp(-lambda)) / (1 - exp(-lambda n)), host tables (scipy's
 *    boltzmann.pmf).  P_j = sum over i >= i_j, ascending, of w_i pi(p_ij, n_i), in binary64.  g = the first j that attains
 *    min h, m = #{i : h_g >= theta_i}: P_g += no_trough_prob (w_1 + .. + w_m), the partial sums a host table.
 * 5. Pitch bins.  n_s = ceil(fl(1 / resolution)), n_b = floor(12 n_s log2(fmax / fmin)) + 1.  period_j = t_j + delta_j, delta
 *    by section 20's rule 6 in binary64 on the three binary32 curve values, 0 at tmin.  b_j = #{q in 1 .. n_b : period_j <= T_q},
 *    T_q = sr / (fmin 2^((q - 0.5) / (12 n_s))), a host table in binary64: librosa's clip(round(12 n_s log2(f / fmin)), 0, n_b)
 *    everywhere but on exact ties, without a logarithm on the device.  b_j = n_b is dropped (librosa's overwrite drops it), and
 *    so is a trough with P_j = 0.  Of two troughs in one bin the larger lag's P stands (librosa's fancy assignment: no sum).
 * 6. Observation.  O[b][f] = fl32(P) of the surviving trough in bin b, else +0.  v[f] = fl32(min(1, sum over b ascending of
 *    O[b][f])), in binary64 on the binary32 values.  Every unvoiced state observes U[f] = (1 - v) / n_b in binary64.
 * 7. Transitions: librosa's transition_local(n_b, Wd, "triangle", wrap=False), kron'ed with transition_loop(2, 1 - switch_prob).
 *    msf = round_half_even(max_transition_rate * 12 * H / sr), Wd = msf n_s + 1, hb = Wd / 2 (integer).  An odd Wd (every
 *    default) has tri[d] = 1 - |d| / ((Wd + 1) / 2) at offset d = i' - i, |d| <= hb.  An even Wd is not made odd: librosa places
 *    scipy's even triangle -- samples (2 min(m, Wd - 1 - m) + 1) / Wd, m = 0 .. Wd - 1, two equal peaks -- at offsets
 *    d = m - Wd / 2 + 1 where n_b is even and d = m - Wd / 2 where n_b is odd, and the offset left over at the other end
 *    holds 0; this call follows that.  Z_i = sum of tri[i' - i] over the i' in range.  Host tables in binary64:
 *    ltri[d] = ln tri[d], lZ[i] = ln Z_i, l_stay = ln(1 - switch_prob), l_sw = ln(switch_prob), L0 = ln(2^-1022).
 *    lt(s -> s') = ltri[i' - i] - lZ[i] + (l_stay or l_sw) where tri[i' - i] > 0, and L0 everywhere else: librosa's
 *    log(0 + tiny); a jump out of the band is allowed at that price.
 * 8. Path.  States 0 .. n_b - 1 are voiced, n_b .. 2 n_b - 1 unvoiced.  lo[f][s] = ln O or ln U, L0 where the value is 0;
 *    lp0 = L0 for voiced states and -ln n_b for unvoiced ones.  S(path) = lp0[s_0] + lo[0][s_0] + sum over f ascending of
 *    (lt(s_(f-1) -> s_f) + lo[f][s_f]).  The call returns a path that maximises S up to the device's own roundings
 *    (section 25 bounds them) and takes the lowest state among equal values.
 * 9. Outputs.  out_mode 0: [K][C][4][F]: plane 0 f0 = fl32(fmin 2^(b / (12 n_s))) from a host table where the frame is
 *    voiced, else `fill` (which may be NaN), or with use_bin_frequency = 1 the bin's frequency all the same (librosa's
 *    fill_na=None); plane 1 the voiced flag, 1 or 0; plane 2 v; plane 3 the bin b.  out_mode 1: [K][C][n_b + 1][F]: O, v in the
 *    last row.  Mode 0's path is the definition's on mode 1's output of the same arguments bit for bit.
 * 10. Refusals (-1, nothing written): whatever pdmp3_amd_pitch_check refuses; n_thresholds outside 1 .. 256; boltzmann <= 0;
 *    switch_prob or no_trough_prob outside (0, 1); n_s outside 1 .. 20; n_b outside 2 .. 2048; Wd > n_b (librosa refuses it);
 *    1 / resolution or 12 n_s log2(fmax / fmin) within 1e-9 of an integer, or the quotient of msf within 1e-9 of a half, unless
 *    the binary64 value of the formula is that boundary itself (section 20's rule 2); rows beyond 31 bits (the curve's, the
 *    observation's, the back-pointers'); an unknown mode or use_bin_frequency. */
typedef struct {
  pdmp3_amd_pitch_spec pitch;          /* rate, channels, width, rolloff, n_frames, frame_length, win_length, hop, fmin, fmax */
  int n_thresholds;                    /* 100 */
  double beta_a, beta_b;               /* 2, 18 */
  const double* threshold_weights;     /* NULL, or n_thresholds weights used in place of the beta distribution's */
  double boltzmann;                    /* 2: lambda */
  double resolution;                   /* 0.1 semitones */
  double max_transition_rate;          /* 35.92 octaves a second */
  double switch_prob, no_trough_prob;  /* 0.01, 0.01 */
  float fill;                          /* plane 0 of an unvoiced frame (NaN) */
  int use_bin_frequency;               /* 1: the bin's frequency there instead */
  int out_mode;                        /* 0: the path's four planes; 1: the observation */
} pdmp3_amd_pyin_spec;
/* 0 when the spec's numbers (n_frames among them) are acceptable at sampling frequency sr, else -1 (item 10) */
int pdmp3_amd_pyin_check(const pdmp3_amd_pyin_spec* spec, long sr);
/* Every table the kernels read, one block as pdmp3_hip_clip_pyin takes it: theta[nt] | w[nt] | wsum[nt + 1] (wsum[m] =
 * w_1 + .. + w_m) | G[mt] | cN[mt + 1] | T[n_b] | ltri[2 hb + 1] (offsets -hb .. hb; -inf where the window holds 0) | lZ[n_b] in
 * binary64, then the n_b bin frequencies in binary32 (padded to a whole double), then l_stay, l_sw, L0 and -ln n_b, which the
 * kernels take as parameters; mt = (tmax - 1 - tmin) / 2 + 1, the most troughs a frame can have.
 * counts (or NULL) receives {nt, mt, n_b, hb}.  Returns the block's size in doubles (tables NULL and cap 0: only that), or -1
 * as the check, or where cap is too small. */
int pdmp3_amd_pyin_tables(const pdmp3_amd_pyin_spec* spec, long sr, double* tables, size_t cap, int* counts);
/* The function the call itself uses.  numbers[8] = {states 2 n_b, n_b, n_s, msf, the band Wd, hb, frames (waves) of a workgroup
 * of k_clip_pyin_obs: 8, or 4, 2, 1 where its LDS would pass 64 KB, threads of a workgroup of k_clip_pyin_path}; lds[2] = the
 * LDS bytes of the two kernels (more than 64 KB: k_clip_pyin_path_big, a static array); stage[3] = the bytes a (clip, channel)
 * takes of the stage for its curve, its observation and its back-pointers (the last two 0 at out_mode 1).  Pointers may be
 * NULL.  0, or -1 as the check. */
int pdmp3_amd_pyin_plan(const pdmp3_amd_pyin_spec* spec, long sr, int* numbers, unsigned* lds, unsigned long long* stage);
/* Row k receives channel c's [4][n_frames] (out_mode 1: [n_b + 1][n_frames]) floats at dst + c * chan_stride.  The audio call
 * in front, then k_clip_pitch into the stage, k_clip_pyin_obs and (out_mode 0) k_clip_pyin_path (csrc/pyin.hip).  Everything
 * else as pdmp3_amd_bulk_decode_clips_pitch.  -1 also where pdmp3_amd_pyin_check says so. */
int pdmp3_amd_bulk_decode_clips_pyin(pdmp3_amd_bulk* b, const pdmp3_amd_audio_clip* clips, int n_clips, const pdmp3_amd_pyin_spec* spec,
                                     long long* valid);

/* ---- Beat tracking of clips (librosa.beat.beat_track, Ellis 2007, as librosa 0.10 states it) ----
 * The dynamic programme over the onset envelope of the tempogram call above, the walk back and the trim, per clip and channel.
 * New entry points only.  Evaluated in binary64 on binary32 values the product itself can return; every binary64 operation
 * below is rounded once and none is fused.  F = tg.mel.mel.n_frames, H = hop.
 *  o[f], f = 0 .. F - 1: mode 0 of pdmp3_amd_bulk_decode_clips_tempogram for the clip, bit for bit.  n = valid[k] frames enter;
 *  frames n .. F - 1 read nothing of the stream and are left out.
 *  1. Period.  bpm > 0: P = round-half-even(60 sr / (H bpm)).  bpm == 0: the tempogram chain runs in its mode 2 on the widened
 *     clip exactly as that call does, P = tau*, and o is the middle F values of its envelope (section 21 item 7: mode 0's bit
 *     for bit).  P lies in 1 .. 1023 (bpm == 0: in first .. Wt - 1, the admissible lags); h = max(1, round-half-even(P / 2)).
 *  2. Normalisation.  m = S / n, S the sum of o[f]; norm = sqrt(SS / (n - 1)), SS the sum of (o[f] - m)^2.  Both sums run in
 *     blocks of 64 frames, each block ascending from 0.0, then the blocks' sums ascending from 0.0.  z[f] = o[f] / norm.
 *  3. Local score.  g[k] = exp(-0.5 (32 k / P)^2), k = 0 .. P, a host table; ls[i] = the sum from 0.0 over j ascending from
 *     max(0, i - P) to min(n - 1, i + P) of z[j] g[|i - j|] (one product, one addition), rounded once to binary32.
 *  4. Programme.  tx[d] = -tightness (log d - log P)^2, d = h .. 2 P, a host table.  For i = 0 .. n - 1: among d = h ..
 *     min(2 P, i) the largest cum[i - d] + tx[d] above -inf, of equal ones the smallest d; cum[i] = (double) ls[i] + it, or
 *     (double) ls[i] where there is none.  i0 = the first i with (double) ls[i] >= 0.01 * (double) max ls.  back[i] = -1 for
 *     i < i0 and where no d is taken, else i - d*.
 *  5. Last beat.  i is a local maximum where i >= 1, cum[i] > cum[i - 1] and (i == n - 1 or cum[i] >= cum[i + 1]).  med = the
 *     exact median of cum over them (an even count: 0.5 (a + b) of the two middle ones).  The tail is the largest local maximum
 *     with cum >= 0.5 med.
 *  6. Walk back from the tail along back until -1: b_0 < .. < b_{q-1}.
 *  7. Trim.  s_t = (0.5 ls[b_{t-1}] + ls[b_t]) + 0.5 ls[b_{t+1}], missing neighbours 0; thr = 0.5 sqrt((sum of s_t^2 ascending
 *     from 0.0) / q) with trim, else 0; b_t is kept from the first to the last t with s_t > thr.
 *  8. No beats (count 0, mask all 0, list all -1): n < 2; norm not finite and positive; no local maximum; no local maximum at
 *     or above 0.5 med; no s_t above thr.  In the first two cases ls and cum are 0 and back is -1 everywhere.
 *  9. out_mode 0 "score": [K][C][F] = ls, 0 from frame n on.  1 "dp": [K][C][2][F] = fl32(cum) (0 from n on) and back as floats
 *     (-1 from n on).  2 "beats": [K][C][2][F], row 0 the beat mask, row 1 the kept beats' frames ascending, then -1.
 *     stats [K][C][8], may be NULL: the bpm used (the caller's as binary32, or the tempo call's out[0] bit for bit), P, beats
 *     kept, beats before the trim, the tail frame, norm, thr, n; kept is 0 and the four between are -1 where not reached (modes
 *     0 and 1 reach norm only).  Mode 2's ls, cum and back are modes 0 and 1's bit for bit.
 * 10. Refusals (-1, nothing written): whatever pdmp3_amd_tempogram_check refuses; bpm negative or not finite, or a P outside
 *     1 .. 1023; tightness not finite and positive; out_mode not 0, 1 or 2; n_frames > 32 768 (a clip's local maxima are ranked
 *     in one stage, its blocks' sums lie in LDS; 32 768 frames are 12.7 minutes at librosa's defaults). */
typedef struct pdmp3_amd_beat_spec {
  pdmp3_amd_tempogram_spec tg;                          /* the envelope and, at bpm 0, the tempo; tg.out_mode is not read */
  double bpm;                                           /* 0: estimated (librosa's default) */
  double tightness;                                     /* 100 */
  int trim;                                             /* 1 */
  int out_mode;                                         /* 0 score, 1 dp, 2 beats */
} pdmp3_amd_beat_spec;
#define PDMP3_BEAT_MAX_PERIOD 1023
#define PDMP3_BEAT_MAX_FRAMES 32768
/* 0 when the spec's numbers are acceptable at sampling frequency sr, else -1 (item 10) */
int pdmp3_amd_beat_check(const pdmp3_amd_beat_spec* spec, long sr);
/* g[0 .. P] and tx[0 .. 2 P] (the entries below h are 0 and not read) of items 3 and 4 for the period P, as the kernels read
 * them.  At bpm 0 the call uploads them for every P = first .. Wt - 1, 3 P + 2 values each, one P after the other.  Either
 * pointer may be NULL.  0, or -1 as the check or for a P outside 1 .. 1023. */
int pdmp3_amd_beat_tables(const pdmp3_amd_beat_spec* spec, long sr, int P, double* g, double* tx);
/* What the call launches, the function the call itself uses.  numbers[8]: P (0: estimated), h (of p_max where estimated), the
 * periods the tables hold p_min and p_max, the threads of a workgroup (256), the steps of the programme ceil(F / h), the lanes
 * of a frame and the frames of a pass of a step.  lds[2]: the LDS bytes of k_clip_beat_score and k_clip_beat_dp.  stage[2]: the
 * bytes a (clip, channel) takes of the stage for its scratch, and the bytes of the tables.  Pointers may be NULL.  0, or -1. */
int pdmp3_amd_beat_plan(const pdmp3_amd_beat_spec* spec, long sr, int* numbers, unsigned* lds, unsigned long long* stage);
/* Row k receives channel c's [F] (mode 0) or [2][F] floats at dst + c * chan_stride; stats: NULL, or [n_clips][C][8] floats in
 * host or device memory (a refused clip's stay as they are).  The audio call in front, k_clip_mel_long, k_clip_onset and (bpm 0)
 * k_clip_tempogram and k_clip_tempo into stages, then k_clip_beat_score, k_clip_beat_dp and k_clip_beat_pick (csrc/beat.hip).
 * Everything else as pdmp3_amd_bulk_decode_clips_tempogram.  -1 also where pdmp3_amd_beat_check says so. */
int pdmp3_amd_bulk_decode_clips_beats(pdmp3_amd_bulk* b, const pdmp3_amd_audio_clip* clips, int n_clips, const pdmp3_amd_beat_spec* spec,
                                      float* stats, long long* valid);

/* A corpus of whole files over the GPUs of a node -- SURVEY 8e's second partitioning ("C4: whole files per GPU, largest
 * first"), the C form of pdmp3_amd/sharding.py assign_files + one decoder per device (nothing of the
 * reference's: it has one handle and one thread).  devices[]: HIP device numbers, one host thread and one whole-stream
 * decoder per entry (a device listed twice gets two decoders); the files are dealt largest first, each device's files are
 * decoded one after the other with the asynchronous call, nothing is exchanged between devices.  pcm[i] (capacity
 * pcm_caps[i]; size it with pdmp3_amd_scan_buffer_iso) receives file i's PCM, pcm_bytes[i] the byte count pdmp3() would
 * write for it.  threads_per_decoder / window_frames / host_huffman as for pdmp3_amd_bulk_new_on.  0, or -1. */
void pdmp3_amd_corpus_assign(const size_t* sizes, int n_files, int world, int* rank_of);
int pdmp3_amd_corpus_decode(const int* devices, int n_devices, const unsigned char* const* mp3s, const size_t* sizes, int n_files,
                            unsigned char* const* pcm, const size_t* pcm_caps, long long* pcm_bytes, unsigned iso_mask,
                            int threads_per_decoder, int window_frames, int host_huffman);

#ifdef __cplusplus
}
#endif
#endif
