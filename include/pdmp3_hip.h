/*
 * pdmp3_hip.h -- C-ABI of the MI355X (gfx950) transform engine.
 *
 * This is the drop-in boundary for the ONE data-parallel hot path of
 * technosaurus/PDMP3: everything `Decode_L3` (pdmp3.c:1024-1060) does to one
 * parsed frame, plus `Convert_Frame_S16` (pdmp3.c:2307-2345):
 *
 *   L3_Requantize (P:1829) -> L3_Reorder (P:1786) -> L3_Stereo (P:1911) ->
 *   L3_Antialias (P:1706) -> L3_Hybrid_Synthesis/IMDCT_Win (P:1752/P:1649) ->
 *   L3_Frequency_Inversion (P:1738) -> L3_Subband_Synthesis (P:1978) ->
 *   interleaved int16 PCM.
 *
 * Plain C: pointers, sizes, PODs.  No C++/torch types.  Device pointers are
 * ordinary `void*` HIP device addresses; `stream` is a `hipStream_t` passed as
 * `void*` (NULL = the default stream).  All entry points return 0 on success
 * or a negative PDMP3_HIP_E* code; pdmp3_hip_last_error() gives the text.
 *
 * "P:n" = /root/reference/pdmp3.c line n.
 */
#ifndef PDMP3_HIP_H
#define PDMP3_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PDMP3_HIP_OK        0
#define PDMP3_HIP_EINVAL   -1   /* bad argument */
#define PDMP3_HIP_EDEVICE  -2   /* HIP runtime error (see pdmp3_hip_last_error) */
#define PDMP3_HIP_ENOMEM   -3

/* ------------------------------------------------------------------------
 * The record the device needs per granule-channel ("gc").
 *
 * It replaces the reference's in-handle structs t_mpeg1_side_info (P:71-95),
 * t_mpeg1_main_data (P:96-101) and the three header fields the hot path reads
 * (mode, mode_extension, sampling_frequency; P:56-70).
 *
 * Spectra travel separately as int16 (the reference keeps Huffman integers in
 * `float is[2][2][576]`, P:99; |value| <= 8206 = 15 + 2^13 - 1, P:1637).
 * Contract (what the reference's own Read_Huffman guarantees, P:2107-2111):
 * spectra[n] == 0 for n >= count1.
 * ---------------------------------------------------------------------- */

/* flags */
#define PDMP3_GC_SCALEFAC_SCALE  0x01u  /* P:92 */
#define PDMP3_GC_PREFLAG         0x02u  /* P:91 */
#define PDMP3_GC_WIN_SWITCH      0x04u  /* P:80 */
#define PDMP3_GC_BLOCK_TYPE_SHIFT 3     /* 2 bits, P:82 (0 when win_switch==0, P:1191) */
#define PDMP3_GC_BLOCK_TYPE_MASK 0x18u
#define PDMP3_GC_MIXED           0x20u  /* P:83 */

/* frame byte (identical in all gc records of one frame) */
#define PDMP3_FR_SFREQ_MASK      0x03u  /* sampling_frequency index: 0=44100 1=48000 2=32000 (P:529) */
#define PDMP3_FR_MODE_SHIFT      2      /* 2 bits: 0 stereo 1 joint 2 dual 3 mono (P:49-55) */
#define PDMP3_FR_MODE_MASK       0x0Cu
#define PDMP3_FR_MODEEXT_SHIFT   4      /* 2 bits: bit1 = MS, bit0 = intensity (P:1918,1932) */
#define PDMP3_FR_MODEEXT_MASK    0x30u
#define PDMP3_FR_RESET           0x40u  /* zero overlap + polyphase FIFO before this frame
                                           (what hsynth_init/synth_init do after
                                           pdmp3_open_feed, P:1757-1766, P:1996-2003) */

/* scalefac_s[12][w] marker: "the reference reads the float bits of
 * is[0][0][w] here" (granule 1 / channel 1 aliases the previous
 * granule's synthesis output).  Resolved on the device. */
#define PDMP3_SF_PEEK            0xFFu

typedef struct pdmp3_gc_side {
  uint16_t count1;            /* P:93; 0..576; first line of the rzero region      */
  uint8_t  global_gain;       /* P:77                                              */
  uint8_t  flags;             /* PDMP3_GC_*                                        */
  uint8_t  subblock_gain[3];  /* P:85                                              */
  uint8_t  frame;             /* PDMP3_FR_*                                        */
  uint8_t  scalefac_l[22];    /* P:97; [21] = value the reference's out-of-bounds
                                 read yields, resolved by the host     */
  uint8_t  scalefac_s[13][3]; /* P:98; [12][w] = out-of-bounds value
                                 or PDMP3_SF_PEEK                                  */
  uint8_t  iso;               /* PDMP3_GC_ISO_*: 0 = the reference's behaviour (below)  */
  uint8_t  lsf;               /* PDMP3_LSF_*: 0 = an MPEG-1 frame (all the reference knows) */
  uint8_t  lsf_slen[4];       /* channel 1 of an LSF intensity-stereo frame: the widths ... */
  uint8_t  lsf_nsfb[4];       /* ... and the sizes of its four scalefactor partitions       */
  uint8_t  reserved[49];      /* must be zero                                      */
} pdmp3_gc_side;              /* 128 bytes                                         */

/* pdmp3_gc_side.lsf -- MPEG-2 LSF and "MPEG-2.5" frames (ISO/IEC 13818-3; SURVEY 8f #4, last third).  NOT the reference,
 * which rejects them (P:1293): there is no reference behaviour to reproduce, so an LSF frame is decoded by the standard
 * -- as if every PDMP3_GC_ISO_* bit were set, with scalefac_l[21] = scalefac_s[12][w] = 0 -- and pinned by FFmpeg's decode
 * of the same streams (tests/golden/lsf_*.npz).  What differs from an MPEG-1 record:
 *   - the frame has ONE granule: the records [1][ch] of its frame slot are ignored, the synthesis state passes over them
 *     untouched, the frame's PCM is the first HALF of its place (576 sample-frames: 2304 bytes stereo, 1152 mono);
 *   - the sampling frequency is kLsfSampleRates[3 * version + (frame & 3)] (pdmp3_amd/csrc/lsf_tables.h): six more
 *     scalefactor-band tables; a mixed block's long part is bands 0..5 (36 lines), not 0..7;
 *   - PDMP3_GC_PREFLAG is what scalefac_compress >= 500 implies (no preflag bit in the stream);
 *   - intensity stereo (13818-3 2.4.3.2): is_pos p scales ONE channel by i0^((p + 1) / 2) (p odd: left, p even: right),
 *     i0 = 2^(-1/4) or 2^(-1/2) by PDMP3_LSF_IS_SCALE; "not intensity coded" is the largest value the partition's
 *     slen can hold, so channel 1's record carries its partitions (lsf_slen / lsf_nsfb, in transmission order: long
 *     bands, or band by band x window).                                                                              */
#define PDMP3_LSF_VERSION_MASK  0x03u  /* 1 = MPEG-2 LSF (22.05 / 24 / 16 kHz), 2 = MPEG-2.5 (11.025 / 12 / 8 kHz); identical
                                          in all gc records of one frame */
#define PDMP3_LSF_IS_SCALE      0x04u  /* channel 1: intensity_scale = scalefac_compress & 1 */

/* pdmp3_gc_side.iso (identical in all gc records of one frame) -- SURVEY 8f #4, "ISO-correct switches".  The reference
 * departs from ISO 11172-3 in five places; by default this engine reproduces them bit for bit.  A caller
 * that wants the standard's behaviour sets these bits (include/pdmp3.h: pdmp3_amd_set_quirks does it for a handle).  Three
 * of the six live in the transforms and travel in the record; the other three (H1 the count1 table, H4 / H5 the
 * one-past-the-end scalefactors) are decided where the records are built: a record with scalefac_l[21] = 0 and
 * scalefac_s[12][w] = 0 IS the standard's.  Nothing in the reference pins these modes; since round 6 an independent ISO
 * decoder does (FFmpeg, through tests/golden/iso_*.npz: DESIGN.md section 4). */
#define PDMP3_GC_ISO_MS_ALL    0x01u  /* H2: MS stereo on every line (P:1920 stops at the smaller count1, counted in reordered
                                         lines; until round 5 this bit meant "below the larger count1", which in short blocks
                                         leaves coded lines of the last band unrotated) */
#define PDMP3_GC_ISO_IS_SHORT  0x02u  /* H3: intensity stereo on short blocks multiplies by the ratios of the line's own
                                         window (P:2191 holds them in `unsigned`, P:2212-2213 assign instead of multiply,
                                         P:2203 takes the window from the un-reordered position) */
#define PDMP3_GC_ISO_IS_STD    0x04u  /* round 6, found with an independent ISO decoder (FFmpeg): the whole
                                         of the standard's intensity stereo -- is_pos from the RIGHT channel's scalefactors
                                         (P:2163 / P:2200 read the left one's), the intensity region bounded by the right
                                         channel's last non-zero line, per window in short blocks (P:1946-1965 use its count1),
                                         the last band (long 21, short 12) with the position of the band below (P:1961 / P:1953
                                         leave it out), the block shape from the right channel, no M/S rotation of intensity-coded
                                         lines.  Implies the arithmetic of PDMP3_GC_ISO_IS_SHORT */

#define PDMP3_GC_LINES          576
#define PDMP3_FRAME_GCS         4                 /* [gr][ch] = 2 x 2                */
#define PDMP3_FRAME_SPECTRA_BYTES (4 * 576 * 2)   /* int16 [2][2][576]               */
#define PDMP3_FRAME_SIDE_BYTES  (4 * 128)
#define PDMP3_FRAME_PCM_BYTES   (1152 * 2 * 2)    /* stereo; mono uses the first half */

typedef struct pdmp3_hip_ctx pdmp3_hip_ctx;

/* Create an engine on HIP device `device` (uploads the constant tables:
 * P:572-870 literals + the libm-derived pow/cos tables of P:979, P:1992,
 * P:2127-2128, P:2144-2146, generated on the host with the same expressions). */
int pdmp3_hip_create(int device, pdmp3_hip_ctx** out);
void pdmp3_hip_destroy(pdmp3_hip_ctx* ctx);
/* Environment read by pdmp3_hip_create() (none of them changes a result):
 *   PDMP3_HIP_CHAIN=0             every launch takes the chunk kernel (a chunk of frames per wave, halo)
 *   PDMP3_HIP_GRAN_MAX=n          largest launch, in frames, that takes the granule kernel (default 12288 on an MI355X)
 *   PDMP3_HIP_RING_MIN=n          launches of at least n frames take the persistent granule kernel k_decode_p (default 0 = never;
 *                                 only in a library built with -DPDMP3_WITH_RING_KERNEL: the default build does not carry the kernel)
 *   PDMP3_HIP_DIRECT_MAX=n        largest batch of a stream object that runs on the pinned host buffers directly (default 32; 0: never)
 *   PDMP3_HIP_SF_HINT=0|1|2       sampling frequency whose line table the granule kernel keeps in LDS (default 0 = 44.1 kHz;
 *                                 granules of another one read the table from memory)
 *   PDMP3_HIP_DEBUG_FAR_TIMEOUT=1 tests: every wait for another workgroup gives up at once (the independent way is taken)
 *   PDMP3_HIP_UNPACK_PROF=1       development: shader-clock stamps of k_unpack's steps, one line per launch on stderr
 *   PDMP3_HIP_GRAN_W=8            development: every launch of the granule kernel in workgroups of 8 waves (84 KB of LDS: one fits a
 *                                 CU beside a workgroup of k_unpack; by default launches that fill the chip take 16 -- measured with the
 *                                 whole-stream decoder: 30.7 against 32.8 M frames/s)
 * and by the host library (libpdmp3.so): PDMP3_DEVICE, PDMP3_STREAM_THREADS, PDMP3_NO_READAHEAD (include/pdmp3.h),
 * PDMP3_BULK_HOST_HUFFMAN, PDMP3_BULK_SNAPSHOT_ROWS, PDMP3_BULK_TRACE (include/pdmp3_bulk.h), PDMP3_CLI_STREAMING, PDMP3_CLI_WAV. */
const char* pdmp3_hip_last_error(void);

/* Bytes of one stream's carried synthesis state (replaces the function-static
 * `store[2][32][18]` P:1755 and `v_vec[2][1024]` P:1983; opaque layout). */
size_t pdmp3_hip_state_bytes(void);

/*
 * Decode `n_frames` consecutive frames of ONE stream: replaces n calls of
 * Decode_L3 (P:1024) + Convert_Frame_S16 (P:2307).
 *
 *   d_spectra  device, int16 [n_frames][2 gr][2 ch][576]
 *   d_side     device, pdmp3_gc_side [n_frames][2][2]
 *   d_pcm      device, int16; frame f occupies bytes [f*4608, f*4608+4608)
 *              (mono frames: the first 2304 bytes are used)
 *   d_state    device, pdmp3_hip_state_bytes() bytes, read before the first
 *              frame and written after the last one; NULL = start from the
 *              zero state and discard the final state
 *   chunk_frames  frames per wavefront ("chunk"); 0 = choose automatically.
 *              Chunks of several frames are independent: each re-derives the
 *              state at its start from a halo of preceding frames.
 *              PDMP3_HIP_CHUNK_PERSISTENT (-3): the persistent granule kernel (k_decode_p; tests and tools: it is
 *              bit-identical and, as measured in round 4, slower than the engine's own choice at every size).
 *              At 0 or 1, launches of up to 12288 frames (MI355X; PDMP3_HIP_GRAN_MAX)
 *              are decoded ONE GRANULE PER WAVEFRONT instead: the wavefronts hand
 *              IMDCT tails and polyphase rows on, no halo (scratch is kept per HIP
 *              stream -- for up to 32 streams, beyond that the halo form is used --
 *              or per pdmp3_hip_stream object).  A wavefront never depends on
 *              another workgroup for progress: that wait is bounded and ends in a
 *              halo decode.  PDMP3_HIP_CHAIN=0 in the environment at
 *              pdmp3_hip_create() keeps the halo form everywhere.  Same PCM and
 *              state either way, bit for bit.  pdmp3_hip_last_launch_kind() tells
 *              which form the engine's latest launch took.
 *
 * Asynchronous on `stream`.
 */
#define PDMP3_HIP_CHUNK_PERSISTENT (-3)   /* chunk_frames: take the persistent granule kernel whatever the launch size (tests, tools);
                                             PDMP3_HIP_EINVAL from a library built without -DPDMP3_WITH_RING_KERNEL (the default) */
int pdmp3_hip_decode_frames(pdmp3_hip_ctx* ctx,
                            const int16_t* d_spectra,
                            const pdmp3_gc_side* d_side,
                            int n_frames,
                            void* d_state,
                            int16_t* d_pcm,
                            int chunk_frames,
                            void* stream);

/* The granule kernel's hand-over scratch for bare calls is kept per HIP stream: 17 KB per frame of the largest such
 * launch seen on the stream (207 MB at the 12288-frame ceiling), for up to 32 streams, least recently used first out.
 * A caller that is done with a HIP stream -- or creates many short-lived ones -- gives the scratch back with this call
 * (it waits for the stream's launches).  pdmp3_hip_stream objects own theirs and free it when destroyed. */
int pdmp3_hip_release_stream_scratch(pdmp3_hip_ctx* ctx, void* stream);

/* How the latest decode launch of this engine (any thread) was laid out:
 * PDMP3_HIP_LAUNCH_CHUNKS = independent chunks with halos (k_decode), otherwise
 * the granule kernel (k_decode_g) with 8 / 16 wavefronts per workgroup.
 * For reports (bench.py names the kernel it timed from this), not for control. */
#define PDMP3_HIP_LAUNCH_NONE      0
#define PDMP3_HIP_LAUNCH_CHUNKS    1
#define PDMP3_HIP_LAUNCH_GRANULES8  8
#define PDMP3_HIP_LAUNCH_GRANULES16 16
#define PDMP3_HIP_LAUNCH_PERSISTENT 32   /* k_decode_p: workgroups of 16 wavefronts going round a range of frames each */
int pdmp3_hip_last_launch_kind(const pdmp3_hip_ctx* ctx);
/* The device's PCI address ("0000:c1:00.0") into buf (len >= 16): what a host stage needs to find the CPUs and the
 * memory next to the GPU (/sys/bus/pci/devices/<address>/local_cpulist, numa_node) -- the whole-stream decoder keeps
 * its helper threads and its pinned buffers there (include/pdmp3_bulk.h).  No reference counterpart. */
int pdmp3_hip_pci_bus_id(const pdmp3_hip_ctx* ctx, char* buf, int len);

/* Float PCM (not in the reference, whose only output is int16): the same decode, but what is stored is
 * the binary32 synthesis sum that P:2028-2031 scale by 32767, truncate and clip -- full scale is +-1.0, nothing is
 * clipped.  d_pcm: device, float; frame f occupies floats [f*2304, f*2304+2304), interleaved L, R (mono frames: the
 * first 1152).  The int16 output of pdmp3_hip_decode_frames is exactly clip(trunc(these * 32767)), which is how the
 * float form is pinned to the reference.  State and chunking as above (the two forms may alternate on one state). */
#define PDMP3_FRAME_PCM_F32_BYTES (1152 * 2 * 4)
int pdmp3_hip_decode_frames_f32(pdmp3_hip_ctx* ctx,
                                const int16_t* d_spectra,
                                const pdmp3_gc_side* d_side,
                                int n_frames,
                                void* d_state,
                                float* d_pcm,
                                int chunk_frames,
                                void* stream);

/* MPEG-2 LSF / MPEG-2.5 frames (pdmp3_gc_side.lsf != 0, above; SURVEY 8f #4 -- nothing in the reference: it rejects the
 * streams, pdmp3.c:1293).  n_frames consecutive frames of ONE stream, all LSF and all of one channel count; records and
 * spectra in the usual layout ([n_frames][2][2], of which only [0][ch] is read: an LSF frame is one granule).  The PCM
 * comes out in stream order, 576 sample-frames per frame: stereo frame f at bytes [f * 2304, + 2304); mono frame f at
 * byte (f / 2) * 4608 + (f % 2) * 1152, 1152 bytes (a PAIR of mono frames in the first half of a 4608-byte place, like
 * the granules of an MPEG-1 mono frame).  _f32: the same places counted in floats.  d_state as for
 * pdmp3_hip_decode_frames, and the same state block: MPEG-1 and LSF launches may follow each other on it. */
int pdmp3_hip_decode_lsf_frames(pdmp3_hip_ctx* ctx, const int16_t* d_spectra, const pdmp3_gc_side* d_side,
                                int n_frames, void* d_state, int16_t* d_pcm, void* stream);
int pdmp3_hip_decode_lsf_frames_f32(pdmp3_hip_ctx* ctx, const int16_t* d_spectra, const pdmp3_gc_side* d_side,
                                    int n_frames, void* d_state, float* d_pcm, void* stream);

/* Same, additionally dumping float32 stage outputs for parity tests
 * (d_stages: float [n_frames][2][2][4][576]; stage 0 = after requantize +
 * reorder, 1 = after stereo, 2 = after antialias, 3 = after hybrid synthesis
 * + frequency inversion).  Single-workgroup, slow; test use only. */
int pdmp3_hip_decode_frames_stages(pdmp3_hip_ctx* ctx,
                                   const int16_t* d_spectra,
                                   const pdmp3_gc_side* d_side,
                                   int n_frames,
                                   void* d_state,
                                   int16_t* d_pcm,
                                   float* d_stages,
                                   void* stream);

/*
 * Synthetic-workload generator of SURVEY 8d (C2 / C5), counter-based
 * splitmix64 so every GPU can generate its own shard on device:
 * frames [first_frame, first_frame + n_frames) of the stream `seed`.
 * The same integer-only generator exists on the host in the oracle
 * (oracle/pdmp3_oracle.c: orc_generate_frames); tests check they agree.
 */
int pdmp3_hip_generate_frames(pdmp3_hip_ctx* ctx,
                              uint64_t seed,
                              int64_t first_frame,
                              int n_frames,
                              int16_t* d_spectra,
                              pdmp3_gc_side* d_side,
                              void* stream);

/* ------------------------------------------------------------------------
 * Host-buffer streaming helper: what the libmpg123-style API (include/pdmp3.h,
 * pdmp3_read) drives.  One pdmp3_hip_stream = one decoder handle's device
 * state (overlap + polyphase history), a HIP stream and pinned, library-owned
 * staging buffers; the sequential Huffman stage on the host fills gc records,
 * this call moves them with hipMemcpyAsync, runs the transforms and brings the
 * PCM back.  Replaces `Decode_L3(id)` at pdmp3.c:2453 for a batch of frames.
 * ---------------------------------------------------------------------- */
typedef struct pdmp3_hip_stream pdmp3_hip_stream;

int pdmp3_hip_stream_create(pdmp3_hip_ctx* ctx, int max_frames, pdmp3_hip_stream** out);
void pdmp3_hip_stream_destroy(pdmp3_hip_stream* hs);
/* zero the carried synthesis state (pdmp3_open_feed, pdmp3.c:2377-2378) */
int pdmp3_hip_stream_reset(pdmp3_hip_stream* hs);
/* pinned staging buffers to fill / read: capacity max_frames frames each */
int16_t* pdmp3_hip_stream_spectra(pdmp3_hip_stream* hs);
pdmp3_gc_side* pdmp3_hip_stream_side(pdmp3_hip_stream* hs);
const int16_t* pdmp3_hip_stream_pcm(pdmp3_hip_stream* hs);
/* decode frames [0, n_frames) of the staging buffers; synchronous */
int pdmp3_hip_stream_decode(pdmp3_hip_stream* hs, int n_frames);

/* Pipelined form for bulk decoding of one long stream (the C3 / C4 corpora of
 * SURVEY 8d): `n_slots` (1..8) independent staging slots of `max_frames` frames.
 * While the host fills slot w+1, slot w is uploading / running / downloading.
 * Batches are decoded in SUBMIT order, each from the synthesis state the
 * previous one left (the same carry Decode_L3's static buffers give the
 * reference, pdmp3.c:1777, 2126), whatever slot they sit in.  The accessors
 * above and pdmp3_hip_stream_decode are slot 0. */
int pdmp3_hip_stream_create_slots(pdmp3_hip_ctx* ctx, int max_frames, int n_slots, pdmp3_hip_stream** out);
int pdmp3_hip_stream_slots(const pdmp3_hip_stream* hs);
int pdmp3_hip_stream_capacity(const pdmp3_hip_stream* hs);
int16_t* pdmp3_hip_stream_slot_spectra(pdmp3_hip_stream* hs, int slot);
pdmp3_gc_side* pdmp3_hip_stream_slot_side(pdmp3_hip_stream* hs, int slot);
const int16_t* pdmp3_hip_stream_slot_pcm(pdmp3_hip_stream* hs, int slot);
/* enqueue H2D + transforms + D2H of the slot's first n_frames frames; returns at once */
int pdmp3_hip_stream_submit(pdmp3_hip_stream* hs, int slot, int n_frames);
/* PCM of pdmp3_hip_stream_submit / _decode as float from now on (on != 0; see pdmp3_hip_decode_frames_f32) or as
 * int16 again.  Call with nothing in flight: the slots' PCM buffers are re-allocated (9216 bytes per frame for float)
 * and the pdmp3_hip_stream_*pcm accessors return the new ones, to be read as float.  Not for the _to / _bits forms. */
int pdmp3_hip_stream_set_f32(pdmp3_hip_stream* hs, int on);
/* The records of the following submits are LSF frames (on != 0: decoded like pdmp3_hip_decode_lsf_frames, PCM in its layout;
 * the _to forms take row_bytes 2304 for stereo and 1152 for mono frames then) or MPEG-1 frames again (0).  Batches are
 * homogeneous: the host splits them where the stream changes version or channel count.  The _bits / _pool forms take it
 * too: their frame bits are then in the LSF form (pdmp3_frame_bits, below), and the device builds LSF records from them. */
int pdmp3_hip_stream_set_lsf(pdmp3_hip_stream* hs, int on);
/* undo the slot's latest pdmp3_hip_stream_submit beyond its first keep_frames frames: the carried synthesis state
 * (P:1755, P:1983) becomes what it was after frame keep_frames - 1 of that batch.  Blocks.  (pdmp3_read hands frames
 * out in the reference's order; frames it decoded ahead that the reference turns out not to reach are taken back.) */
int pdmp3_hip_stream_rewind(pdmp3_hip_stream* hs, int slot, int keep_frames);

/* ------------------------------------------------------------------------
 * Bitstream-level input: scalefactor + Huffman decoding on the
 * device.  The host keeps only the strictly sequential part of Read_Frame
 * (pdmp3.c:1217-1244: header sync, side info P:1129-1200, bit reservoir
 * P:1096-1122) and hands over, per frame, the side info and a snapshot of the
 * reservoir buffer g_main_data_vec (P:137) as Get_Main_Data left it.  One lane
 * per granule-channel then does what Read_Main_L3 (P:1376-1437), Read_Huffman
 * (P:2051-2115) and Huffman_Decode (P:1593-1643) do, a second small kernel
 * carries scalefactors / count1 from frame to frame exactly as the reference's
 * never-cleared g_main_data / g_side_info do, and the transform
 * kernel runs on the records in place: decoded spectra never cross PCIe
 * (2144 B per frame up instead of 5120).
 * ---------------------------------------------------------------------- */
#define PDMP3_RESERVOIR_BYTES 2064          /* 2048 + 16: one row per frame              */

typedef struct pdmp3_gc_bits {              /* side info of one granule-channel, P:74-93 */
  uint16_t part2_3_length;                  /* P:75 */
  uint16_t big_values;                      /* P:76 */
  uint8_t  global_gain;                     /* P:77 */
  uint8_t  scalefac_compress;               /* P:78 */
  uint8_t  flags;                           /* PDMP3_GC_* exactly as in pdmp3_gc_side    */
  uint8_t  table_select[3];                 /* P:84 */
  uint8_t  subblock_gain[3];                /* P:85 */
  uint8_t  region0_count, region1_count;    /* P:86-87 (the implicit 8 / 7 and 20 - r0 of
                                               P:1177-1180 already filled in)            */
  uint8_t  count1table_select;              /* P:90 */
} pdmp3_gc_bits;                            /* 16 bytes */

/* pdmp3_frame_bits.frame only: the parse state that survives frames (scalefactors, count1: SURVEY H4-H6) is zero
 * before this frame -- what a freshly allocated handle of the reference starts with.  Lets several independent
 * streams follow each other through one pdmp3_hip_stream without a host-side reset in between (the synthesis
 * state has PDMP3_FR_RESET for that).  Not copied into the gc records. */
#define PDMP3_FR_NEWSTREAM       0x80u

typedef struct pdmp3_frame_bits {
  uint8_t  frame;                           /* PDMP3_FR_* (+ PDMP3_FR_NEWSTREAM) */
  uint8_t  scfsi[2];                        /* [ch]: bit b = band group b reuses granule 0, P:73 */
  uint8_t  iso;                             /* PDMP3_ISO_* of include/pdmp3.h for this frame (0 = the reference's behaviour):
                                               TABLE33 selects the code book, SF21 / SF12 keep the one-past-the-end
                                               scalefactor slots of the records zero, MS_BOUND / IS_SHORT / IS_BOUND
                                               become the records' PDMP3_GC_ISO_* bits */
  uint8_t  lsf;                             /* 0 = an MPEG-1 frame; 1 = MPEG-2 LSF, 2 = MPEG-2.5 (PDMP3_LSF_VERSION_MASK) */
  uint8_t  sfc_hi;                          /* LSF: bit ch = bit 8 of channel ch's 9-bit scalefac_compress */
  uint8_t  reserved[10];                    /* must be zero */
  pdmp3_gc_bits gc[4];                      /* [gr][ch] */
} pdmp3_frame_bits;                         /* 80 bytes */

/* The LSF form of pdmp3_frame_bits (ISO/IEC 13818-3; pdmp3_gc_side.lsf above; not the reference).  An LSF frame is ONE
 * granule: gc[0][ch] hold its side info exactly as for MPEG-1, gc[2] and gc[3] are zero and ignored, scfsi is zero.
 *   lsf                 the version; the sampling frequency is kLsfSampleRates[3 * lsf + (frame & 3)] (lsf_tables.h)
 *   gc[ch].scalefac_compress + ((sfc_hi >> ch) & 1) << 8
 *                       the 9-bit scalefac_compress, resolved on the device into the four partitions' slen and sizes
 *                       (lsf_tables.h lsf_slen_of / kLsfNsfb; channel 1 of a frame with mode_extension bit 0 set takes the
 *                       intensity-stereo code, which frame's PDMP3_FR_MODEEXT says)
 *   gc[ch].flags        PDMP3_GC_PREFLAG set where scalefac_compress >= 500 implies it
 *   gc[ch].region0_count / region1_count   the implicit 7 / 8 and 20 - region0_count of a window-switching block filled
 *                       in, as for MPEG-1; the boundaries come from the LSF long-band table of the frame's rate
 *   gc[ch].count1table_select   2 where the stream's bit is set (the standard's table B)
 * A window of pdmp3_hip_stream_submit_bits / _pool_to is homogeneous: all of its frames are LSF (pdmp3_hip_stream_set_lsf
 * on) and of one channel count, or all MPEG-1 (off).  The records the device builds from it are the host stage's, byte for
 * byte, in the per-frame layout (gc records [1][ch] of an LSF frame: frame, iso and lsf bytes only). */

/* pinned staging of a slot: n frames of side info and n reservoir rows */
pdmp3_frame_bits* pdmp3_hip_stream_slot_bits(pdmp3_hip_stream* hs, int slot);
uint8_t* pdmp3_hip_stream_slot_reservoir(pdmp3_hip_stream* hs, int slot);
/* like pdmp3_hip_stream_submit, from bits: H2D, unpack, merge, transforms, D2H of the PCM */
int pdmp3_hip_stream_submit_bits(pdmp3_hip_stream* hs, int slot, int n_frames);
/* Pinned host memory for PCM that should not be copied twice: with a destination inside such an allocation -- or in
 * device memory, for consumers on the GPU -- the _to forms below move a batch's PCM straight to it (row_bytes 4608, or 2304 to pack mono frames densely)
 * instead of into the slot's staging buffer; pdmp3_hip_stream_wait() then means "it is there". */
int pdmp3_hip_host_alloc(size_t bytes, void** out);
void pdmp3_hip_host_free(void* p);
int pdmp3_hip_host_is_pinned(const void* p, size_t bytes);          /* [p, p + bytes): 1 = pinned host memory, 2 = device memory
                                                                       (both are valid _to destinations), 0 = neither */
/* plain copy of `bytes` from host memory to a destination pdmp3_hip_host_is_pinned() classified (1 or 2); blocks until
 * it is done.  The whole-stream decoder uses it for the windows that cannot go to a DEVICE destination directly
 * (mixed mono / stereo frames, the clipped tail): they are staged in the slot's pinned buffer and copied from there. */
int pdmp3_hip_copy_to_dest(void* dst, const void* src_host, size_t bytes);
int pdmp3_hip_stream_submit_to(pdmp3_hip_stream* hs, int slot, int n_frames, void* pinned_dst, int row_bytes);
int pdmp3_hip_stream_submit_bits_to(pdmp3_hip_stream* hs, int slot, int n_frames, void* pinned_dst, int row_bytes);

/* Compact form of the same input.  A frame's reservoir buffer is the last main_data_begin bytes of what was there
 * before plus the frame's own main data (Get_Main_Data, P:1096-1122), so consecutive snapshots overlap almost
 * entirely: instead of 2064 bytes per frame the host uploads a POOL -- the main-data bytes of the window's frames,
 * each appended once, in stream order -- and a descriptor per frame, and the device rebuilds the rows
 * (k_rows; unpack_core.h row_byte) before k_unpack reads them.  Byte j of frame f's buffer is
 *     pool[row_off(f) + j]                 j <  top(f)       written by this frame's Get_Main_Data
 *     pool[row_off(g) + j]                 j >= top(f)       left there by frame g, the nearest earlier frame of the
 *                                                            same SEGMENT with top(g) > j (the reference never clears
 *                                                            g_main_data_vec: corrupt streams read those bytes); g is
 *                                                            found along the `up` links, each to a larger top
 *     pool[s_off + j]                      no such frame     the buffer as it was before the segment began
 * A segment is a run of frames over which "the buffer's valid bytes are the tail of the pool" holds; it starts with a
 * 2064-byte image of the buffer (at s_off) followed by a copy of its last bytes, and a new one starts at every
 * window and after anything irregular (reservoir underflow H9, short reads H18).  A frame whose buffer does not fit
 * the rule carries its own image: row_off = s_off, top = 2064.  ~1.1 KB per frame up instead of 2144. */
typedef struct pdmp3_row_desc {
  uint32_t row_off;                         /* pool offset of byte 0 of the frame's buffer            */
  uint32_t s_off;                           /* pool offset of its segment's 2064-byte image            */
  uint16_t top;                             /* bytes [0, top) come from row_off                        */
  uint16_t back;                            /* frames before this one in its segment                   */
  uint16_t up;                              /* distance (in frames) to the nearest earlier frame of the
                                             * segment with a larger top; 0 = none (the image at s_off) */
  uint16_t reserved;
} pdmp3_row_desc;                           /* 16 bytes */
pdmp3_row_desc* pdmp3_hip_stream_slot_rowdesc(pdmp3_hip_stream* hs, int slot);
uint8_t* pdmp3_hip_stream_slot_pool(pdmp3_hip_stream* hs, int slot);       /* = pdmp3_hip_stream_slot_reservoir's memory */
#define PDMP3_POOL_SLACK_BYTES 8192         /* a window of ONE frame still takes a segment start + its frame + an image */
size_t pdmp3_hip_stream_pool_bytes(const pdmp3_hip_stream* hs);            /* capacity of a slot's pool:
                                                                            * max_frames * 2064 + PDMP3_POOL_SLACK_BYTES */
/* like pdmp3_hip_stream_submit_bits_to, from the slot's bits, descriptors and the first pool_bytes of its pool */
int pdmp3_hip_stream_submit_pool_to(pdmp3_hip_stream* hs, int slot, int n_frames, size_t pool_bytes, void* pinned_dst, int row_bytes);

/* Clips (include/pdmp3_bulk.h pdmp3_amd_bulk_decode_clips): a window whose PCM does not go to one contiguous place.  The
 * batch is decoded like pdmp3_hip_stream_submit_bits (snapshot rows), its PCM stays in the slot's device buffer -- frame f at
 * byte f * 4608 of an MPEG-1 window, in pdmp3_hip_decode_lsf_frames' layout in an LSF one -- and k_clip_pack then copies
 * each piece: `bytes` bytes from offset `src` of that buffer to device address `dst` (memory of the engine's device: a
 * caller's tensor, or the slot's clip stage).  Pieces must not overlap each other's destinations; src + bytes stays inside
 * the batch's PCM.  stage_bytes > 0: the first stage_bytes of the slot's clip stage (pdmp3_hip_stream_slot_clip_stage) are
 * then downloaded into the slot's pinned PCM buffer (pdmp3_hip_stream_slot_pcm), from where the host copies them to host
 * destinations.  At most max_frames pieces; returns at once, pdmp3_hip_stream_wait() as for the other submits. */
typedef struct pdmp3_clip_piece {
  uint64_t dst;                             /* device address of the piece's first byte                 */
  uint32_t src;                             /* byte offset in the batch's PCM                           */
  uint32_t bytes;
} pdmp3_clip_piece;                         /* 16 bytes */
int pdmp3_hip_stream_submit_bits_clips(pdmp3_hip_stream* hs, int slot, int n_frames, const pdmp3_clip_piece* pieces, int n_pieces,
                                       size_t stage_bytes);
/* device memory of max_frames * 4608 bytes per slot (allocated on first use), NULL on failure */
void* pdmp3_hip_stream_slot_clip_stage(pdmp3_hip_stream* hs, int slot);

/* Clips as float batches (include/pdmp3_bulk.h pdmp3_amd_bulk_decode_clips_audio).  The clips' int16 PCM
 * is placed by clip windows (above) in a device stage the stream object owns; k_clip_audio (resample.hip) then writes every
 * clip's row of the batch: planar float32, channels made (downmix / doubling), resampled by the clip's filter table or
 * copied at the stream's own rate, zeros behind the stream's end.
 * One clip of the launch: its staged frames are [frame0, frame0 + n_frames) of its stream, frame f's PCM at
 * src + (frames[frame_tab + f - frame0] >> 1) * 1152 and mono when that entry's bit 0 is set (a stereo frame: spf samples
 * of L, R interleaved; a mono one: spf samples).  Output sample t of channel c, dst[c * chan_stride + t], is sample
 * start + t of the stream at the new rate: j M = q L + r picks row r of the clip's table (taps coefficients at
 * tables[table + r * taps]), whose tap k multiplies input sample q + d0 + k (0 outside [0, n_in)); M == L: input sample j
 * itself; j >= n_out: 0.0.  flags: where the workgroups keep the input span and the table (the host's choice by size). */
#define PDMP3_AUDIO_TILE 1024                /* output samples (per channel) of a workgroup                */
#define PDMP3_AUDIO_LDS_BYTES (64u * 1024u) /* LDS a workgroup may take: span_cap floats per channel, then the table */
#define PDMP3_AUDIO_LDS_X 1u                /* the tile's input span is converted into LDS first */
#define PDMP3_AUDIO_LDS_TABLE 2u            /* ... and the whole table lies behind it */
typedef struct pdmp3_audio_desc {
  uint64_t src;                             /* device address of the clip's staged PCM (16-byte aligned)  */
  uint64_t dst;                             /* device address of channel 0's first float                  */
  uint64_t chan_stride;                     /* floats between the channels of the row                     */
  int64_t start;                            /* the row's first output sample                              */
  int64_t n_in, n_out;                      /* N and J: samples of the stream at its rate, at the new one */
  int64_t frame0;
  uint32_t n_frames, frame_tab;
  uint32_t M, L;                            /* in / gcd, out / gcd                                        */
  uint32_t spf;                             /* samples per frame and channel: 1152 or 576                 */
  uint32_t table;                           /* floats in front of the clip's table in `tables`            */
  int32_t taps, d0;
  uint32_t flags, span_cap;                 /* PDMP3_AUDIO_LDS_*; input samples a tile reads at most      */
} pdmp3_audio_desc;                         /* 96 bytes */
/* The stream object's audio stages: device memory (hipMalloc, kept and grown on demand; call with nothing of the audio
 * path in flight).  which = 0: the clips' int16 PCM; 1: float rows of clips whose destination is host memory; 2: the
 * resampled signal the log-mel call reads (below); 3: what the tempogram call keeps between its kernels (log-mel, envelope,
 * tempogram), the separation call its spectrum, or the long MFCC call its log-mel and thresholds.  NULL on failure. */
void* pdmp3_hip_stream_audio_stage(pdmp3_hip_stream* hs, int which, size_t bytes);
/* Uploads the launch's tables (descs, frames, tables: host memory) and runs k_clip_audio on the slot's HIP stream, behind
 * whatever the slot ran last (the last clip window's k_clip_pack); n_samples output samples per row, channels = 1 or 2.
 * Blocks until the rows are written. */
int pdmp3_hip_clip_audio(pdmp3_hip_stream* hs, int slot, const pdmp3_audio_desc* descs, int n_clips, const uint32_t* frames,
                         size_t n_frames, const float* tables, size_t n_coef, long long n_samples, int channels);
/* plain copy of `bytes` from device memory (an audio stage) to host memory; blocks until it is done */
int pdmp3_hip_copy_from_device(void* host_dst, const void* dev_src, size_t bytes);

/* Log-mel features of clips (include/pdmp3_bulk.h pdmp3_amd_bulk_decode_clips_mel).  k_clip_mel
 * (mel.hip) reads rows of the resampled signal that k_clip_audio wrote into audio stage 2 and writes [n_mels][n_frames]
 * floats per channel.  One clip of the launch: sample t of channel c of its row is src[c * src_chan_stride + t], 0 <= t <
 * n_in, and stands for the signal at start - n_fft / 2 + lead + t: `lead` zeros lie in front of it (a clip that starts inside
 * the stream's first n_fft / 2 samples); everything outside [0, n_in) is 0.  Frame f reads t = f hop - lead + n, n < n_fft. */
typedef struct pdmp3_mel_desc {
  uint64_t src, dst;                        /* device addresses: channel 0's first sample, channel 0's first output float */
  uint64_t src_chan_stride, dst_chan_stride; /* floats between the channels                                              */
  uint32_t lead, pad_;
} pdmp3_mel_desc;                           /* 40 bytes */
typedef struct pdmp3_mel_params {
  int64_t n_in;                             /* samples of a row                                                         */
  int32_t n_fft, rows;                      /* N; N rounded up to 4: the DFT table's rows                               */
  int32_t hop, row_pad;                     /* H; LDS floats between two hops' worth of the signal                      */
  int32_t bins16, n_mels, mels16;           /* Kp, n_mels, n_mels rounded up to 16                                      */
  int32_t n_frames, tile;                   /* F; frames of a workgroup: 16 or 32                                       */
  int32_t channels, out_mode;
  float floor;
  uint32_t span_floats;                     /* LDS floats of the workgroup's first region (the signal, then the mel tile) */
  uint32_t lds_bytes;
} pdmp3_mel_params;
#define PDMP3_MEL_LDS_SOFT (64u * 1024u)    /* a tile of 32 frames is taken where it fits this, else 16 frames          */
#define PDMP3_MEL_LDS_MAX (160u * 1024u - 64u) /* ... which a static array of this size serves (k_clip_mel_big)  */
/* Uploads the descriptors, the DFT table (rows x 2 bins16 floats) and the transposed padded filterbank (bins16 x mels16
 * floats) -- host memory -- and runs k_clip_mel (and, out_mode 3, the finishing kernel) on the slot's HIP stream.  Blocks
 * until the rows are written. */
int pdmp3_hip_clip_mel(pdmp3_hip_stream* hs, int slot, const pdmp3_mel_desc* descs, int n_clips, const float* dft, const float* fbt,
                       const pdmp3_mel_params* params);

/* Kaldi-style filterbank features of clips (include/pdmp3_bulk.h pdmp3_amd_bulk_decode_clips_fbank).
 * k_clip_fbank (fbank.hip) reads rows of the resampled signal in audio stage 2 and writes [n_frames][D] floats per channel,
 * D = n_mels + use_energy, coefficients innermost.  One clip of the launch: sample t of channel c of its row is
 * src[c * src_chan_stride + t], 0 <= t < n_in, the signal at start + t; everything outside [0, n_in) is 0.  Frame f reads
 * t = f hop + n, n < win.  valid: the frames wholly inside the stream (subtract_mean averages over them). */
typedef struct pdmp3_fbank_desc {
  uint64_t src, dst;                        /* device addresses: channel 0's first sample, channel 0's first output float */
  uint64_t src_chan_stride, dst_chan_stride; /* floats between the channels                                              */
  uint32_t valid, pad_;
} pdmp3_fbank_desc;                         /* 40 bytes: pdmp3_mel_desc's layout, `valid` where that has `lead` (the host fills one array) */
typedef struct pdmp3_fbank_params {
  int64_t n_in;                             /* samples of a row                                                         */
  int32_t win, rows;                        /* Nw; Nw rounded up to 4: the folded table's rows                          */
  int32_t n_dft;                            /* N: Nw, or the least power of two >= Nw                                   */
  int32_t hop, row_pad;                     /* H; LDS floats between two hops' worth of the signal                      */
  int32_t bins16, n_mels, mels16;           /* N / 2 rounded up to 16, n_mels, n_mels rounded up to 16                  */
  int32_t n_frames, tile;                   /* F; frames of a workgroup: 16 or 32                                       */
  int32_t channels, out_mode;               /* out_mode 0: M (and E), 1: their logarithms                               */
  int32_t use_energy, htk_compat;           /* the energy column: in front, or (htk_compat) behind the mel columns      */
  int32_t subtract_mean, remove_dc;         /* remove_dc: the energy is taken of s - mean (the table carries it for the DFT) */
  float scale;                              /* of the samples the energy is taken of (the table carries it for the DFT) */
  float eps;                                /* the floor of the logarithms: 2^-23                                       */
  float energy_log_floor;                   /* ln energy_floor as binary32, -inf for none                               */
  uint32_t span_floats;                     /* LDS floats of the workgroup's first region (the signal, then the mel tile) */
  uint32_t lds_bytes;
} pdmp3_fbank_params;
/* Uploads the descriptors, the folded table (rows x 2 bins16 floats) and the transposed padded filterbank (bins16 x mels16
 * floats) -- host memory -- into one device block and runs k_clip_fbank (and, subtract_mean, k_clip_fbank_finish) on the
 * slot's HIP stream.  The LDS limits are the log-mel call's (PDMP3_MEL_LDS_SOFT / _MAX).  Blocks until the rows are written. */
int pdmp3_hip_clip_fbank(pdmp3_hip_stream* hs, int slot, const pdmp3_fbank_desc* descs, int n_clips, const float* dft, const float* fbt,
                         const pdmp3_fbank_params* params);

/* Kaldi-style MFCC features of clips (include/pdmp3_bulk.h pdmp3_amd_bulk_decode_clips_mfcc).
 * k_clip_mfcc (mfcc.hip) is k_clip_fbank up to the mel tile, takes its logarithm in LDS and multiplies it by the folded DCT
 * table: [n_frames][n_ceps] floats per channel, cepstra innermost.  The descriptor is pdmp3_fbank_desc.  fb: the filterbank
 * stages' parameters as pdmp3_hip_clip_fbank takes them, with out_mode 1, and span_floats / lds_bytes of this kernel: the
 * first region as there, then max(bins16 + 2, ceps16 + 1) floats a frame -- the powers, later the cepstra [tile][ceps16 + 1]
 * (a row's spare float holds the frame's energy). */
typedef struct pdmp3_mfcc_params {
  pdmp3_fbank_params fb;
  int32_t n_ceps, ceps16;                   /* num_ceps (1 .. n_mels); rounded up to 16: the folded DCT table's columns    */
} pdmp3_mfcc_params;
/* Uploads the descriptors, the folded table (rows x 2 bins16 floats), the transposed padded filterbank (bins16 x mels16) and
 * the folded DCT table (mels16 x ceps16: lifter, htk_compat's sqrt 2 and column order in it, zeros in the energy's column and
 * in the padding) -- host memory -- into one device block with the column sums behind them and runs k_clip_mfcc (and,
 * subtract_mean, k_clip_mfcc_finish) on the slot's HIP stream.  Blocks until the rows are written. */
int pdmp3_hip_clip_mfcc(pdmp3_hip_stream* hs, int slot, const pdmp3_fbank_desc* descs, int n_clips, const float* dft, const float* fbt,
                        const float* dct, const pdmp3_mfcc_params* params);

/* The short-time Fourier transform of clips (include/pdmp3_bulk.h pdmp3_amd_bulk_decode_clips_stft).
 * k_clip_stft (stft.hip) reads rows of the resampled signal in audio stage 2 as k_clip_mel does -- the descriptor is
 * pdmp3_mel_desc -- and writes [bins][n_frames] floats per channel, frames innermost; out_mode 0: [bins][n_frames][2], Re and
 * Im interleaved.  The LDS of a workgroup: span_floats for the tile's span in chunks of hop + row_pad floats, then a staging
 * tile per wave of (out_mode 0 ? 2 : 1) planes of 16 rows of tile + 4 floats. */
typedef struct pdmp3_stft_params {
  int64_t n_in;                             /* samples of a row                                                         */
  int32_t n_fft, rows;                      /* N; N rounded up to 4: the folded table's rows                            */
  int32_t hop, row_pad;                     /* H; LDS floats between two hops' worth of the signal                      */
  int32_t bins, bins16;                     /* K = N / 2 + 1; Kp = K rounded up to 16                                   */
  int32_t n_frames, tile;                   /* F; frames of a workgroup: 16 or 32                                       */
  int32_t channels, out_mode;               /* out_mode 0 complex, 1 magnitude, 2 power, 3 ln, 4 log10                  */
  float floor;                              /* of the logarithms (modes 3 and 4)                                        */
  uint32_t span_floats;                     /* LDS floats of the tile's span, a multiple of 4                           */
  uint32_t lds_bytes;
} pdmp3_stft_params;
/* Uploads the descriptors and the folded table (rows x 2 bins16 floats: window and scale in it) -- host memory -- and runs
 * k_clip_stft on the slot's HIP stream.  The LDS limits are the log-mel call's (PDMP3_MEL_LDS_SOFT / _MAX).  Blocks until the
 * rows are written. */
int pdmp3_hip_clip_stft(pdmp3_hip_stream* hs, int slot, const pdmp3_mel_desc* descs, int n_clips, const float* table,
                        const pdmp3_stft_params* params);

/* The short-time Fourier transform of clips at n_fft 2048 and 4096 (include/pdmp3_bulk.h
 * pdmp3_amd_bulk_decode_clips_stft_long).  k_clip_stft_long (stft_long.hip) reads the rows as
 * k_clip_stft does (pdmp3_mel_desc) and writes the same layouts.  N = 64 n2; a workgroup of eight waves takes `tile` frames
 * and 16 of the 64 values of k1.  Its LDS: span_floats for the tile's span, plain ((tile - 1) hop + n_fft floats; later the
 * staging tile of (out_mode 0 ? 2 : 1) x 16 x n2 / 2 x (tile + 1) floats), then Z: tile x n2 x 32 floats. */
typedef struct pdmp3_stft_long_params {
  int64_t n_in;                             /* samples of a row                                                         */
  int32_t n_fft, n2;                        /* N: 2048 or 4096; N / 64                                                  */
  int32_t hop, bins;                        /* H; K = N / 2 + 1                                                         */
  int32_t n_frames, tile;                   /* F; frames of a workgroup: 16 or 8 (N 2048), 8 or 4 (N 4096)              */
  int32_t channels, out_mode;               /* out_mode 0 complex, 1 magnitude, 2 power, 3 ln, 4 log10                  */
  float floor;                              /* of the logarithms (modes 3 and 4)                                        */
  uint32_t span_floats;                     /* LDS floats of the first region, a multiple of 4                          */
  uint32_t lds_bytes;
} pdmp3_stft_long_params;
/* Uploads the descriptors and the four tables (one block of n_fft + 8192 + 2 n2^2 + 128 n2 floats: wt, the 64-point DFT, the
 * n2-point half DFT, the twiddles; csrc/stft_long_core.h has the layouts) -- host memory -- and runs k_clip_stft_long on the
 * slot's HIP stream.  lds_bytes <= PDMP3_MEL_LDS_MAX: the kernel has a static array of that size.  Blocks until the rows are
 * written. */
int pdmp3_hip_clip_stft_long(pdmp3_hip_stream* hs, int slot, const pdmp3_mel_desc* descs, int n_clips, const float* tables,
                             const pdmp3_stft_long_params* params);

/* Log-mel features of clips at n_fft 2048 and 4096 (include/pdmp3_bulk.h pdmp3_amd_bulk_decode_clips_mel_long; DESIGN.md
 * section 15).  k_clip_mel_long (mel_long.hip) reads the rows as k_clip_stft_long does (pdmp3_mel_desc) and writes
 * [n_mels][n_frames] floats per channel, frames innermost.  N = 64 n2; a workgroup of eight waves takes `tile` frames and all
 * four tiles of k1, one after the other.  Its LDS: span_floats for the tile's span, plain ((tile - 1) hop + n_fft floats, kept
 * for all four), then Z: tile x n2 x 32 floats, then the powers of one tile of k1: tile x (8 n2 + 2) floats. */
typedef struct pdmp3_mel_long_params {
  int64_t n_in;                             /* samples of a row                                                         */
  int32_t n_fft, n2;                        /* N: 2048 or 4096; N / 64                                                  */
  int32_t hop, n_mels;                      /* H; the bands                                                             */
  int32_t mels16, n_frames;                 /* n_mels rounded up to 16: the operand's columns; F                        */
  int32_t tile, channels;                   /* frames of a workgroup: 16 or 8 (N 2048), 8 or 4 (N 4096)                 */
  int32_t out_mode;                         /* 0 power, 1 ln, 2 log10                                                   */
  float floor;                              /* of the logarithms                                                        */
  uint32_t span_floats;                     /* LDS floats of the span's region, a multiple of 4                         */
  uint32_t lds_bytes;
} pdmp3_mel_long_params;
/* Uploads the descriptors, the four tables (pdmp3_hip_clip_stft_long's block) and the filterbank operand (n_fft / 2 rows of
 * mels16 floats in the kernel's order of the bins; csrc/mel_long_core.h has the map) -- host memory -- into one block and runs
 * k_clip_mel_long on the slot's HIP stream.  lds_bytes <= PDMP3_MEL_LDS_MAX: the kernel has a static array of that size.
 * Blocks until the rows are written. */
int pdmp3_hip_clip_mel_long(pdmp3_hip_stream* hs, int slot, const pdmp3_mel_desc* descs, int n_clips, const float* tables,
                            const float* operand, const pdmp3_mel_long_params* params);

/* Spectral descriptors of clips at n_fft 2048 and 4096 (include/pdmp3_bulk.h pdmp3_amd_bulk_decode_clips_spectral; DESIGN.md
 * section 22).  k_clip_spectral (spectral.hip) reads the rows as k_clip_stft_long does (pdmp3_mel_desc) and writes [6][n_frames]
 * floats per channel, frames innermost: rms, zcr, centroid, bandwidth, rolloff, flatness.  N = 64 n2; a workgroup of eight
 * waves takes `tile` frames and all four tiles of k1, one after the other.  Its LDS: span_floats for the tile's span, plain
 * ((tile - 1) hop + n_fft floats, kept), then Z: tile x n2 x 32 floats, then the plane: tile x (n_fft / 2 + 1) floats, then
 * 8 x tile floats of results; csrc/spectral_core.h has the layouts. */
typedef struct pdmp3_spectral_params {
  int64_t n_in;                             /* samples of a row                                                         */
  int32_t n_fft, n2;                        /* N: 2048 or 4096; N / 64                                                  */
  int32_t hop, n_frames;                    /* H; F                                                                     */
  int32_t tile, channels;                   /* frames of a workgroup: 8 (N 2048) or 4 (N 4096)                          */
  double bin_hz;                            /* sr / N                                                                   */
  double roll_percent;                      /* inside (0, 1)                                                            */
  float amin, zcr_threshold;                /* the floor of the flatness' powers (> 0); the zero crossings' dead band (>= 0) */
  uint32_t span_floats;                     /* LDS floats of the span's region, a multiple of 4                         */
  uint32_t lds_bytes;
} pdmp3_spectral_params;
/* Uploads the descriptors and the four tables (pdmp3_hip_clip_stft_long's block) -- host memory -- and runs k_clip_spectral on
 * the slot's HIP stream, one launch per 32 768 clips.  lds_bytes <= PDMP3_MEL_LDS_MAX: the kernel has a static array of that
 * size.  Blocks until the rows are written. */
int pdmp3_hip_clip_spectral(pdmp3_hip_stream* hs, int slot, const pdmp3_mel_desc* descs, int n_clips, const float* tables,
                            const pdmp3_spectral_params* params);

/* Median-filter harmonic-percussive separation of clips (include/pdmp3_bulk.h pdmp3_amd_bulk_decode_clips_hpss; DESIGN.md
 * section 23).  k_clip_hpss (hpss.hip) reads what k_clip_stft_long wrote into audio stage 3 -- a descriptor's src: channel 0's
 * [bins][n_stage] magnitudes (out_mode 2: [bins][n_stage][2], Re and Im), src_chan_stride floats between the channels; stage
 * frame j is the clip's frame j - kernel_harm / 2 -- and writes [2][bins][n_frames] floats per channel at dst (out_mode 2:
 * [2][bins][n_frames][2]), component 0 harmonic, 1 percussive, frames innermost; lead is not read.  A workgroup of four waves
 * takes tile_bins x tile_frames elements; its LDS is the tile with 15 bins and 15 frames around it, of which kernel_perc / 2 and
 * kernel_harm / 2 are loaded, rows `pitch` floats apart (csrc/hpss_core.h). */
typedef struct pdmp3_hpss_params {
  int32_t n_fft, bins;                      /* N: 2048 or 4096; K = N / 2 + 1                                           */
  int32_t n_frames, n_stage;                /* F; F + kernel_harm - 1: the frames of a row of the stage                 */
  int32_t kernel_harm, kernel_perc;         /* odd, 3 .. 31: frames; bins                                               */
  int32_t tile_bins, tile_frames;           /* 64 x 64                                                                  */
  int32_t pitch, channels;                  /* tile_frames + 30                                                         */
  int32_t out_mode, power;                  /* 0 mask, 1 magnitude, 2 complex, 3 median; 1, 2, or 0 for +inf            */
  double margin_harm, margin_perc;          /* >= 1                                                                     */
  uint32_t lds_bytes, pad_;
} pdmp3_hpss_params;
/* Uploads the descriptors -- host memory -- and runs k_clip_hpss on the slot's HIP stream, one launch per 32 768 clips.  The
 * tile, the pitch and lds_bytes must be csrc/hpss_core.h's (pdmp3_amd_hpss_plan's), and lds_bytes <= PDMP3_MEL_LDS_MAX.  Blocks until the rows are written. */
int pdmp3_hip_clip_hpss(pdmp3_hip_stream* hs, int slot, const pdmp3_mel_desc* descs, int n_clips, const pdmp3_hpss_params* params);

/* MFCC, deltas and dB mel of clips (include/pdmp3_bulk.h pdmp3_amd_bulk_decode_clips_mfcc_long).  The
 * kernels of mfcc_long.hip read what k_clip_mel_long wrote into audio stage 3 -- a descriptor's src: channel 0's
 * [n_mels][n_stage] log10 mel, src_chan_stride floats between the channels, and behind the last channel's one float per
 * channel, the plane's threshold (written by k_clip_db_max, read by the others; only with use_top); stage frame j is the
 * clip's frame j - halo -- and write [(1 + deltas) n_mfcc][n_frames] floats per channel at dst (out_mode 1:
 * [n_mels][n_frames]), frames innermost; lead is not read.  A workgroup of k_clip_mfcc_long, four waves, takes `tile` frames:
 * its LDS is a plane [mels16][d_pitch] of dB values and a plane [ceps16][c_pitch] of cepstra (csrc/mfcc_long_core.h). */
typedef struct pdmp3_mfcc_long_params {
  int32_t n_mels, mels16;                   /* <= 256; rounded up to 16                                                  */
  int32_t n_mfcc, ceps16;                   /* <= 128; rounded up to 16 (out_mode 1: 0, 0)                               */
  int32_t n_frames, n_stage;                /* F; F + 2 halo: the frames of a row of the stage                           */
  int32_t halo, deltas;                     /* (delta_width - 1) / 2 with deltas > 0, else 0; 0 .. 2                     */
  int32_t tile, channels;                   /* 64                                                                        */
  int32_t d_pitch, c_pitch;                 /* 80, 84                                                                    */
  int32_t out_mode, use_top;                /* 0 mfcc, 1 db; 1: clamp at the plane's maximum - top_db                    */
  float top_db;                             /* fl32(top_db), >= 0, with use_top                                          */
  uint32_t lds_bytes;
  double taps[2][17];                       /* [order - 1][j + halo], binary64                                           */
} pdmp3_mfcc_long_params;
/* Uploads the descriptors and the table T [ceps16][mels16] -- host memory; dct may be NULL at out_mode 1 -- and runs, on the
 * slot's HIP stream and per 32 768 clips, k_clip_db_max (use_top) and then k_clip_mfcc_long or k_clip_db.  The tile, the
 * pitches and lds_bytes must be csrc/mfcc_long_core.h's (pdmp3_amd_mfcc_long_plan's), lds_bytes <= PDMP3_MEL_LDS_MAX.
 * Blocks until the rows are written. */
int pdmp3_hip_clip_mfcc_long(pdmp3_hip_stream* hs, int slot, const pdmp3_mel_desc* descs, int n_clips, const float* dct,
                             const pdmp3_mfcc_long_params* params);

/* The constant-Q transform of clips (include/pdmp3_bulk.h pdmp3_amd_bulk_decode_clips_cqt).
 * k_clip_cqt (cqt.hip) reads the rows as k_clip_stft does (pdmp3_mel_desc; a frame's span is rows0 samples, its centre the
 * sample h_0) and writes [n_bins][n_frames] floats per channel, frames innermost; out_mode 0: [n_bins][n_frames][2].  The table
 * is ragged: tile t of 16 bins has tile_rows[t] rows (a multiple of 4) of 32 floats from row tile_at[t] on, and its row r
 * multiplies the frame's sample tile_base[t] + r.  A workgroup of eight waves takes `tile` frames.  Its LDS: span_floats for
 * the tile's span in chunks of hop + row_pad floats, then 8 x 2 x 16 x 17 floats of partial sums. */
#define PDMP3_CQT_MAX_TILES 32
#define PDMP3_CQT_PART_FLOATS (8 * 2 * 16 * 17)
typedef struct pdmp3_cqt_params {
  int64_t n_in;                             /* samples of a row                                                         */
  int32_t rows0, half0;                     /* tile_rows[0]: what a frame reads; h_0: the frame's centre in it          */
  int32_t hop, row_pad;                     /* H; LDS floats between two hops' worth of the signal                      */
  int32_t n_bins, n_tiles;                  /* n_tiles = n_bins rounded up to 16, over 16                               */
  int32_t n_split;                          /* tiles 0 .. n_split - 1 are cut into eight segments of rows, one a wave   */
  int32_t n_frames, tile;                   /* F; frames of a workgroup: 16, 8 or 4                                     */
  int32_t channels, out_mode;               /* out_mode 0 complex, 1 magnitude, 2 power, 3 ln, 4 log10                  */
  float floor;                              /* of the logarithms (modes 3 and 4)                                        */
  uint32_t span_floats;                     /* LDS floats of the tile's span, a multiple of 4                           */
  uint32_t lds_bytes;
  int32_t tile_rows[PDMP3_CQT_MAX_TILES];   /* descending                                                               */
  int32_t tile_base[PDMP3_CQT_MAX_TILES];   /* h_0 - h_(16 t)                                                           */
  uint32_t tile_at[PDMP3_CQT_MAX_TILES];    /* the tile's first row in the table                                        */
} pdmp3_cqt_params;
/* Uploads the descriptors and the table (table_rows x 32 floats) -- host memory -- and runs k_clip_cqt on the slot's HIP
 * stream, once per 32 768 clips.  The LDS limits are the log-mel call's (PDMP3_MEL_LDS_SOFT / _MAX).  Blocks until the rows
 * are written. */
int pdmp3_hip_clip_cqt(pdmp3_hip_stream* hs, int slot, const pdmp3_mel_desc* descs, int n_clips, const float* table, size_t table_rows,
                       const pdmp3_cqt_params* params);

/* Chroma features of clips (include/pdmp3_bulk.h pdmp3_amd_bulk_decode_clips_chroma).  k_clip_chroma
 * (chroma.hip) is k_clip_cqt's tile loop with the values kept in LDS: where that kernel stores bin k of frame fl, this one
 * writes the same binary32 value to the q plane, [n_tiles x 16][17] floats from LDS float q_at on; after a barrier the classes
 * are folded into the class plane, [n_chroma][17] floats from class_at on, and after another one normalised and stored as
 * [n_chroma][n_frames] floats per channel, frames innermost.  The class plane lies over the partial sums (class_at =
 * cqt.span_floats): the barrier in front of the fold is behind every wave's last read of them.  cqt.out_mode is 1 or 2,
 * cqt.lds_bytes the whole workgroup's: span, partial sums and q plane. */
typedef struct pdmp3_chroma_params {
  pdmp3_cqt_params cqt;
  int32_t n_chroma, r;                      /* classes; r = bins_per_octave / n_chroma bins of an octave in a class     */
  int32_t base_class, chroma_norm;          /* the class of bin 0; 0 none, 1 L1, 2 L2, 3 max                            */
  float norm_floor;                         /* the divisor is max(d, norm_floor)                                        */
  uint32_t q_at, class_at;                  /* LDS floats in front of the q plane and of the class plane                */
} pdmp3_chroma_params;
/* As pdmp3_hip_clip_cqt, with k_clip_chroma / k_clip_chroma_big. */
int pdmp3_hip_clip_chroma(pdmp3_hip_stream* hs, int slot, const pdmp3_mel_desc* descs, int n_clips, const float* table, size_t table_rows,
                          const pdmp3_chroma_params* params);

/* Loudness of clips (include/pdmp3_bulk.h pdmp3_amd_bulk_decode_clips_loudness).  The rows are
 * k_clip_audio's in audio stage 2 (pdmp3_mel_desc with lead = 0: sample t of channel c is src[c * src_chan_stride + t], t <
 * n_in, src 16-byte aligned and src_chan_stride a multiple of 4); dst receives x * g, dst_chan_stride floats between the
 * channels.  A row is cut into blocks of PDMP3_LOUD_B samples and chunks of PDMP3_LOUD_CHUNK blocks; the K-weighting of a block
 * is y = Hm u + O s with s the four-value state of the two biquads at the block's start.  Five kernels (loudness.hip):
 *   k_loud_states  a wave a chunk: w_b = R u_b and the states from rest at the chunk's start, binary64, a wave-level scan
 *   k_loud_chain   a wave a row: the states at the chunks' starts, binary64, a wave-level scan over 64 chunks at a time
 *   k_loud_blocks  four waves a chunk: [Hm | O | O] [U ; S_hi ; S_lo] on v_mfma_f32_16x16x4_f32, y^2 into three partial
 *                  sub-block sums a wave and |x| into a peak a wave, both in one fixed order, no atomics
 *   k_loud_gate    a workgroup a clip: sub-block sums, blocks, gates, L, M, P, g in binary64; writes stats and momentary
 *   k_loud_scale   dst = x * g
 * The tables are made once per rate on the host (pdmp3_amd/host/clip_loudness.c), in binary64; Hm and O rounded once. */
#define PDMP3_LOUD_B 64                     /* samples of a block                                                        */
#define PDMP3_LOUD_CHUNK 64                 /* blocks of a chunk of the scan: 4096 samples                               */
#define PDMP3_LOUD_POWS 70                  /* Phi^k, k = 0 .. 64, then Phi^(64 * 2^k), k = 1 .. 5                       */
#define PDMP3_LOUD_LDS_BYTES (64 * 68 * 4)  /* k_loud_blocks: a chunk's samples, a block every 68 floats                 */
typedef struct pdmp3_loud_tables {
  double pow[PDMP3_LOUD_POWS][16];          /* powers of Phi [4 x 4], row-major                                          */
  double R[4][PDMP3_LOUD_B];                /* the state a block's samples leave behind                                  */
  float Hm[PDMP3_LOUD_B][PDMP3_LOUD_B];     /* lower-triangular Toeplitz of the impulse response: the kernel reads column 0 */
  float O[PDMP3_LOUD_B][4];                 /* the free response of a block to the state at its start                    */
} pdmp3_loud_tables;
typedef struct pdmp3_loud_params {
  int64_t n_in;                             /* T: samples of a row, < 2^31                                               */
  int32_t channels, q;                      /* 1 or 2; samples of a sub-block, (fs + 5) / 10                             */
  int32_t n_chunks, n_sub;                  /* ceil(T / 4096); I = T / q                                                 */
  int32_t n_mom, dual_mono;                 /* J = max(0, I - 3); G_0 = 2                                                */
  double target, peak_limit;                /* NaN: no gain; 0: no limit                                                 */
} pdmp3_loud_params;
/* stats_dst[i], mom_dst[i]: the device addresses of clip i's 8 floats and (or 0) n_mom floats.  Blocks until all is written. */
int pdmp3_hip_clip_loudness(pdmp3_hip_stream* hs, int slot, const pdmp3_mel_desc* descs, int n_clips, const pdmp3_loud_tables* tables,
                            const uint64_t* stats_dst, const uint64_t* mom_dst, const pdmp3_loud_params* params);

/* True peak, short-term loudness and loudness range of clips (include/pdmp3_bulk.h pdmp3_amd_bulk_decode_clips_r128; DESIGN.md
 * section 19): the loudness call's five kernels, two of them in their second instantiation (loudness.hip):
 *   k_loud_blocks<true>  besides the K-weighting, phases 1-3 of the 4x interpolator as banded Toeplitz products on the same
 *                        operands: 84 more v_mfma_f32_16x16x4_f32 a wave; max |y| into a second maximum a wave (part: 8 floats)
 *   k_loud_gate<true>    besides L, M, P: TP, the 3 s windows S_j, Smax, the two gates of the range and its two order
 *                        statistics by counting in LDS (n_rng <= PDMP3_R128_MAX_RANGE); the gain held to TP or P
 * k_loud_states, k_loud_chain and k_loud_scale are the loudness call's. */
#define PDMP3_R128_TAPS 12                  /* taps of a phase of the interpolator                                        */
#define PDMP3_R128_MAX_RANGE 4096           /* 3 s windows a second apart that k_loud_gate<true> ranks in LDS             */
typedef struct pdmp3_r128_params {
  pdmp3_loud_params loud;
  int32_t n_st, n_rng;                      /* Js = max(0, I - 29); Jr = ceil(Js / 10) <= PDMP3_R128_MAX_RANGE            */
  int32_t limit_true_peak, reserved;        /* 1: the gain is held to TP, 0: to P                                        */
} pdmp3_r128_params;
/* taps: [3][PDMP3_R128_TAPS] floats, c_p[d] of phases 1 .. 3.  stats_dst[i], mom_dst[i], st_dst[i]: the device addresses of
 * clip i's 16 floats, (or 0) n_mom floats and (or 0) n_st floats.  Blocks until all is written. */
int pdmp3_hip_clip_r128(pdmp3_hip_stream* hs, int slot, const pdmp3_mel_desc* descs, int n_clips, const pdmp3_loud_tables* tables,
                        const float* taps, const uint64_t* stats_dst, const uint64_t* mom_dst, const uint64_t* st_dst,
                        const pdmp3_r128_params* params);

/* Pitch of clips (YIN) (include/pdmp3_bulk.h pdmp3_amd_bulk_decode_clips_pitch).  k_clip_pitch (pitch.hip)
 * reads the rows as k_clip_stft does (pdmp3_mel_desc) and writes [3][n_frames] (out_mode 0: f0, d'(tau*), tau*) or
 * [tmax + 1][n_frames] (out_mode 1: the curve d') floats per channel, frames innermost.  A workgroup of frames_wg waves takes
 * frames_wg consecutive frames of one (clip, channel), one frame a wave.  Its LDS, in this order (csrc/pitch_core.h has the
 * indexing): span_floats floats for the span -- position x = p + 16 of it (p = 0: the first sample of the workgroup's first
 * frame; 16 zeros in front, zeros behind the span up to `ext` positions) lies at x + 2 (x >> 4) --, q_doubles binary64 prefix
 * sums of squares, 64 binary64 scratch values a wave, 256 tiles floats a wave for its curve, 4 floats a wave for its result. */
typedef struct pdmp3_pitch_params {
  int64_t n_in;                             /* samples of a row                                                         */
  double sr, threshold;                     /* the call's sampling frequency; the trough threshold                      */
  int32_t n, win, hop;                      /* N, W, H                                                                  */
  int32_t tmin, tmax;                       /* the lag range                                                            */
  int32_t tiles, ksteps;                    /* lag tiles of 256: ceil((tmax + 1) / 256) <= 8; ceil((W + 15) / 4)         */
  int32_t n_frames, frames_wg;              /* F; frames (waves) of a workgroup: 8, 4, 2 or 1                           */
  int32_t channels, out_mode;
  uint32_t ext;                             /* positions of the span region that are written: 16 + the span + its padding */
  uint32_t span_floats;                     /* LDS floats of the span region, a multiple of 4                           */
  uint32_t q_doubles;                       /* (frames_wg - 1) H + N + 1                                                */
  uint32_t lds_bytes;
} pdmp3_pitch_params;
/* Uploads the descriptors -- host memory -- and runs k_clip_pitch on the slot's HIP stream.  The LDS limits are the log-mel
 * call's (PDMP3_MEL_LDS_SOFT / _MAX).  Blocks until the rows are written. */
int pdmp3_hip_clip_pitch(pdmp3_hip_stream* hs, int slot, const pdmp3_mel_desc* descs, int n_clips, const pdmp3_pitch_params* params);

/* Onset strength, tempogram and tempo of clips (include/pdmp3_bulk.h pdmp3_amd_bulk_decode_clips_tempogram; DESIGN.md section
 * 21).  Three kernels (tempogram.hip), each reading what the one before wrote:
 *   k_clip_onset      a lane a frame: the log-mel [n_mels][n_mel_frames] that k_clip_mel_long wrote (frame 0 of it lies `lag`
 *                     frames in front of envelope frame 0) to the envelope [n_env], a binary64 sum over the bands
 *   k_clip_tempogram  (modes 1, 2) a wave a frame, frames_wg waves a workgroup: the windowed envelope x_f into the wave's own
 *                     skewed LDS span (csrc/pitch_core.h pitch_at; 16 zeros in front, zeros behind as far as the operands
 *                     reach: ext positions, span_floats floats), its autocorrelation on v_mfma_f32_16x16x4_f32 as
 *                     k_clip_pitch's with W = win, divided by r^(0) into the wave's curve (256 tiles + 8 floats), stored
 *                     [win][n_frames], frames innermost
 *   k_clip_tempo      (mode 2) a workgroup a (clip, channel), a thread a lag: the mean over the frames, log1p, the prior, the
 *                     argmax and the margin, in binary64
 * Envelope frame e is o[e - win / 2] in modes 1 and 2 (n_env = n_frames + win - 1), o[e] in mode 0 (n_env = n_frames). */
typedef struct pdmp3_tempogram_desc {
  uint64_t mel;                             /* device address of channel 0's log-mel; channels n_mels n_mel_frames apart        */
  uint64_t env;                             /* ... of channel 0's envelope; mode 0: the destination                             */
  uint64_t tg;                              /* ... of channel 0's tempogram (modes 1, 2); mode 1: the destination               */
  uint64_t dst;                             /* ... of channel 0's four floats (mode 2)                                          */
  uint64_t dst_chan_stride;                 /* floats between the channels of the destination                                   */
} pdmp3_tempogram_desc;                     /* 40 bytes */
typedef struct pdmp3_tempogram_params {
  double sr;                                /* the call's sampling frequency                                            */
  int32_t n_mels, lag, half;                /* half = (max_size - 1) / 2                                                */
  int32_t hop, win;                         /* H; Wt                                                                    */
  int32_t tiles, ksteps;                    /* lag tiles of 256: ceil(Wt / 256) <= 4; ceil((Wt + 15) / 4)               */
  int32_t n_frames, frames_wg;              /* F; frames (waves) of a workgroup: 8, 4, 2 or 1                           */
  int32_t n_mel_frames, n_env;              /* frames of the log-mel batch: n_env + lag; of the envelope                */
  int32_t channels, out_mode;
  uint32_t env_stride;                      /* floats between the channels of the envelope stage (modes 1, 2)           */
  uint32_t ext;                             /* positions of a wave's span that are written                              */
  uint32_t span_floats;                     /* LDS floats of a wave's span, a multiple of 4                             */
  uint32_t lds_bytes;
} pdmp3_tempogram_params;
/* Uploads the descriptors, the window (win floats) and the prior (win doubles) -- host memory -- and runs the kernels of
 * out_mode on the slot's HIP stream.  The LDS limits are the log-mel call's.  Blocks until the rows are written. */
int pdmp3_hip_clip_tempogram(pdmp3_hip_stream* hs, int slot, const pdmp3_tempogram_desc* descs, int n_clips, const float* window,
                             const double* prior, const pdmp3_tempogram_params* params);

/* pYIN pitch tracking of clips (include/pdmp3_bulk.h pdmp3_amd_bulk_decode_clips_pyin).  Two kernels
 * (pyin.hip) behind k_clip_pitch, which writes its out_mode 1 curve [tmax + 1][n_frames] into a stage:
 *   k_clip_pyin_obs   a wave a frame, frames_wg waves a workgroup: the frame's curve into LDS, its troughs in passes of 64 lags
 *                     (ballots and prefix counts, the counts per threshold carried in LDS), their probabilities in binary64,
 *                     their bins by a search in T_q, the observation row and v in LDS, stored [n_bins + 1][n_frames] (mode 1:
 *                     the destination) or [n_frames][n_bins + 1] (mode 0: the stage k_clip_pyin_path reads)
 *   k_clip_pyin_path  (mode 0) a workgroup a (clip, channel), sequential over the frames: the values of the 2 n_bins states
 *                     double-buffered in LDS as binary64 (the window's logarithms beside them), two band scans and one maximum per half a step, back-pointers two
 *                     bytes a state [n_frames][2 n_bins], the walk back by one thread, the four planes
 * The tables are one block of binary64 values in the order theta[n_thr] | w[n_thr] | wsum[n_thr + 1] | G[max_troughs] |
 * cN[max_troughs + 1] | T[n_bins] | ltri[2 hb + 1] (offsets -hb .. hb) | lZ[n_bins], then n_bins binary32 bin frequencies (csrc/pyin_core.h
 * pyin_table_layout; pdmp3_amd_pyin_tables fills it). */
typedef struct pdmp3_pyin_desc {
  uint64_t curve;                           /* device address of channel 0's curve; channels (tmax + 1) n_frames floats apart  */
  uint64_t obs;                             /* ... of channel 0's observation; mode 1: the destination, channels dst_chan_stride
                                               apart; mode 0: the stage, channels (n_bins + 1) n_frames apart                   */
  uint64_t bp;                              /* ... of channel 0's back-pointers (mode 0), channels 2 n_bins n_frames uint16 apart */
  uint64_t dst;                             /* ... of channel 0's output                                                        */
  uint64_t dst_chan_stride;                 /* floats between the channels of the destination                                   */
} pdmp3_pyin_desc;                          /* 40 bytes */
typedef struct pdmp3_pyin_params {
  double no_trough;                         /* no_trough_prob                                                           */
  double l_stay, l_sw, l0, lp0_u;           /* ln(1 - switch_prob), ln(switch_prob), ln(2^-1022), -ln(n_bins)           */
  float fill; int32_t use_bin;              /* plane 0 of an unvoiced frame: fill, or (use_bin) the bin's frequency      */
  int32_t tmin, tmax;                       /* the lag range of the curve                                               */
  int32_t n_thr, n_bins, hb;                /* thresholds; pitch bins n_b; half the transition band, Wd / 2             */
  int32_t max_troughs;                      /* (tmax - 1 - tmin) / 2 + 1: troughs lie two lags apart at least           */
  int32_t n_frames, frames_wg;              /* F; frames (waves) of a workgroup of k_clip_pyin_obs: 8, 4, 2 or 1        */
  int32_t channels, out_mode;
  int32_t path_threads;                     /* threads of a workgroup of k_clip_pyin_path: n_bins up to 64s, <= 1024    */
  uint32_t obs_lds_bytes, path_lds_bytes;   /* obs: <= PDMP3_MEL_LDS_SOFT; path: <= PDMP3_MEL_LDS_MAX                   */
  uint32_t reserved;
} pdmp3_pyin_params;
/* Uploads the descriptors and the tables -- host memory -- and runs k_clip_pyin_obs and (mode 0) k_clip_pyin_path on the slot's
 * HIP stream.  The geometry must be csrc/pyin_core.h's (pdmp3_amd_pyin_plan's).  Blocks until the rows are written. */
int pdmp3_hip_clip_pyin(pdmp3_hip_stream* hs, int slot, const pdmp3_pyin_desc* descs, int n_clips, const double* tables,
                        const pdmp3_pyin_params* params);

/* Beat tracking of clips (include/pdmp3_bulk.h pdmp3_amd_bulk_decode_clips_beats).  Three kernels
 * (beat.hip) behind the tempogram call's, which wrote the onset envelope (and, where the tempo is estimated, k_clip_tempo's four
 * floats) into a stage:
 *   k_clip_beat_score  a workgroup a (clip, channel): the blocked sums, the norm, the local score in tiles of 256 frames
 *   k_clip_beat_dp     a workgroup a (clip, channel): the programme in steps of h frames on a ring of 2 P + h binary64 values
 *   k_clip_beat_pick   a workgroup a (clip, channel): local maxima, the median by counting, the tail, the walk, the trim, the rows
 * A (clip, channel) has work_stride doubles of scratch at work + ((first + i) channels + ch) work_stride doubles
 * (csrc/beat_core.h beat_work): a header of 8 (the tempo call's four floats in the first two, the norm in the third), cum[F],
 * the local maxima's values [F], then as 32-bit words ls[F], back[F] and the walk's beats [F].
 * The tables are one block of binary64 values: for every P = p_min .. p_max in turn g[0 .. P], then tx[0 .. 2 P] (the entries
 * below h are not read), 3 P + 2 values (csrc/beat_core.h beat_table_at; pdmp3_amd_beat_tables fills one P's). */
typedef struct pdmp3_beat_desc {
  uint64_t env;                             /* device address of channel 0's o[0]; channels env_stride floats apart             */
  uint64_t stats;                           /* ... of the clip's [channels][8] floats, or 0                                       */
  uint64_t dst;                             /* ... of channel 0's output                                                          */
  uint64_t dst_chan_stride;                 /* floats between the channels of the destination                                     */
  uint32_t n;                               /* the frames that enter: the centred calls' valid count                              */
  uint32_t reserved;
} pdmp3_beat_desc;                          /* 40 bytes */
typedef struct pdmp3_beat_params {
  double tightness;
  float bpm;                                /* the caller's, where period > 0                                            */
  int32_t period;                           /* P, or 0: the tempo call's tau* in the scratch's header                    */
  int32_t p_min, p_max;                     /* the periods the tables hold (period > 0: both are it)                     */
  int32_t n_frames, channels;               /* F                                                                         */
  int32_t trim, out_mode;                   /* 0 score, 1 dp, 2 beats                                                    */
  uint32_t env_stride;                      /* floats between the channels of the envelope                               */
  uint32_t work_stride;                     /* doubles of a (clip, channel)'s scratch                                    */
  uint32_t score_lds_bytes, dp_lds_bytes;   /* <= PDMP3_MEL_LDS_SOFT                                                     */
} pdmp3_beat_params;
/* Uploads the descriptors and the tables -- host memory -- and runs the three kernels (mode 0: the first, mode 1: two) on the
 * slot's HIP stream.  work: device memory of n_clips channels work_stride doubles.  The geometry must be csrc/beat_core.h's
 * (pdmp3_amd_beat_plan's).  Blocks until the rows are written. */
int pdmp3_hip_clip_beat(pdmp3_hip_stream* hs, int slot, const pdmp3_beat_desc* descs, int n_clips, const double* tables, double* work,
                        const pdmp3_beat_params* params);

/* test hook: the gc records the device built for the slot's last submit_bits (after pdmp3_hip_stream_wait) */
int pdmp3_hip_stream_fetch_records(pdmp3_hip_stream* hs, int slot, int n_frames, int16_t* spectra, pdmp3_gc_side* side);
/* block until the slot's PCM is in its pinned buffer (no-op if nothing is in flight) */
int pdmp3_hip_stream_wait(pdmp3_hip_stream* hs, int slot);
/* 1: the wait above would return at once (nothing in flight on the slot, or the GPU is through with it), 0: not yet,
 * < 0: bad argument.  Never blocks. */
int pdmp3_hip_stream_done(pdmp3_hip_stream* hs, int slot);

/* Host-side twin of the generator (fills host buffers); used to build
 * identical inputs for the CPU baseline without a device round trip. */
int pdmp3_host_generate_frames(uint64_t seed, int64_t first_frame, int n_frames,
                               int16_t* spectra, pdmp3_gc_side* side);

#ifdef __cplusplus
}
#endif
#endif /* PDMP3_HIP_H */
