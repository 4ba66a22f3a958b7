// unpack_kernels.h -- the device Huffman stage's kernels that come in an MPEG-1 and an LSF form (unpack_core.h on the GPU):
// k_unpack and k_merge_apply (k_rows and k_merge_outcome, which do not care, are in engine.hip).  Included by engine.hip,
// which launches the MPEG-1 forms (unpack_window_head / _carry), and by engine_lsf.hip, which holds the LSF
// instantiations of k_unpack / k_merge_apply in a module of their own: compiled into one module with the MPEG-1 ones they
// changed the MPEG-1 kernels' code (out-of-line helpers that two kernels share lose the constants of their one caller).
#pragma once
#include <hip/hip_runtime.h>

#include "decode_core.h"
#include "unpack_core.h"

namespace pdmp3 {
// ---------------------------------------------------------------------------
// main-data decoding on the device (unpack_core.h)
// ---------------------------------------------------------------------------
constexpr int kUnpackLanes = 64;                        // one wave = 16 frames per pass decodes ...
constexpr int kUnpackThreads = 256;                     // ... four bring the tables and the rows into LDS and zero the output
constexpr int kUnpackRows = kUnpackLanes / 4;
constexpr int kRowBytes = PDMP3_RESERVOIR_BYTES;
// LDS row stride in 32-bit words, chosen ODD: the 64 lanes read their rows at about the same offset at the same
// time, and with the natural stride (516 words) that is 8 of the 32 banks for the whole wave
constexpr int kRowStrideW = kRowBytes / 4 + 1;          // 517
constexpr int kFrameBitsW = sizeof(pdmp3_frame_bits) / 4;   // 20

// LDS: the 34 KB table blob, the 16 reservoir rows the workgroup works on (33 KB) and their side info, brought in with
// coalesced loads, and the 16 KB ring of symbol records: 85 KB, one workgroup per CU.  The kernel is a long dependent
// chain per lane -- where does the next code word start -- and a window of 2048 frames has only 8192 of them (128
// waves on 1024 SIMDs), so what counts is the length of that chain: WAVE 0 of the workgroup walks the 64 bit streams
// (unpack_core.h unpack_step: two table lookups and an add per symbol, pairs and quads in one loop) and leaves a record
// per symbol and lane in the ring; WAVES 1-3 take turns with the ring's rows (row i belongs to wave 1 + i % 3), read
// linbits and signs and store the lines (unpack_value).  Round 2's single loop did all of it in wave 0, a loop per
// symbol kind: 406 trips of ~700 cycles per window, 140 us; this one: <= 288 trips of the walker's half.
// The lines go straight to HBM, into spectra that two of the value waves zero with coalesced stores first.
constexpr int kRingRows = 16;                              // trips the walker may be ahead of the value waves (16, not 32: the ring's 8 KB
                                                           // are what lets TWO workgroups share a CU -- 80.0 KB each --, which is worth more on the
                                                           // windows of 4096 frames the whole-stream decoder now uses: 17.0 -> 18.5 M frames/s)
constexpr int kRingCheck = 8;                              // ... looked at every so many trips
static_assert(kRingRows % kRingCheck == 0 && kRingCheck >= 3, "blocks of trips do not wrap around the ring");
struct UnpackRing {
  SymRec rec[kRingRows][kUnpackLanes];                     // tag (trip / kRingRows) & 3 in bits 30-31 of .x: the row is of THIS turn
  unsigned next[3];                                        // value wave c: the first trip it has not taken yet
  unsigned zeroed;                                         // value waves 2 and 3: my half of the pass's spectra is zero
};
typedef unsigned ring_u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ ring_u32x2 ring_load(const SymRec* p) {
  return *(const volatile __attribute__((address_space(3))) ring_u32x2*)(p);
}
__device__ __forceinline__ void ring_store(SymRec* p, uint32_t x, uint32_t y) {
  ring_u32x2 v;
  v.x = x; v.y = y;
  *(volatile __attribute__((address_space(3))) ring_u32x2*)(p) = v;
}

// LSF: the window's frames are all LSF (pdmp3_hip_stream_set_lsf; unpack_core.h kFramesLsf) -- the lanes of granule 1
// have nothing to do.  The MPEG-1 instantiation is the kernel as it was.
template <bool LSF>
__global__ __launch_bounds__(kUnpackThreads) void k_unpack(const UnpackTables* tabs, const pdmp3_frame_bits* bits,
                                                            const uint8_t* res, int n_frames, int16_t* spectra,
                                                            GcRaw* raw, int tab_n16, unsigned long long* prof) {
  __shared__ UnpackTables U;
  __shared__ uint32_t rows[kUnpackRows * kRowStrideW + 4];
  __shared__ uint32_t fbits[kUnpackRows * kFrameBitsW];
  __shared__ UnpackRing ring;
  // development only (PDMP3_HIP_UNPACK_PROF=1): s_memtime of workgroup's wave 0 at the steps of its first pass
#define PD_UP_STAMP(k) do { if (prof && threadIdx.x == 0) prof[blockIdx.x * 8 + (k)] = __builtin_readcyclecounter(); } while (0)
  PD_UP_STAMP(0);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int fl = lane >> 2, g = lane & 3;                  // the granule-channel of this lane, in every wave
  bool first = true;
  for (int f0 = blockIdx.x * kUnpackRows; f0 < n_frames; f0 += gridDim.x * kUnpackRows) {
    const int nrows = n_frames - f0 < kUnpackRows ? n_frames - f0 : kUnpackRows;
    if (!first) __syncthreads();                           // (previous pass done with the buffers)
    {
      // the pass's rows, 16 bytes per lane and trip, all asked for before the tables (first pass) so that the two
      // round trips to HBM overlap
      constexpr int kRow16 = kRowBytes / 16, kRowTrips = (kUnpackRows * kRow16 + kUnpackThreads - 1) / kUnpackThreads;
      static_assert(kRowBytes % 16 == 0, "rows are copied 16 bytes at a time");
      const uint4* src = reinterpret_cast<const uint4*>(res + (size_t)f0 * kRowBytes);
      uint4 rv[kRowTrips];
      PD_UNROLL for (int k = 0; k < kRowTrips; ++k) {
        const int i = (int)threadIdx.x + k * kUnpackThreads;
        if (i < nrows * kRow16) rv[k] = src[i];
      }
      if (first) {
        const uint4* tsrc = reinterpret_cast<const uint4*>(tabs);
        uint4* dst = reinterpret_cast<uint4*>(&U);
        for (int i = threadIdx.x; i < tab_n16; i += kUnpackThreads) dst[i] = tsrc[i];
      }
      PD_UNROLL for (int k = 0; k < kRowTrips; ++k) {
        const int i = (int)threadIdx.x + k * kUnpackThreads;
        if (i < nrows * kRow16) {
          const int r = i / kRow16, c = i - r * kRow16;
          uint32_t* d = rows + r * kRowStrideW + 4 * c;    // (unpack_core.h PD_ROW_BE: big-endian words as numbers)
          d[0] = __builtin_bswap32(rv[k].x); d[1] = __builtin_bswap32(rv[k].y);
          d[2] = __builtin_bswap32(rv[k].z); d[3] = __builtin_bswap32(rv[k].w);
        }
      }
      const uint32_t* fsrc = reinterpret_cast<const uint32_t*>(bits + f0);
      for (int i = threadIdx.x; i < nrows * kFrameBitsW; i += kUnpackThreads) fbits[i] = fsrc[i];
      for (int i = threadIdx.x; i < kRingRows * kUnpackLanes; i += kUnpackThreads) (&ring.rec[0][0])[i].x = 3u << 30;   // "the turn before trip 0"
      if (threadIdx.x < 3) ring.next[threadIdx.x] = threadIdx.x;
      if (threadIdx.x == 3) ring.zeroed = 0;
    }
    __syncthreads();
    PD_UP_STAMP(1);
    const size_t idx = (size_t)(f0 + fl) * 4 + g;
    const uint8_t* row = reinterpret_cast<const uint8_t*>(rows + fl * kRowStrideW);
    int16_t* is = spectra + idx * 576;
    SymPlan P;
    SymState st;
    bool live = false;
    if (wave == 0) {
      // ---- the walker
      if (fl < nrows) live = unpack_plan<LSF ? kFramesLsf : kFramesMpeg1>(U, *reinterpret_cast<const pdmp3_frame_bits*>(fbits + fl * kFrameBitsW), g, P, st);
      PD_UP_STAMP(2);
      Win2 w;
      w2_open(w, row, live ? st.pos : 0u);
      if (!live) { st.pos = 0; st.line = 0; }
      // the plan in REGISTERS (as a struct it stays in memory and every trip starts with a load of its table base)
      unsigned qt0 = P.tab0, qt1 = P.tab1, qt2 = P.tab2, qq = P.qbase, qe0 = P.e0, qe1 = P.e1, qn = P.nbig, qend = P.end;
      PD_PIN(qt0); PD_PIN(qt1); PD_PIN(qt2); PD_PIN(qq); PD_PIN(qe0); PD_PIN(qe1); PD_PIN(qn); PD_PIN(qend);
      // kRingCheck trips at a time: room in the ring and "is any lane still at it" are looked at once per block (a lone
      // wave issues an instruction every ~6 cycles whatever it is: the loop's own bookkeeping was a third of a trip)
      const unsigned ztab = U.book_base[kZeroBook];
      unsigned trip = 0;
      for (;; trip += kRingCheck) {
        for (;;) {                                         // room for the block's rows?  (rarely not: three waves take them out)
          const unsigned n0 = PD_LDS_FLAG(&ring.next[0]), n1 = PD_LDS_FLAG(&ring.next[1]), n2 = PD_LDS_FLAG(&ring.next[2]);
          const unsigned lo = n0 < n1 ? (n0 < n2 ? n0 : n2) : (n1 < n2 ? n1 : n2);
          if (__builtin_amdgcn_readfirstlane(lo) + kRingRows >= trip + kRingCheck) break;
          PD_SLEEP();
        }
        if (!__any(live && sym_active(qn, qend, st))) break;
        SymRec* blk = &ring.rec[trip % kRingRows][lane];   // (kRingRows is a multiple of kRingCheck: the block does not wrap)
        const uint32_t tag = ((trip / kRingRows) & 3u) << 30;
        PD_UNROLL for (int j = 0; j < kRingCheck; ++j) {
          const SymRec r = unpack_step(U.lut, qt0, qt1, qt2, qq, ztab, qe0, qe1, qn, live && sym_active(qn, qend, st), st, w);
          ring_store(blk + j * kUnpackLanes, r.x | tag, r.y);
        }
      }
      PD_UP_STAMP(3);
      if (prof && threadIdx.x == 0) prof[blockIdx.x * 8 + 6] = trip;
      for (int k = 0; k < 3; ++k)                          // one end row per value wave (the block's room was checked)
        ring_store(&ring.rec[(trip + k) % kRingRows][lane], (kRecNopLine << 16) | (((trip + k) / kRingRows) & 3u) << 30, kRecEnd);
    } else {
      // ---- a value wave: rows wave - 1, wave + 2, ...  The first one writes the records' side fields and scalefactors
      // before it joins in (the ring holds what the walker produces meanwhile; the other two are taking rows out already)
      // and the other two zero the pass's spectra (lines are stored only where the stream has any) -- all of it beside
      // the walker's first trips instead of in front of them
      if (wave == 1) {
        if (fl < nrows)
          unpack_scalefactors<LSF ? kFramesLsf : kFramesMpeg1>(U, row, *reinterpret_cast<const pdmp3_frame_bits*>(fbits + fl * kFrameBitsW), g, raw + idx);
      } else {
        uint4* z = reinterpret_cast<uint4*>(spectra + (size_t)f0 * 4 * 576);
        for (int i = (int)threadIdx.x - 128; i < nrows * 4 * 72; i += 128) z[i] = make_uint4(0, 0, 0, 0);
        PD_VMEM_DRAIN();                                   // the zeroes have arrived before any wave stores a line
        if (lane == 0) atomicAdd(&ring.zeroed, 1u);
      }
      while (PD_UNIFORM(PD_LDS_FLAG(&ring.zeroed)) < 2) PD_SLEEP();
      asm volatile("" ::: "memory");
      for (unsigned trip = (unsigned)wave - 1;; trip += 3) {
        const SymRec* slot = &ring.rec[trip % kRingRows][lane];
        const unsigned tag = (trip / kRingRows) & 3u;
        ring_u32x2 r;
        for (;;) {
          r = ring_load(slot);
          if (__all((r.x >> 30) == tag)) break;
          __builtin_amdgcn_s_sleep(1);
        }
        if (lane == 0) PD_LDS_FLAG(&ring.next[wave - 1]) = trip + 3;
        if (r.y & kRecEnd) break;
        unpack_value(row, SymRec{r.x, r.y}, is);
      }
    }
    __syncthreads();                                       // every line of every record is stored, and wave 1's part of `raw`
    PD_UP_STAMP(4);
    if (wave == 0 && live) unpack_tail(U, U.lut, row, P, st, is, raw + idx);
    PD_UP_STAMP(5);
    first = false;
  }
#undef PD_UP_STAMP
}

// The merge (unpack_core.h "The same merge by BLOCKS"): a workgroup per block of 32 frames, a lane per surviving value.
// k_merge_outcome: the block's 10 KB of merge input into LDS with 16-byte loads, every lane walks the 32 frames for its
// slot, a row of outcomes goes out; the workgroup that is through last among the eight of a super-block (a counter that
// wraps back to zero by itself) composes the eight rows into the super-block's.  What the eight exchange travels as the
// granule kernel's hand-overs do: device-scope relaxed atomic accesses, ordered by the wait for the stores and the counter.
constexpr int kMergeRaw16 = kMergeBlk * 4 * (int)sizeof(GcRaw) / 16;              // 640
constexpr int kMergeBits16 = kMergeBlk * (int)sizeof(pdmp3_frame_bits) / 16;      // 160
constexpr int kMergeSide16 = kMergeBlk * PDMP3_FRAME_SIDE_BYTES / 16;             // 1024
constexpr int kMergeRow16 = kMergeLanes * 4 / 16;                                 // a row of outcomes: 64
constexpr int kMergeStageRows = 40;                                               // rows of outcomes a block looks at in one go (a window of 8192 frames: 38 at most)
constexpr int kMergeRawPer = (kMergeRaw16 + kMergeLanes - 1) / kMergeLanes, kMergeBitsPer = (kMergeBits16 + kMergeLanes - 1) / kMergeLanes;
static_assert(sizeof(GcRaw) % 16 == 0 && sizeof(pdmp3_frame_bits) % 16 == 0 && kMergeSlots <= kMergeLanes, "the merge copies 16 bytes at a time");
// k_merge_apply: block b asks for its frames' inputs, walks the rows of outcomes in front of it -- super-blocks 0 .. b / 8 - 1,
// then the blocks of its own super-block -- from the values the window before left, then its own frames; the records are
// built in LDS -- zeroes, the frame's own side fields (a thread per granule-channel), scalefactors and count1 (a thread per
// slot: byte stores) -- and leave with 16-byte stores: the whole of `side` is written here, once.  The last block leaves
// the values for the next window.  LSF: the window's frames are all LSF (their records: unpack_core.h side_fields, merge_frame_meta).
template <bool LSF>
__global__ __launch_bounds__(kMergeLanes) void k_merge_apply(const GcRaw* raw, const pdmp3_frame_bits* bits, int n_frames, const uint32_t* outc,
                                                              const uint32_t* sup, const uint16_t* state_in, uint16_t* state_out, pdmp3_gc_side* side) {
  __shared__ uint4 raw_s[kMergeRaw16];
  __shared__ uint4 bits_s[kMergeBits16];
  __shared__ uint4 img_s[kMergeSide16];
  __shared__ uint4 stage_s[kMergeStageRows * kMergeRow16];
  __shared__ uint32_t meta_s[kMergeBlk];
  __shared__ uint8_t trash_s[kMergeLanes];
  const int b = blockIdx.x, f0 = b * kMergeBlk, t = threadIdx.x;
  const int nb = n_frames - f0 < kMergeBlk ? n_frames - f0 : kMergeBlk;
  uint4 rv[kMergeRawPer], bv[kMergeBitsPer];
  uint32_t hw = 0;
  {
    if (t < nb) hw = *reinterpret_cast<const uint32_t*>(bits + f0 + t);      // frame | scfsi | iso
    const uint4* src = reinterpret_cast<const uint4*>(raw + (size_t)f0 * 4);
    // (values, not arrays in memory: every element is assigned on every path)
    PD_UNROLL for (int k = 0; k < kMergeRawPer; k++) { const int i = t + k * kMergeLanes; rv[k] = make_uint4(0, 0, 0, 0); if (i < nb * 20) rv[k] = src[i]; }
    const uint4* bsrc = reinterpret_cast<const uint4*>(bits + f0);
    PD_UNROLL for (int k = 0; k < kMergeBitsPer; k++) { const int i = t + k * kMergeLanes; bv[k] = make_uint4(0, 0, 0, 0); if (i < nb * 5) bv[k] = bsrc[i]; }
  }
  const int tw = t < kMergeSlots ? merge_twin(t) : -1;
  const unsigned kind = PD_UNIFORM(merge_wave_kind(t & ~63));
  unsigned val = t < kMergeSlots ? state_in[t] : 0u, val0 = tw >= 0 ? state_in[tw] : 0u;
  const int nsup = b / kMergeSuper, total = nsup + b % kMergeSuper;
  for (int c0 = 0; c0 < total; c0 += kMergeStageRows) {
    const int nc = total - c0 < kMergeStageRows ? total - c0 : kMergeStageRows;
    if (c0) __syncthreads();
    for (int i = t; i < nc * kMergeRow16; i += kMergeLanes) {
      const int r = c0 + i / kMergeRow16;
      const uint32_t* row = r < nsup ? sup + (size_t)r * kMergeLanes : outc + (size_t)(nsup * kMergeSuper + r - nsup) * kMergeLanes;
      stage_s[i] = reinterpret_cast<const uint4*>(row)[i % kMergeRow16];
    }
    __syncthreads();
    if (t < kMergeSlots) {
      if (kind & 1u) merge_carry_rows<true>(reinterpret_cast<const uint32_t*>(stage_s), nc, t, tw, val, val0);
      else merge_carry_rows<false>(reinterpret_cast<const uint32_t*>(stage_s), nc, t, tw, val, val0);
    }
  }
  PD_UNROLL for (int k = 0; k < kMergeRawPer; k++) { const int i = t + k * kMergeLanes; if (i < nb * 20) raw_s[i] = rv[k]; }
  PD_UNROLL for (int k = 0; k < kMergeBitsPer; k++) { const int i = t + k * kMergeLanes; if (i < nb * 5) bits_s[i] = bv[k]; }
  for (int i = t; i < kMergeSide16; i += kMergeLanes) img_s[i] = make_uint4(0, 0, 0, 0);
  if (t < nb) meta_s[t] = merge_frame_meta(hw & 0xffu, hw >> 24, LSF);
  __syncthreads();
  const pdmp3_frame_bits* F = reinterpret_cast<const pdmp3_frame_bits*>(bits_s);
  pdmp3_gc_side* img = reinterpret_cast<pdmp3_gc_side*>(img_s);
  if ((t >> 2) < nb) side_fields<LSF ? kFramesLsf : kFramesMpeg1>(F[t >> 2], t & 3, img + t);
  if (t < kMergeSlots) {
    val = merge_block_apply(t, val, val0, reinterpret_cast<const GcRaw*>(raw_s), meta_s, nb, img, trash_s + t, kind);
    if (f0 + nb == n_frames) state_out[t] = (uint16_t)val;
  }
  __syncthreads();
  uint4* dst = reinterpret_cast<uint4*>(side + (size_t)f0 * 4);
  for (int i = t; i < nb * (PDMP3_FRAME_SIDE_BYTES / 16); i += kMergeLanes) dst[i] = img_s[i];
}

}  // namespace pdmp3
