// engine.hip -- the gfx950 kernels, and the part of the C-ABI of include/pdmp3_hip.h that launches them: the engine
// context, launch_decode (which kernel, which grid) behind the bare decode entry points, the device Huffman stage's
// launches (unpack_window_head / _carry), generate, the debug entries.  The pdmp3_hip_stream object is stream.hip;
// what the two share is engine_internal.h.
//
// Launch geometry: one 64-lane workgroup (= one wavefront) per chunk of
// `chunk_frames` frames; a launch of N frames makes ceil(N/chunk) workgroups,
// so at throughput sizes (>= 10^5 frames) the grid is >> 256 CUs x 8 XCDs and
// consecutive workgroups (which the dispatcher round-robins over the XCDs)
// stream disjoint, contiguous spans of the spectra / PCM buffers.  There is no
// inter-workgroup communication: chunk boundaries are re-derived from a
// 3-granule halo (decode_core.h).
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "decode_core.h"
#include "engine_internal.h"
#include "gen_core.h"
#include "host_tables.h"
#include "unpack_core.h"
#include <new>

using namespace pdmp3;

#ifndef PDMP3_WAVES_PER_EU
#define PDMP3_WAVES_PER_EU 2
#endif

__constant__ ConstBank c_bank;

// Workgroup b is observed to run on XCD b % 8, each XCD with its own L2.  A chunk's halo is the tail of the chunk
// before it, so neighbouring chunks should share an L2: XCD x gets the x-th contiguous eighth of the chunks
// (bijective for any count).  Purely a placement choice -- nothing is communicated between workgroups.
__device__ __forceinline__ int xcd_contiguous(int b, int n) {
  const int q = n >> 3, r = n & 7, x = b & 7;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (b >> 3);
}

// Independent chunks: one wavefront (= one workgroup) per chunk of frames, a halo in front of each.
// F32: float PCM (the sums of P:2028 unscaled, DecodeArgs::pcm_f32) instead of int16
// (The wave's LDS block is addressed through its wave number although a workgroup is one wave: with the block at a
//  constant address the same source compiles to a kernel that issues 40 more vector loads per granule and takes 1.45 ms
//  instead of 1.05 ms for 131072 frames -- measured on MI355X, ROCm 7.2; profiles/r03_kernel_experiments.txt.)
template <bool DUMP, bool F32 = false, int WPW = 1>
__global__ __launch_bounds__(64 * WPW, PDMP3_WAVES_PER_EU) void k_decode(DecodeArgs a, GlobalTables T, int n_chunks, unsigned* rare_flag, unsigned rare_epoch) {
  __shared__ WaveLds L[WPW];
  const int w = threadIdx.x >> 6;
  const int n_wgs = (n_chunks + WPW - 1) / WPW;
  const int chunk = xcd_contiguous((int)blockIdx.x, n_wgs) * WPW + w;
  if (chunk >= n_chunks) return;
  // Two KERNELS per launch of chunks: this one is compiled without intensity stereo and LSF -- the code every ordinary
  // chunk runs, as tight as it was before those existed (both copies in one kernel cost it a spilled register and 4 % of
  // a 131072-frame launch: profiles/r06_kernel_experiments.txt) -- and leaves the chunks that hold such a frame
  // (decode_core.h chunk_is_rare: a look at the chunk's frame bytes) to k_decode_rare behind it, which it tells so.
  if (DUMP) { run_chunk<DUMP, false, F32, true, true>(a, T, (BankPtr)&c_bank, chunk, L[w], L[w].tab); return; }
  // (rare_flag: a word of the engine's, rare_epoch: this launch's number -- k_decode_rare goes home at once unless the word
  //  says that this launch has a chunk for it; never reset.  Kernel parameters, not DecodeArgs: the granule kernels, which
  //  keep every argument in scalar registers, slowed down by 2.5 % with two more of them)
  if (rare_flag && chunk_is_rare(a, chunk)) {
    if ((threadIdx.x & 63) == 0) __hip_atomic_store(rare_flag, rare_epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  run_chunk<DUMP, false, F32, true, false>(a, T, (BankPtr)&c_bank, chunk, L[w], L[w].tab);
}

// ... the second kernel of the launch: nothing to do unless the first one found a chunk with a frame_is_rare() frame
// (the flag is an epoch number: never reset), then those chunks, with the full code (intensity stereo, LSF)
template <bool F32>
__global__ __launch_bounds__(64, PDMP3_WAVES_PER_EU) void k_decode_rare(DecodeArgs a, GlobalTables T, int n_chunks, int always, const unsigned* rare_flag, unsigned rare_epoch) {
  __shared__ WaveLds L[1];
  const int chunk = (int)blockIdx.x;
  if (chunk >= n_chunks) return;
  if (!always) {
    if (__hip_atomic_load(rare_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != rare_epoch) return;
    if (!chunk_is_rare(a, chunk)) return;
  }
  run_chunk<false, false, F32, true, true>(a, T, (BankPtr)&c_bank, chunk, L[0], L[0].tab);
}

// One granule per wave (decode_core.h run_granule): WPW consecutive granules per workgroup, the workgroup's place in the
// chain is its blockIdx.  128 VGPRs and 9.3 KB of LDS per wave + one table block per workgroup: two workgroups = 16 waves
// per CU, four per SIMD.
// W = 16: one workgroup per CU holds the CU's sixteen waves (a launch of 2048 frames is one workgroup on every CU of
// an MI355X); W = 8 for the smaller launches: twice as many CUs share the work, two waves per SIMD -- which is also all
// the occupancy that form is compiled for (a workgroup of 8 waves is one per CU in the launches that take it; asked for
// four waves per SIMD the compiler could not get there and said so: 217 registers, occupancy 2).
//
// A launch of 2048 frames is ONE resident round -- 4096 waves on 4096 wave slots -- so nothing hides what a wave does
// before its first transform instruction, and the kernel keeps every argument in scalar registers for its whole life.
// GranArgs: its parameters are the twelve values the hot path reads (20 scalar registers, not the 42 of DecodeArgs +
// GlobalTables); the DecodeArgs / GlobalTables the rest of decode_core.h wants are rebuilt here, what this kernel never
// has (stage dumps, an LSF launch's granule count, the PCM pointer of the other type, the profile buffer unless PROF) as
// constants that fold, the tables as constant offsets from the one allocation they share (engine_internal.h kTabOff*).
// k_decode_g_prof = the development launch with shader-clock stamps (chunk_frames = -2 with a profile buffer:
// tools/gran_profile.py): the same workgroup code with PROF set, its buffer a second kernel parameter of that kernel alone.
// Static figures of k_decode_g<false, 16> against DecodeArgs + GlobalTables as parameters: kernarg 168 -> 80 bytes, its
// s_load 21 -> 15, instructions 5872 -> 5698, spilled SGPRs 82 -> 72 (profiles/gran_entry_ab.txt).
struct GranArgs {
  const int16_t* spectra;
  const pdmp3_gc_side* side;
  void* pcm;                     // int16 or float by F32
  const float* state_in;
  float* state_out;
  float* chain_state;
  unsigned* chain_flag;
  const char* tables;            // the tables' allocation (engine_internal.h kTabOff*)
  int n_frames;
  unsigned chain_epoch, debug_flags;
  int sf_hint;
};

// (on the host too: launch_decode builds the other kernels' GlobalTables with it)
__host__ __device__ __forceinline__ GlobalTables tables_at(const char* base) {
  const float* frag = reinterpret_cast<const float*>(base + kTabOffFrag);
  return GlobalTables{reinterpret_cast<const float*>(base + kTabOffPow43), reinterpret_cast<const uint16_t*>(base + kTabOffLinetab),
                      reinterpret_cast<const float*>(base + kTabOffWin), frag, frag + kFragShort, frag + kFragMat, frag + kFragTaps,
                      base + kTabOffImage};
}

template <bool F32, int W, bool PROF>
__device__ __forceinline__ void gran_workgroup(const GranArgs& ga, unsigned long long* prof) {
  DecodeArgs a;
  a.spectra = ga.spectra;
  a.side = ga.side;
  a.pcm = F32 ? nullptr : static_cast<int16_t*>(ga.pcm);
  a.pcm_f32 = F32 ? static_cast<float*>(ga.pcm) : nullptr;
  a.state_in = ga.state_in;
  a.state_out = ga.state_out;
  a.stages = nullptr;
  a.n_frames = ga.n_frames;
  a.chunk_frames = 1;
  a.prof = PROF ? prof : nullptr;
  a.chain_state = ga.chain_state;
  a.chain_flag = ga.chain_flag;
  a.chain_epoch = ga.chain_epoch;
  a.debug_flags = ga.debug_flags;
  a.sf_hint = ga.sf_hint;
  a.n_gran = 0;
  const GlobalTables T = tables_at(ga.tables);
  __shared__ WaveData L[W];
  __shared__ TabLds S;
  __shared__ GranMb mb[W];
  __shared__ unsigned tabs_ready;
  __shared__ ScaleTabs G;                // (the band scales' tables: decode_core.h ph_scales_tab)
  static_assert(sizeof(WaveData) * W + sizeof(TabLds) + sizeof(GranMb) * W + sizeof(ScaleTabs) + 16 <= 160 * 1024, "one workgroup of 16 waves per CU");
  const int tid = (int)threadIdx.x;
  const unsigned long long t_entry = PROF ? PD_CLOCK() : 0ull;     // (read before the kernel arguments have arrived: the first phase holds their round trip)
  const int w = tid >> 6;
  const int g = (int)blockIdx.x * W + w;
  const bool valid = g < 2 * a.n_frames;
  // the wave's own input first: its round trip passes under the workgroup's table loads.  Right behind it the wave's byte
  // of the routing gather (decode_core.h GranRoute): everything run_granule_wave decides from is on its way before the
  // barrier, and the wait behind the table loads below -- which the input has to pass anyway -- covers it.  (The table
  // pieces and the lane's B fragments asked for here too, ahead of the barrier, measured slower: DESIGN.md §3 "Entry".)
  LaneRegs pf;
  if (valid) {
    ph_prefetch(tid & 63, pf, a.spectra + (size_t)g * 1152, a.side + (size_t)g * 2);
    pf.route = gran_route_issue(tid & 63, a.side, g, a.n_frames);
  }
  if (tid < W * (int)(sizeof(GranMb) / 4)) reinterpret_cast<unsigned*>(mb)[tid] = 0u;
  if (tid == 0) tabs_ready = 0u;
  __syncthreads();                       // (nothing to wait for in front of it: the waves arrive together)
  // the workgroup's tables; the line tables are for the sampling frequency the caller expects (granules of another
  // one read the global line table).  No barrier behind the loads: each wave counts itself in when its part is
  // stored (GranPos::tabs_ready) and whoever needs the tables waits for the count -- by then it is long there
  tab_load_image(tid, 64 * W, S, T, a.sf_hint);
  if (PD_GRAN_SCALE_TABS) scale_tabs_load(tid, 64 * W, G, T);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  if ((tid & 63) == 0) atomicAdd(&tabs_ready, 1u);
  if (!valid) return;
  if (PROF && (tid & 63) == 0) a.prof[(size_t)g * kProfSlots] = t_entry;
  const GranPos gp{L, mb, w, W, &tabs_ready, 0, 0, 0, &G};
  run_granule_wave<F32, false, PD_GRAN_SCALE_TABS != 0, true>(a, T, (BankPtr)&c_bank, g, L[w], S, gp, pf);
}

template <bool F32, int W>
__global__ __launch_bounds__(64 * W) __attribute__((amdgpu_waves_per_eu(W / 4, W / 4))) void k_decode_g(GranArgs ga) {
  gran_workgroup<F32, W, false>(ga, nullptr);
}
template <int W>                         // (development: int16 PCM only)
__global__ __launch_bounds__(64 * W) __attribute__((amdgpu_waves_per_eu(W / 4, W / 4))) void k_decode_g_prof(GranArgs ga, unsigned long long* prof) {
  gran_workgroup<false, W, true>(ga, prof);
}

// OPT-IN BUILD (make EXTRA=-DPDMP3_WITH_RING_KERNEL): measured 1.66 x slower than the engine's own choice at every size
// (profiles/r04_ring_bench.txt), so the default library does not carry its two 7 k-instruction kernels.
// Persistent form (decode_core.h run_granule_ring): a workgroup of 16 waves goes round a contiguous range of
// `frames_per_wg` frames, one granule per wave and turn; constants and tables once per wave / workgroup, hand-over through
// the LDS mailboxes as a ring, one halo per range.  One workgroup per CU (158 KB of LDS), four waves per SIMD.
#if defined(PDMP3_WITH_RING_KERNEL)
template <bool F32>
__global__ __launch_bounds__(64 * 16) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_decode_p(DecodeArgs a, GlobalTables T, int frames_per_wg) {
  constexpr int W = 16;
  __shared__ WaveData L[W];
  __shared__ TabLds S;
  __shared__ GranMb mb[W];
  __shared__ unsigned tabs_ready;
  const int tid = (int)threadIdx.x;
  const int w = tid >> 6;
  if (tid < W * (int)(sizeof(GranMb) / 4)) reinterpret_cast<unsigned*>(mb)[tid] = 0u;
  if (tid == 0) tabs_ready = 0u;
  __syncthreads();
  tab_load_image(tid, 64 * W, S, T, a.sf_hint);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  if ((tid & 63) == 0) atomicAdd(&tabs_ready, 1u);
  const int f0 = (int)blockIdx.x * frames_per_wg;
  int f1 = f0 + frames_per_wg;
  if (f1 > a.n_frames) f1 = a.n_frames;
  const GranPos gp{L, mb, w, W, &tabs_ready, 1, 2 * f0, 2 * f1};
  run_granule_ring<F32>(a, T, (BankPtr)&c_bank, L[w], S, gp, f0, f1);
}
#endif

// same kernel with shader-clock stamps after every phase (tools/phase_profile.py)
__global__ __launch_bounds__(64, PDMP3_WAVES_PER_EU) void k_decode_prof(DecodeArgs a, GlobalTables T) {
  __shared__ WaveLds L[1];
  const int w = threadIdx.x >> 6;
  run_chunk<false, true, false, true, false>(a, T, (BankPtr)&c_bank, (int)blockIdx.x, L[w], L[w].tab);   // (the copy ordinary chunks run)
}

// LSF launches (launch_decode): record-frame p of the output = the first granules ([0][ch]: 2 x 576 int16 of spectra, 2 x 128
// bytes of side records) of the input's frames 2 p and 2 p + 1; a missing second one (odd n) is zeroed and never decoded.
__global__ __launch_bounds__(256) void k_lsf_pair(const int16_t* in_sp, const pdmp3_gc_side* in_sd, int n_frames, int16_t* out_sp, pdmp3_gc_side* out_sd) {
  const int p = blockIdx.x;
  const uint4 zero = make_uint4(0, 0, 0, 0);
  for (int gr = 0; gr < 2; gr++) {
    const int f = 2 * p + gr;
    const uint4* ssp = reinterpret_cast<const uint4*>(in_sp + (size_t)f * 2304);
    const uint4* ssd = reinterpret_cast<const uint4*>(in_sd + (size_t)f * 4);
    uint4* dsp = reinterpret_cast<uint4*>(out_sp + (size_t)p * 2304 + gr * 1152);
    uint4* dsd = reinterpret_cast<uint4*>(out_sd + (size_t)p * 4 + gr * 2);
    for (int k = threadIdx.x; k < 144 + 16; k += blockDim.x) {
      if (k < 144) dsp[k] = f < n_frames ? ssp[k] : zero;
      else dsd[k - 144] = f < n_frames ? ssd[k - 144] : zero;
    }
  }
}

__global__ __launch_bounds__(64) void k_generate(uint64_t seed, int64_t first, int16_t* spectra, pdmp3_gc_side* side) {
  const int64_t gc = blockIdx.x;           // (frame_local*4 + gr*2 + ch)
  const int64_t f = gc >> 2;
  gen_gc(seed, first + f, (unsigned)((gc >> 1) & 1), (unsigned)(gc & 1), (int)threadIdx.x,
         spectra + gc * 576, side + gc);
}

// ---------------------------------------------------------------------------
// main-data decoding on the device: unpack_kernels.h (the LSF instantiations: engine_lsf.hip)
// ---------------------------------------------------------------------------
#include "unpack_kernels.h"

// reservoir rows from the pool (unpack_core.h row_chunk16): a wave per frame, 16 bytes per lane and trip (a 4-byte word
// per thread was 21 us for 8192 frames, 1.2 TB/s)
constexpr int kRowsWaves = 4;
__global__ __launch_bounds__(64 * kRowsWaves) void k_rows(const pdmp3_row_desc* desc, const uint8_t* pool, uint8_t* rows, int n_frames) {
  const int f = blockIdx.x * kRowsWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (f >= n_frames) return;
  const pdmp3_row_desc* d = desc + f;
  uint4* out = reinterpret_cast<uint4*>(rows + (size_t)f * kRowBytes);
  for (int c = lane; c < kRowBytes / 16; c += 64) {
    uint32_t v[4];
    row_chunk16(d, pool, 16u * (unsigned)c, v);
    out[c] = make_uint4(v[0], v[1], v[2], v[3]);
  }
}

// k_merge_outcome: unpack_kernels.h "The merge"
__global__ __launch_bounds__(kMergeLanes) void k_merge_outcome(const GcRaw* raw, const pdmp3_frame_bits* bits, int n_frames, uint32_t* outc,
                                                                uint32_t* sup, unsigned* counters) {
  __shared__ uint4 raw_s[kMergeRaw16];
  __shared__ uint8_t fr_s[kMergeBlk];
  __shared__ unsigned last_s;
  const int b = blockIdx.x, f0 = b * kMergeBlk, t = threadIdx.x;
  const int nb = n_frames - f0 < kMergeBlk ? n_frames - f0 : kMergeBlk;
  const uint4* src = reinterpret_cast<const uint4*>(raw + (size_t)f0 * 4);
  for (int i = t; i < nb * 20; i += kMergeLanes) raw_s[i] = src[i];
  if (t < nb) fr_s[t] = bits[f0 + t].frame;
  __syncthreads();
  unsigned o = 0;
  if (t < kMergeSlots) o = merge_block_outcome(t, reinterpret_cast<const GcRaw*>(raw_s), fr_s, nb, PD_UNIFORM(merge_wave_kind(t & ~63)));
  const int sb = b / kMergeSuper, b0 = sb * kMergeSuper;
  const int n_in = (int)gridDim.x - b0 < kMergeSuper ? (int)gridDim.x - b0 : kMergeSuper;
  if (n_in == 1) {                                         // (a super-block of one block: its outcome is the block's)
    outc[(size_t)b * kMergeLanes + t] = o;
    sup[(size_t)sb * kMergeLanes + t] = o;
    return;
  }
  __hip_atomic_store(outc + (size_t)b * kMergeLanes + t, o, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  PD_VMEM_DRAIN();
  __syncthreads();
  if (t == 0) last_s = atomicInc(counters + sb, (unsigned)n_in - 1u) == (unsigned)n_in - 1u;
  __syncthreads();
  if (!last_s) return;
  const int tw = t < kMergeSlots ? merge_twin(t) : -1;
  unsigned oj[kMergeSuper], o0j[kMergeSuper];
  PD_UNROLL for (int j = 0; j < kMergeSuper; j++) {
    const int jj = j < n_in ? j : n_in - 1;
    oj[j] = PD_LOAD_DEVICE(outc + (size_t)(b0 + jj) * kMergeLanes + t);
    o0j[j] = tw >= 0 ? PD_LOAD_DEVICE(outc + (size_t)(b0 + jj) * kMergeLanes + tw) : 0u;
  }
  unsigned acc = 0, acc0 = 0;
  PD_UNROLL for (int j = 0; j < kMergeSuper; j++)
    if (j < n_in) merge_compose_step(oj[j], o0j[j], acc, acc0);
  sup[(size_t)sb * kMergeLanes + t] = acc;
}


// what a launch gets of a ChainBuf (engine_internal.h; a copy made under the lock: another thread's launch may replace the
// buffers right after)
struct ChainUse { float* state; unsigned* flag; unsigned epoch; };

static thread_local char g_err[256] = "";

int fail(int code, const char* what, hipError_t e) {
  snprintf(g_err, sizeof g_err, "%s: %s", what, e == hipSuccess ? "" : hipGetErrorString(e));
  return code;
}

extern "C" const char* pdmp3_hip_last_error(void) { return g_err; }
// (for the library's other translation unit, node.hip: the calling thread's error text)
extern "C" void pdmp3_hip_set_error_(const char* text) { snprintf(g_err, sizeof g_err, "%s", text ? text : ""); }

extern "C" size_t pdmp3_hip_state_bytes(void) { return (size_t)kStateFloats * sizeof(float); }
extern "C" int pdmp3_hip_pci_bus_id(const pdmp3_hip_ctx* c, char* buf, int len) {
  if (!c || !buf || len < 16) return PDMP3_HIP_EINVAL;
  if (hipDeviceGetPCIBusId(buf, len, c->device) != hipSuccess) { buf[0] = 0; return PDMP3_HIP_EDEVICE; }
  return PDMP3_HIP_OK;
}

extern "C" int pdmp3_hip_last_launch_kind(const pdmp3_hip_ctx* c) { return c ? c->last_kind.load(std::memory_order_relaxed) : PDMP3_HIP_LAUNCH_NONE; }

static void chain_free(ChainBuf* b) {                      // (hipFree waits for whatever still uses the memory)
  (void)hipFree(b->state); (void)hipFree(b->flag); (void)hipFree(b->state_tmp); (void)hipFree(b->pair_sp); (void)hipFree(b->pair_sd);
  *b = ChainBuf{};
}

extern "C" void pdmp3_hip_destroy(pdmp3_hip_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)hipFree(c->d_tables);
  (void)hipFree(c->d_rare_flags);
  (void)hipFree(c->d_unpack);
  (void)hipFree(c->d_uprof);
  for (ChainBuf& b : c->chain) chain_free(&b);
  delete c;
}

extern "C" int pdmp3_hip_create(int device, pdmp3_hip_ctx** out) {
  if (!out) return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_create: out is NULL", hipSuccess);
  *out = nullptr;
  HIP_TRY(hipSetDevice(device), "hipSetDevice");
  HostTables H;
  build_host_tables(H);
  if (!H.ldexp_forms_exact)
    return fail(PDMP3_HIP_EDEVICE, "this host's libm pow() disagrees with the device's ldexp forms of 2^(k/4), 2^(-n/2)", hipSuccess);
  pdmp3_hip_ctx* c = new (std::nothrow) pdmp3_hip_ctx();      // (value-initialised: every pointer null)
  if (!c) return fail(PDMP3_HIP_ENOMEM, "new", hipSuccess);
  c->device = device;
  {
    const char* e = getenv("PDMP3_HIP_CHAIN");
    c->chain_mode = (e && *e == '0') ? 0 : 1;
  }
  {
    hipDeviceProp_t prop;
    const int cus = (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 256;
    c->wave_slots = cus * 4 * PDMP3_WAVES_PER_EU;
    c->wave_slots_gran = cus * 4 * 4;
    const char* dm = getenv("PDMP3_HIP_DIRECT_MAX");
    c->direct_max_frames = dm ? atoi(dm) : 32;
    { const char* gw = getenv("PDMP3_HIP_GRAN_W"); c->gran_w8 = gw && atoi(gw) == 8; }
    const char* h = getenv("PDMP3_HIP_SF_HINT");
    c->sf_hint = (h && *h >= '0' && *h <= '2') ? *h - '0' : 0;
    const char* d = getenv("PDMP3_HIP_DEBUG_FAR_TIMEOUT");
    c->debug_flags = (d && *d == '1') ? PD_DEBUG_FAR_TIMEOUT : 0u;
    const char* e = getenv("PDMP3_HIP_GRAN_MAX");
    c->cus = cus;
    { const char* rm = getenv("PDMP3_HIP_RING_MIN"); c->ring_min_frames = rm ? atoi(rm) : 0; }
    c->gran_max_frames = e && atoi(e) > 0 ? atoi(e) : c->wave_slots_gran * 3;     // (measured on MI355X: faster than chunks with halos up to about 14000 frames)
  }
  // every failure from here on releases what was allocated so far (pdmp3_hip_destroy takes a partly built context)
  UnpackTables* U = new UnpackTables;
  const char* what = nullptr;
  hipError_t e = hipSuccess;
#define CREATE_STEP(call, text) if ((e = (call)) != hipSuccess) { what = text; break; }
  do {
    if (!build_unpack_tables(*U)) { what = "Huffman lookup tables exceed kHuffLutMax"; break; }
    CREATE_STEP(hipMemcpyToSymbol(HIP_SYMBOL(c_bank), &H.cb, sizeof(ConstBank)), "upload const bank")
    // the tables GlobalTables points into: one allocation, each at its constant offset (engine_internal.h)
    if (H.pow43.size() * sizeof(float) != kTabPow43Bytes || H.linetab.size() * sizeof(uint16_t) != kTabLinetabBytes ||
        H.win.size() * sizeof(float) != kTabWinBytes || H.frag_long.size() != (size_t)kFragShort || H.frag_short.size() != (size_t)(kFragMat - kFragShort) ||
        H.frag_mat.size() != (size_t)(kFragTaps - kFragMat) || H.taps.size() != (size_t)(kFragFloats - kFragTaps) ||
        H.tab_image.size() * sizeof(TabLds) < kTabImageBytes || H.tab_image.size() != (size_t)kNumSfreq + kScaleTabImages) { what = "the host tables do not have the sizes of the device layout"; break; }
    CREATE_STEP(hipMalloc((void**)&c->d_tables, kTabBytes), "hipMalloc tables")
    CREATE_STEP(hipMemset(c->d_tables, 0, kTabBytes), "hipMemset tables")
    CREATE_STEP(hipMalloc((void**)&c->d_unpack, sizeof(UnpackTables)), "hipMalloc unpack tables")
    { const char* up = getenv("PDMP3_HIP_UNPACK_PROF");
      if (up && *up == '1') CREATE_STEP(hipMalloc((void**)&c->d_uprof, 2048 * 8 * sizeof(unsigned long long)), "hipMalloc unpack prof") }
    CREATE_STEP(hipMemcpy(c->d_tables + kTabOffPow43, H.pow43.data(), kTabPow43Bytes, hipMemcpyHostToDevice), "upload pow43")
    CREATE_STEP(hipMemcpy(c->d_tables + kTabOffLinetab, H.linetab.data(), kTabLinetabBytes, hipMemcpyHostToDevice), "upload linetab")
    CREATE_STEP(hipMemcpy(c->d_tables + kTabOffWin, H.win.data(), kTabWinBytes, hipMemcpyHostToDevice), "upload win")
    CREATE_STEP(hipMemcpy(c->d_tables + kTabOffFrag, H.frag_long.data(), H.frag_long.size() * sizeof(float), hipMemcpyHostToDevice), "upload frag_long")
    CREATE_STEP(hipMemcpy(c->d_tables + kTabOffFrag + kFragShort * sizeof(float), H.frag_short.data(), H.frag_short.size() * sizeof(float), hipMemcpyHostToDevice), "upload frag_short")
    CREATE_STEP(hipMemcpy(c->d_tables + kTabOffFrag + kFragMat * sizeof(float), H.frag_mat.data(), H.frag_mat.size() * sizeof(float), hipMemcpyHostToDevice), "upload frag_mat")
    CREATE_STEP(hipMemcpy(c->d_tables + kTabOffFrag + kFragTaps * sizeof(float), H.taps.data(), H.taps.size() * sizeof(float), hipMemcpyHostToDevice), "upload taps")
    CREATE_STEP(hipMemcpy(c->d_tables + kTabOffImage, H.tab_image.data(), kTabImageBytes, hipMemcpyHostToDevice), "upload table images")
    CREATE_STEP(hipMalloc((void**)&c->d_rare_flags, kRareSlots * sizeof(unsigned)), "hipMalloc rare flags")
    CREATE_STEP(hipMemset(c->d_rare_flags, 0, kRareSlots * sizeof(unsigned)), "hipMemset rare flags")
    c->rare_epoch.store(1);
    CREATE_STEP(hipMemcpy(c->d_unpack, U, sizeof(UnpackTables), hipMemcpyHostToDevice), "upload unpack tables")
    c->unpack_n16 = (int)((offsetof(UnpackTables, lut) + (size_t)U->n_lut * 4 + 15) / 16);
    CREATE_STEP(hipDeviceSynchronize(), "sync after uploads")
  } while (0);
#undef CREATE_STEP
  delete U;
  if (what) {
    pdmp3_hip_destroy(c);
    return fail(PDMP3_HIP_EDEVICE, what, e);
  }
  *out = c;
  return PDMP3_HIP_OK;
}

// Frames per chunk (= per wave).  The kernel holds 2 waves per SIMD, so a launch runs in rounds of `slots` waves
// (2048 on MI355X: 256 CUs x 4 SIMDs x 2); a partly filled last round costs as much as a full one (measured: 131072
// frames at 48 frames per chunk = 1.33 rounds take 20 % longer than at 32 or 64).  So: the fewest rounds that keep a
// chunk at <= 32 frames (halo overhead 2-3 granules per chunk), and the chunk size that spreads the frames evenly
// over them.  Up to one round of frames: one frame per chunk (measured fastest for the 2048-frame batch).
static int auto_chunk(int n_frames, int slots) {
  if (slots < 64) slots = 2048;
  if (n_frames <= slots) return 1;
  const long long per_round_max = (long long)slots * 32;
  const long long rounds = (n_frames + per_round_max - 1) / per_round_max;
  const long long L = (n_frames + slots * rounds - 1) / (slots * rounds);
  return (int)(L < 1 ? 1 : L);
}

// The scratch of a chained launch of n_frames frames on stream s; false: none to be had, the chunks stay independent.
// NO hipMallocAsync in here (until round 6 the scratch below, a bare call's state block and an LSF launch's regrouped records
// were stream-ordered allocations).  On ROCm 7.0.2 / MI355X memory fresh from the stream-ordered allocator can lose the writes of
// the first kernels that touch it, in a process's first moments: tools/ubench/malloc_async_probe.cpp -- allocate, one trivial
// kernel writes, the next reads -- finds up to 2304 of 2560 16-byte words unwritten in 7 of 300 fresh processes (hipMalloc: 0 of
// 300; a stream synchronise between allocation and use: 2 of 300).  It showed as an LSF stream's second batch through the
// streaming API decoding single channels of single frames from zero spectra, in 3-30 % of fresh processes depending on the box
// (tests/fuzz_gpu.py -> tests/test_gpu_lsf.py's CLI test).  Everything is hipMalloc'ed once now and kept: a free or a regrow
// synchronises, which happens when a stream's launches grow, not per launch.
static ChainBuf* chain_entry(pdmp3_hip_ctx* c, const void* key) {   // (c->chain_mu held)
  ChainBuf* b = nullptr;
  for (ChainBuf& x : c->chain) if (x.used && x.key == key) { b = &x; break; }
  if (!b) for (ChainBuf& x : c->chain) if (!x.used) { b = &x; *b = ChainBuf{}; b->used = true; b->key = key; break; }
  if (!b) {
    // every slot is taken: the least recently used one goes (a HIP stream that bare calls once ran on may be long gone,
    // and its scratch -- 17 KB per frame -- would otherwise stay until the engine is destroyed)
    ChainBuf* lru = &c->chain[0];
    for (ChainBuf& x : c->chain) if (x.last_use < lru->last_use) lru = &x;
    chain_free(lru);
    lru->used = true; lru->key = key;
    b = lru;
  }
  b->last_use = ++c->chain_clock;
  return b;
}
// a bare call's state block / regrouped LSF records on stream `key` (see ChainBuf); false: no memory
static bool bare_state_tmp(pdmp3_hip_ctx* c, const void* key, float** out) {
  std::lock_guard<std::mutex> lock(c->chain_mu);
  ChainBuf* b = chain_entry(c, key);
  if (!b->state_tmp && hipMalloc((void**)&b->state_tmp, pdmp3_hip_state_bytes()) != hipSuccess) { (void)hipGetLastError(); b->state_tmp = nullptr; return false; }
  *out = b->state_tmp;
  return true;
}
static bool bare_pairs(pdmp3_hip_ctx* c, const void* key, int np, int16_t** sp, pdmp3_gc_side** sd) {
  std::lock_guard<std::mutex> lock(c->chain_mu);
  ChainBuf* b = chain_entry(c, key);
  if (b->pair_cap < np) {
    (void)hipFree(b->pair_sp); (void)hipFree(b->pair_sd);          // (synchronises: earlier launches are done with them)
    b->pair_sp = nullptr; b->pair_sd = nullptr; b->pair_cap = 0;
    const int cap = np < 64 ? 64 : np;
    if (hipMalloc((void**)&b->pair_sp, (size_t)cap * PDMP3_FRAME_SPECTRA_BYTES) != hipSuccess ||
        hipMalloc((void**)&b->pair_sd, (size_t)cap * PDMP3_FRAME_SIDE_BYTES) != hipSuccess) {
      (void)hipGetLastError();
      (void)hipFree(b->pair_sp); b->pair_sp = nullptr; b->pair_sd = nullptr;
      return false;
    }
    b->pair_cap = cap;
  }
  *sp = b->pair_sp; *sd = b->pair_sd;
  return true;
}
static bool chain_get(pdmp3_hip_ctx* c, const void* key, hipStream_t s, int n_frames, ChainUse* use) {
  std::lock_guard<std::mutex> lock(c->chain_mu);
  ChainBuf* b = chain_entry(c, key);
  constexpr size_t kFloatsPerFrame = (size_t)2 * kGranFloats;
  if (b->cap < n_frames) {
    (void)hipFree(b->state); (void)hipFree(b->flag);       // (synchronises: earlier launches are done with the old ones)
    b->state = nullptr; b->flag = nullptr; b->cap = 0;
    const int cap = n_frames < 256 ? 256 : n_frames;
    const size_t flag_bytes = (size_t)cap * 4 * sizeof(unsigned);
    if (hipMalloc((void**)&b->state, (size_t)cap * kFloatsPerFrame * sizeof(float)) != hipSuccess ||
        hipMalloc((void**)&b->flag, flag_bytes) != hipSuccess ||
        hipMemsetAsync(b->flag, 0, flag_bytes, s) != hipSuccess) {
      (void)hipGetLastError();
      (void)hipFree(b->state); (void)hipFree(b->flag);
      b->state = nullptr; b->flag = nullptr;
      return false;
    }
    b->cap = cap;
    b->epoch = 0;
  }
  if (b->epoch == 0xffffffffu) {                           // (never in practice: flags start over)
    if (hipMemsetAsync(b->flag, 0, (size_t)b->cap * 4 * sizeof(unsigned), s) != hipSuccess) return false;
    b->epoch = 0;
  }
  b->epoch++;
  use->state = b->state;
  use->flag = b->flag;
  use->epoch = b->epoch;
  return true;
}

void chain_release(pdmp3_hip_ctx* c, const void* key) {     // (its launches are complete)
  std::lock_guard<std::mutex> lock(c->chain_mu);
  for (ChainBuf& x : c->chain)
    if (x.used && x.key == key) chain_free(&x);
}

// What launch_decode chose; the functions below only launch it.
struct DecodePlan {
  int kind;            // PDMP3_HIP_LAUNCH_*: the kernel family (the granule kernel's: its waves per workgroup, 8 or 16)
  int n_wgs;
  int frames_per_wg;   // the persistent kernel's range
};

// the hipLaunchKernelGGL ladders over F32 (x W), one per kernel family
#if defined(PDMP3_WITH_RING_KERNEL)
static void launch_ring(const DecodeArgs& a, const GlobalTables& T, const DecodePlan& p, bool f32, hipStream_t s) {
  if (f32) hipLaunchKernelGGL((k_decode_p<true>), dim3(p.n_wgs), dim3(64 * 16), 0, s, a, T, p.frames_per_wg);
  else hipLaunchKernelGGL((k_decode_p<false>), dim3(p.n_wgs), dim3(64 * 16), 0, s, a, T, p.frames_per_wg);
}
#endif
static void launch_granules(pdmp3_hip_ctx* c, const DecodeArgs& a, const DecodePlan& p, bool f32, hipStream_t s) {
  const int W = p.kind;
  const GranArgs ga{a.spectra, a.side, f32 ? (void*)a.pcm_f32 : (void*)a.pcm, a.state_in, a.state_out, a.chain_state, a.chain_flag, c->d_tables,
                    a.n_frames, a.chain_epoch, a.debug_flags, a.sf_hint};
  if (a.prof) {                                  // (development: stamps; launch_decode lets no float PCM come here)
    if (W == 8) hipLaunchKernelGGL((k_decode_g_prof<8>), dim3(p.n_wgs), dim3(64 * W), 0, s, ga, a.prof);
    else hipLaunchKernelGGL((k_decode_g_prof<16>), dim3(p.n_wgs), dim3(64 * W), 0, s, ga, a.prof);
  } else if (W == 8) {
    if (f32) hipLaunchKernelGGL((k_decode_g<true, 8>), dim3(p.n_wgs), dim3(64 * W), 0, s, ga);
    else hipLaunchKernelGGL((k_decode_g<false, 8>), dim3(p.n_wgs), dim3(64 * W), 0, s, ga);
  } else {
    if (f32) hipLaunchKernelGGL((k_decode_g<true, 16>), dim3(p.n_wgs), dim3(64 * W), 0, s, ga);
    else hipLaunchKernelGGL((k_decode_g<false, 16>), dim3(p.n_wgs), dim3(64 * W), 0, s, ga);
  }
}
// chunks with halos: the profiling / dumping forms, every chunk to k_decode_rare (LSF), or k_decode with k_decode_rare
// behind it for the chunks it leaves out (told through this launch's flag word)
static void launch_chunks(pdmp3_hip_ctx* c, const DecodeArgs& a, const GlobalTables& T, const DecodePlan& p, bool f32, bool lsf, hipStream_t s) {
  const int nchunks = p.n_wgs;
  if (a.prof) hipLaunchKernelGGL(k_decode_prof, dim3(nchunks), dim3(64), 0, s, a, T);
  else if (a.stages) hipLaunchKernelGGL(k_decode<true>, dim3(nchunks), dim3(64), 0, s, a, T, nchunks, (unsigned*)nullptr, 0u);
  else if (lsf) {                                // every chunk of an LSF launch is k_decode_rare's
    if (f32) hipLaunchKernelGGL(k_decode_rare<true>, dim3(nchunks), dim3(64), 0, s, a, T, nchunks, 1, (const unsigned*)nullptr, 0u);
    else hipLaunchKernelGGL(k_decode_rare<false>, dim3(nchunks), dim3(64), 0, s, a, T, nchunks, 1, (const unsigned*)nullptr, 0u);
  } else {
    const unsigned ep = c->rare_epoch.fetch_add(1);
    unsigned* flag = c->d_rare_flags + (ep % kRareSlots);
    if (f32) {
      hipLaunchKernelGGL((k_decode<false, true>), dim3(nchunks), dim3(64), 0, s, a, T, nchunks, flag, ep);
      hipLaunchKernelGGL(k_decode_rare<true>, dim3(nchunks), dim3(64), 0, s, a, T, nchunks, 0, (const unsigned*)flag, ep);
    } else {
      // (development: PDMP3_HIP_DEBUG_LDS_PAD = bytes of dynamic LDS added to every workgroup of the chunk kernel, which
      //  lowers the number of waves a CU holds -- 24576: one wave per SIMD instead of two; tools/occupancy_scaling.py)
      static const int lds_pad = [] { const char* e = getenv("PDMP3_HIP_DEBUG_LDS_PAD"); return e ? atoi(e) : 0; }();
      hipLaunchKernelGGL(k_decode<false>, dim3(nchunks), dim3(64), (size_t)lds_pad, s, a, T, nchunks, flag, ep);
      hipLaunchKernelGGL(k_decode_rare<false>, dim3(nchunks), dim3(64), 0, s, a, T, nchunks, 0, (const unsigned*)flag, ep);
    }
  }
}

// One decode launch (engine_internal.h DecodeLaunch).
// state_tmp: where the kernel leaves the new state before it is copied over the state (chunk 0 and the channel-1
// pre-halo read the OLD state while the last chunk writes the new one).  Streams own one; a bare
// pdmp3_hip_decode_frames call takes the one kept for its HIP stream (bare_state_tmp), so that calls on different HIP streams never share it.
int launch_decode(pdmp3_hip_ctx* c, const DecodeLaunch& q) {
  if (!c || q.n_frames < 0) return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_decode_frames: bad argument", hipSuccess);
  if (q.n_frames == 0) return PDMP3_HIP_OK;
  if (!q.spectra || !q.side || !q.pcm)
    return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_decode_frames: NULL buffer", hipSuccess);
  if (((uintptr_t)q.spectra | (uintptr_t)q.side | (uintptr_t)q.pcm) & 15)
    return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_decode_frames: buffers must be 16-byte aligned", hipSuccess);
  hipStream_t s = q.stream;
  HIP_TRY(hipSetDevice(c->device), "hipSetDevice");     // (a bare call may come from a thread whose current device is another one)
  const void* chain_key = q.owner ? q.owner : (const void*)s;   // (a stream object, or the bare call's HIP stream)
  // LSF (pdmp3_gc_side.lsf != 0): a frame is ONE granule.  The kernels keep their two-granule frames: the
  // launch's n frames are regrouped on the device into ceil(n / 2) record-frames whose granules are consecutive FRAMES
  // (k_lsf_pair: [0][ch] of frame 2 p and of frame 2 p + 1), decoded by the chunk kernel -- an odd last frame is a
  // record-frame of one granule (DecodeArgs::n_gran) -- and the PCM comes out in stream order, 576 sample-frames a frame.
  const int16_t* d_spectra = q.spectra;
  const pdmp3_gc_side* d_side = q.side;
  int n_frames = q.n_frames, chunk_frames = q.chunk_frames, n_gran = 0;
  if (q.lsf) {
    if (q.stages || q.prof) return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_decode_lsf_frames: no stage dumps / profiles of LSF launches", hipSuccess);
    const int np = (n_frames + 1) / 2;
    // (a stream object brings its own buffers for the pairs, kept from batch to batch: pair_sp / pair_sd; a bare call's are the
    //  ones kept for its HIP stream)
    int16_t* d_pair_sp = q.pair_sp;
    pdmp3_gc_side* d_pair_sd = q.pair_sd;
    if (!d_pair_sp && !bare_pairs(c, chain_key, np, &d_pair_sp, &d_pair_sd)) return fail(PDMP3_HIP_ENOMEM, "hipMalloc LSF pairs", hipSuccess);
    hipLaunchKernelGGL(k_lsf_pair, dim3(np), dim3(256), 0, s, d_spectra, d_side, n_frames, d_pair_sp, d_pair_sd);
    n_gran = n_frames;
    d_spectra = d_pair_sp; d_side = d_pair_sd; n_frames = np;
    if (chunk_frames <= 1) chunk_frames = 0;             // (never the granule kernels: they hand on whole frames)
  }
  const int chunk_frames_arg = q.lsf ? 2 : chunk_frames;   // (0 = the engine's choice; an LSF launch: chunks)
  if (chunk_frames <= 0) chunk_frames = auto_chunk(n_frames, c->wave_slots);
  if (q.stages || chunk_frames > n_frames) chunk_frames = n_frames;
  float* d_state_tmp = q.state_tmp;
  if (q.state && !d_state_tmp && !bare_state_tmp(c, chain_key, &d_state_tmp)) return fail(PDMP3_HIP_ENOMEM, "hipMalloc state", hipSuccess);
  DecodeArgs a;
  a.spectra = d_spectra;
  a.side = d_side;
  a.pcm = q.f32 ? nullptr : (int16_t*)q.pcm;               // (one destination: DecodeLaunch)
  a.pcm_f32 = q.f32 ? (float*)q.pcm : nullptr;
  a.state_in = (const float*)q.state;
  a.state_out = q.state ? d_state_tmp : nullptr;
  a.stages = q.stages;
  a.n_frames = n_frames;
  a.chunk_frames = chunk_frames;
  a.prof = q.prof;
  a.chain_state = nullptr; a.chain_flag = nullptr; a.chain_epoch = 0; a.debug_flags = c->debug_flags; a.sf_hint = c->sf_hint;
  a.n_gran = n_gran;

  // ---- the choice: which kernel family, which grid ----
  bool gran = false, ring = false;
  const bool plain = !q.stages && !q.prof;
  // the persistent granule kernel: launches of at least ring_min_frames frames (and chunk_frames = -3: always)
  const bool ring_prof = q.prof && chunk_frames_arg == -4;          // (development: the persistent kernel with per-turn stamps)
  if ((plain || ring_prof) && c->chain_mode != 0 && n_frames >= 16 &&
      (chunk_frames_arg == PDMP3_HIP_CHUNK_PERSISTENT || ring_prof || (chunk_frames_arg <= 1 && chunk_frames_arg >= 0 && c->ring_min_frames > 0 && n_frames >= c->ring_min_frames)))
    ring = true;
#if !defined(PDMP3_WITH_RING_KERNEL)
  if (ring && (chunk_frames_arg == PDMP3_HIP_CHUNK_PERSISTENT || ring_prof)) {
    return fail(PDMP3_HIP_EINVAL, "this build of libpdmp3_hip.so does not carry the persistent kernel (make -C pdmp3_amd/csrc EXTRA=-DPDMP3_WITH_RING_KERNEL)", hipSuccess);
  }
  ring = false;
#endif
  const bool gran_prof = q.prof && chunk_frames_arg == -2;          // (development: the granule kernel with per-wave stamps)
  if (gran_prof && q.f32) return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_decode_frames: the stamped granule kernel writes int16 PCM only", hipSuccess);
  if (!ring && (plain || gran_prof) && c->chain_mode != 0 && chunk_frames_arg <= 1 && n_frames <= c->gran_max_frames) {
    // one granule per wave (run_granule): tails and matrixing rows are handed from wave to wave, no halo.  Waits for
    // another workgroup are bounded (then: halo), so the launch finishes whatever part of it is resident; up to
    // gran_max_frames all of it is
    ChainUse u;
    if (chain_get(c, chain_key, s, n_frames, &u)) {
      a.chain_state = u.state; a.chain_flag = u.flag; a.chain_epoch = u.epoch;
      a.chunk_frames = 1;
      gran = true;
    }
  }
  DecodePlan p{PDMP3_HIP_LAUNCH_CHUNKS, (n_frames + a.chunk_frames - 1) / a.chunk_frames, 0};
  if (ring) {
    // one workgroup per CU while a range keeps at least 8 frames (= one turn of the 16 waves)
    const int cus = c->cus > 0 ? c->cus : 256;
    int per = (n_frames + cus - 1) / cus;
    if (per < 8) per = 8;
    a.chunk_frames = 1;
    p = DecodePlan{PDMP3_HIP_LAUNCH_PERSISTENT, (n_frames + per - 1) / per, per};
  } else if (gran) {
    // (workgroups of 8 waves while that gives every CU at most one of them)
    const int W = (2 * n_frames <= c->wave_slots_gran / 2 || c->gran_w8) ? 8 : 16;
    p = DecodePlan{W, (2 * n_frames + W - 1) / W, 0};
  }
  c->last_kind = p.kind;

  // ---- the launch ----
  const GlobalTables T = tables_at(c->d_tables);
#if defined(PDMP3_WITH_RING_KERNEL)
  if (ring) launch_ring(a, T, p, q.f32, s);
  else
#endif
  if (gran) launch_granules(c, a, p, q.f32, s);
  else launch_chunks(c, a, T, p, q.f32, q.lsf, s);
  hipError_t e = hipGetLastError();
  const char* what = "launch k_decode";
  if (e == hipSuccess && q.state && !q.leave_state_in_tmp) {
    what = "state copy";
    e = hipMemcpyAsync(q.state, d_state_tmp, pdmp3_hip_state_bytes(), hipMemcpyDeviceToDevice, s);
  }
  if (e != hipSuccess) return fail(PDMP3_HIP_EDEVICE, what, e);
  return PDMP3_HIP_OK;
}

// The hand-over scratch the engine keeps for bare decode calls on `stream` (17 KB per frame of the largest granule-kernel
// launch seen there, until 32 other streams have been used or the engine is destroyed): given back now.  Blocks until the
// launches on that stream that use it are complete.
extern "C" int pdmp3_hip_release_stream_scratch(pdmp3_hip_ctx* ctx, void* stream) {
  if (!ctx) return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_release_stream_scratch: NULL", hipSuccess);
  HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream), "stream sync");
  chain_release(ctx, (const void*)stream);
  return PDMP3_HIP_OK;
}

// the request of a bare call: records in, PCM out, the caller's state block (or none) on the caller's HIP stream
static DecodeLaunch bare_request(const int16_t* d_spectra, const pdmp3_gc_side* d_side, int n_frames, void* d_state, void* d_pcm, void* stream) {
  DecodeLaunch q;
  q.spectra = d_spectra; q.side = d_side; q.n_frames = n_frames;
  q.pcm = d_pcm;
  q.state = d_state;
  q.stream = (hipStream_t)stream;
  return q;
}

extern "C" int pdmp3_hip_decode_frames(pdmp3_hip_ctx* ctx, const int16_t* d_spectra, const pdmp3_gc_side* d_side,
                                       int n_frames, void* d_state, int16_t* d_pcm, int chunk_frames, void* stream) {
  DecodeLaunch q = bare_request(d_spectra, d_side, n_frames, d_state, d_pcm, stream);
  q.chunk_frames = chunk_frames;
  return launch_decode(ctx, q);
}

extern "C" int pdmp3_hip_decode_frames_f32(pdmp3_hip_ctx* ctx, const int16_t* d_spectra, const pdmp3_gc_side* d_side,
                                           int n_frames, void* d_state, float* d_pcm, int chunk_frames, void* stream) {
  if (!d_pcm) return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_decode_frames_f32: d_pcm is NULL", hipSuccess);
  DecodeLaunch q = bare_request(d_spectra, d_side, n_frames, d_state, d_pcm, stream);
  q.f32 = true;
  q.chunk_frames = chunk_frames;
  return launch_decode(ctx, q);
}

// LSF frames (include/pdmp3_hip.h): n_frames one-granule frames of one channel count -> PCM in stream order
extern "C" int pdmp3_hip_decode_lsf_frames(pdmp3_hip_ctx* ctx, const int16_t* d_spectra, const pdmp3_gc_side* d_side,
                                           int n_frames, void* d_state, int16_t* d_pcm, void* stream) {
  DecodeLaunch q = bare_request(d_spectra, d_side, n_frames, d_state, d_pcm, stream);
  q.lsf = true;
  return launch_decode(ctx, q);
}
extern "C" int pdmp3_hip_decode_lsf_frames_f32(pdmp3_hip_ctx* ctx, const int16_t* d_spectra, const pdmp3_gc_side* d_side,
                                               int n_frames, void* d_state, float* d_pcm, void* stream) {
  if (!d_pcm) return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_decode_lsf_frames_f32: d_pcm is NULL", hipSuccess);
  DecodeLaunch q = bare_request(d_spectra, d_side, n_frames, d_state, d_pcm, stream);
  q.lsf = true;
  q.f32 = true;
  return launch_decode(ctx, q);
}

extern "C" int pdmp3_hip_decode_frames_stages(pdmp3_hip_ctx* ctx, const int16_t* d_spectra, const pdmp3_gc_side* d_side,
                                              int n_frames, void* d_state, int16_t* d_pcm, float* d_stages, void* stream) {
  if (!d_stages) return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_decode_frames_stages: d_stages is NULL", hipSuccess);
  DecodeLaunch q = bare_request(d_spectra, d_side, n_frames, d_state, d_pcm, stream);
  q.stages = d_stages;
  return launch_decode(ctx, q);
}

// ---------------------------------------------------------------------------
// The device Huffman stage of one window (engine_internal.h UnpackWindow): stream.hip orders these behind the window's
// uploads and the previous window's state; the kernels, their grids and templates are here (the LSF instantiations:
// engine_lsf.hip).
// ---------------------------------------------------------------------------
// PDMP3_HIP_UNPACK_PROF=1 (development only: serialises): one line per k_unpack launch from the stamps of its workgroups
static int unpack_prof_print(pdmp3_hip_ctx* c, hipStream_t s, int n_frames, int blocks) {
  static std::vector<unsigned long long> hp(2048 * 8);
  HIP_TRY(hipStreamSynchronize(s), "unpack prof sync");
  HIP_TRY(hipMemcpy(hp.data(), c->d_uprof, (size_t)blocks * 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost), "unpack prof D2H");
  double d[5] = {0, 0, 0, 0, 0}, trips = 0, tmax = 0;
  for (int b = 0; b < blocks; b++) {
    for (int k = 0; k < 5; k++) d[k] += (double)(hp[b * 8 + k + 1] - hp[b * 8 + k]);
    trips += (double)hp[b * 8 + 6];
    const double tot = (double)(hp[b * 8 + 5] - hp[b * 8]);
    if (tot > tmax) tmax = tot;
  }
  fprintf(stderr, "k_unpack prof: %d frames %d wgs | ticks/wg: setup %.0f head %.0f loop %.0f drain %.0f tail %.0f | trips %.1f -> %.1f ticks/trip | longest wg %.0f\n",
          n_frames, blocks, d[0] / blocks, d[1] / blocks, d[2] / blocks, d[3] / blocks, d[4] / blocks, trips / blocks,
          trips > 0 ? d[2] / trips : 0.0, tmax);
  return PDMP3_HIP_OK;
}

// rows of outcomes in UnpackWindow::outc: one per block of kMergeBlk frames, then one per super-block
static unsigned merge_blocks(int n_frames) { return (unsigned)((n_frames + kMergeBlk - 1) / kMergeBlk); }

int unpack_window_head(pdmp3_hip_ctx* c, const UnpackWindow& w) {
  const int n_frames = w.n_frames;
  if (w.desc) {
    hipLaunchKernelGGL(k_rows, dim3((unsigned)((n_frames + kRowsWaves - 1) / kRowsWaves)), dim3(64 * kRowsWaves), 0, w.stream, w.desc, w.pool, w.res, n_frames);
    HIP_TRY(hipGetLastError(), "launch k_rows");
  }
  int blocks = (n_frames + kUnpackRows - 1) / kUnpackRows;
  if (blocks > 2048) blocks = 2048;
  if (w.lsf) HIP_TRY(pdmp3_launch_unpack_lsf(dim3(blocks), w.stream, c->d_unpack, w.bits, w.res, n_frames, w.spectra, w.raw,
                                             c->unpack_n16, c->d_uprof), "launch k_unpack (LSF)");
  else {
    hipLaunchKernelGGL(k_unpack<false>, dim3(blocks), dim3(kUnpackThreads), 0, w.stream, c->d_unpack, w.bits, w.res,
                       n_frames, w.spectra, w.raw, c->unpack_n16, c->d_uprof);
    HIP_TRY(hipGetLastError(), "launch k_unpack");
  }
  if (c->d_uprof) { const int rc = unpack_prof_print(c, w.stream, n_frames, blocks); if (rc != PDMP3_HIP_OK) return rc; }
  // what each block of 64 frames does to the values that survive frames needs nothing of the batch before ...
  const unsigned nblk = merge_blocks(n_frames);
  hipLaunchKernelGGL(k_merge_outcome, dim3(nblk), dim3(kMergeLanes), 0, w.stream, w.raw, w.bits, n_frames, w.outc, w.outc + (size_t)nblk * kMergeLanes, w.mcnt);
  HIP_TRY(hipGetLastError(), "launch k_merge_outcome");
  return PDMP3_HIP_OK;
}

// ... everything from here on continues it (scalefactor / count1 carry, synthesis state)
int unpack_window_carry(const UnpackWindow& w) {
  const unsigned nblk = merge_blocks(w.n_frames);
  const uint32_t* d_sup = w.outc + (size_t)nblk * kMergeLanes;
  if (w.lsf) HIP_TRY(pdmp3_launch_merge_apply_lsf(dim3(nblk), w.stream, w.raw, w.bits, w.n_frames, w.outc, d_sup, w.sf_in, w.sf_out, w.side), "launch k_merge_apply (LSF)");
  else {
    hipLaunchKernelGGL(k_merge_apply<false>, dim3(nblk), dim3(kMergeLanes), 0, w.stream, w.raw, w.bits, w.n_frames, w.outc, d_sup, w.sf_in, w.sf_out, w.side);
    HIP_TRY(hipGetLastError(), "launch k_merge_apply");
  }
  return PDMP3_HIP_OK;
}

extern "C" int pdmp3_hip_generate_frames(pdmp3_hip_ctx* ctx, uint64_t seed, int64_t first_frame, int n_frames,
                                         int16_t* d_spectra, pdmp3_gc_side* d_side, void* stream) {
  if (!ctx || !d_spectra || !d_side || n_frames < 0)
    return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_generate_frames: bad argument", hipSuccess);
  if (n_frames == 0) return PDMP3_HIP_OK;
  HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
  hipLaunchKernelGGL(k_generate, dim3((unsigned)n_frames * 4u), dim3(64), 0, (hipStream_t)stream, seed, first_frame,
                     d_spectra, d_side);
  HIP_TRY(hipGetLastError(), "launch k_generate");
  return PDMP3_HIP_OK;
}

extern "C" int pdmp3_host_generate_frames(uint64_t seed, int64_t first_frame, int n_frames, int16_t* spectra,
                                          pdmp3_gc_side* side) {
  if (!spectra || !side || n_frames < 0) return fail(PDMP3_HIP_EINVAL, "pdmp3_host_generate_frames: bad argument", hipSuccess);
  for (int f = 0; f < n_frames; ++f)
    for (int gc = 0; gc < 4; ++gc)
      for (int lane = 0; lane < 64; ++lane)
        gen_gc(seed, first_frame + f, (unsigned)(gc >> 1), (unsigned)(gc & 1), lane,
               spectra + ((size_t)f * 4 + gc) * 576, side + (size_t)f * 4 + gc);
  return PDMP3_HIP_OK;
}

// Test entry (not part of the product boundary): the two merge kernels alone on merge input from the host -- raw: n_frames x 4
// GcRaw (320 bytes per frame, unpack_core.h), bits: the frames' side-info records, state_in / state_out: 256 uint16 each, side:
// n_frames x 4 records out.  tests/test_gpu_bulk.py runs it on random input beside the rule's host form.
extern "C" int pdmp3_hip_debug_merge(pdmp3_hip_ctx* ctx, const void* raw, const pdmp3_frame_bits* bits, int n_frames,
                                     const uint16_t* state_in, uint16_t* state_out, pdmp3_gc_side* side) {
  if (!ctx || !raw || !bits || !state_in || !state_out || !side || n_frames <= 0)
    return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_debug_merge: bad argument", hipSuccess);
  HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
  const size_t n = (size_t)n_frames, nblk = (n + kMergeBlk - 1) / kMergeBlk, nsup = (nblk + kMergeSuper - 1) / kMergeSuper;
  GcRaw* d_raw = nullptr; pdmp3_frame_bits* d_bits = nullptr; uint32_t* d_outc = nullptr; unsigned* d_cnt = nullptr;
  uint16_t* d_st = nullptr; pdmp3_gc_side* d_side = nullptr;
  int rc = PDMP3_HIP_OK;
  do {
#define DM_STEP(call, text) if ((call) != hipSuccess) { rc = fail(PDMP3_HIP_EDEVICE, text, hipGetLastError()); break; }
    DM_STEP(hipMalloc((void**)&d_raw, n * 4 * sizeof(GcRaw)), "hipMalloc raw")
    DM_STEP(hipMalloc((void**)&d_bits, n * sizeof(pdmp3_frame_bits)), "hipMalloc bits")
    DM_STEP(hipMalloc((void**)&d_outc, (nblk + nsup) * kMergeLanes * sizeof(uint32_t)), "hipMalloc outcomes")
    DM_STEP(hipMalloc((void**)&d_cnt, (nsup + 1) * sizeof(unsigned)), "hipMalloc counters")
    DM_STEP(hipMalloc((void**)&d_st, 2 * 256 * sizeof(uint16_t)), "hipMalloc state")
    DM_STEP(hipMalloc((void**)&d_side, n * 4 * sizeof(pdmp3_gc_side)), "hipMalloc side")
    DM_STEP(hipMemset(d_cnt, 0, (nsup + 1) * sizeof(unsigned)), "memset counters")
    DM_STEP(hipMemset(d_side, 0xee, n * 4 * sizeof(pdmp3_gc_side)), "memset side")          // (every byte of the records is the kernel's to write)
    DM_STEP(hipMemcpy(d_raw, raw, n * 4 * sizeof(GcRaw), hipMemcpyHostToDevice), "H2D raw")
    DM_STEP(hipMemcpy(d_bits, bits, n * sizeof(pdmp3_frame_bits), hipMemcpyHostToDevice), "H2D bits")
    DM_STEP(hipMemcpy(d_st, state_in, 256 * sizeof(uint16_t), hipMemcpyHostToDevice), "H2D state")
    hipLaunchKernelGGL(k_merge_outcome, dim3((unsigned)nblk), dim3(kMergeLanes), 0, 0, d_raw, d_bits, n_frames, d_outc, d_outc + nblk * kMergeLanes, d_cnt);
    hipLaunchKernelGGL(k_merge_apply<false>, dim3((unsigned)nblk), dim3(kMergeLanes), 0, 0, d_raw, d_bits, n_frames, d_outc, d_outc + nblk * kMergeLanes,
                       d_st, d_st + 256, d_side);
    DM_STEP(hipGetLastError(), "launch merge kernels")
    DM_STEP(hipDeviceSynchronize(), "sync")
    DM_STEP(hipMemcpy(side, d_side, n * 4 * sizeof(pdmp3_gc_side), hipMemcpyDeviceToHost), "D2H side")
    DM_STEP(hipMemcpy(state_out, d_st + 256, 256 * sizeof(uint16_t), hipMemcpyDeviceToHost), "D2H state")
    unsigned left[64] = {0};                              // (the super-blocks' counters are back at zero: the next launch finds them so)
    DM_STEP(hipMemcpy(left, d_cnt, (nsup < 64 ? nsup : 64) * sizeof(unsigned), hipMemcpyDeviceToHost), "D2H counters")
    for (size_t i = 0; i < (nsup < 64 ? nsup : 64); i++) if (left[i]) rc = fail(PDMP3_HIP_EDEVICE, "pdmp3_hip_debug_merge: a super-block's counter did not wrap", hipSuccess);
#undef DM_STEP
  } while (0);
  (void)hipFree(d_raw); (void)hipFree(d_bits); (void)hipFree(d_outc); (void)hipFree(d_cnt); (void)hipFree(d_st); (void)hipFree(d_side);
  return rc;
}

// Debug/profiling entry (not part of the product boundary): per-chunk shader-clock
// ticks spent in each pipeline phase.  d_prof: uint64 [n_chunks][10].
extern "C" int pdmp3_hip_debug_profile_phases(pdmp3_hip_ctx* ctx, const int16_t* d_spectra, const pdmp3_gc_side* d_side,
                                              int n_frames, int16_t* d_pcm, int chunk_frames,
                                              unsigned long long* d_prof, void* stream) {
  if (!d_prof) return fail(PDMP3_HIP_EINVAL, "pdmp3_hip_debug_profile_phases: d_prof is NULL", hipSuccess);
  DecodeLaunch q = bare_request(d_spectra, d_side, n_frames, nullptr, d_pcm, stream);
  q.chunk_frames = chunk_frames;
  q.prof = d_prof;
  return launch_decode(ctx, q);
}
