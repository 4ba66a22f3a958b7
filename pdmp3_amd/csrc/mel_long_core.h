// mel_long_core.h -- what k_clip_mel_long (mel_long.hip) adds to stft_long_core.h / mel_core.h: the
// order in which a workgroup meets the bins (the rows of the filterbank operand), the LDS layout of the powers of one tile of
// k1 with its banks, and the floats of the three LDS regions.  One source for the kernel and for the host build the tests
// compile with g++ (tests/host_emul/mel_long_emul.cpp).
#ifndef PDMP3_MEL_LONG_CORE_H
#define PDMP3_MEL_LONG_CORE_H
#include "stft_long_core.h"

namespace pdmp3 {

constexpr int kMelLongThreads = 512;        // eight waves: one workgroup a CU at these LDS sizes, two waves a SIMD

// ---- the order of the bins ----
// A workgroup runs kt = 0 .. 3 one after the other; stage 2 of one kt gives the 8 N2 bins k = 16 kt + k1l + 64 k2, k1l < 16,
// k2 < N2 / 2 (the Nyquist bin N / 2 is never computed: its weight is exactly 0 in every accepted filterbank).  Within a kt
// bin (k1l, k2) takes slot
//   32 (((k1l & 3) | (k1l >> 3) << 2) (N2 / 32) + (k2 >> 4))  +  16 ((k1l >> 2) & 1)  +  (k2 & 15)
// -- a bijection onto 0 .. 8 N2 - 1 -- and the filterbank GEMM sums a band over the slots ascending, kt ascending: one fixed
// order for every frame.  The operand's row of a bin is 8 N2 kt + slot; the host lays it out so (host/clip_mel_long.c).
MEL_FN int mell_slots(int N2) { return 8 * N2; }
MEL_FN int mell_slot(int k1l, int k2, int N2) {
  return 32 * (((k1l & 3) | ((k1l >> 3) << 2)) * (N2 >> 5) + (k2 >> 4)) + 16 * ((k1l >> 2) & 1) + (k2 & 15);
}
MEL_FN int mell_operand_row(int kt, int k1l, int k2, int N2) { return mell_slots(N2) * kt + mell_slot(k1l, k2, N2); }
MEL_FN int mell_bin(int kt, int k1l, int k2) { return 16 * kt + k1l + 64 * k2; }

// ---- LDS: the span (plain, kept for all four kt), then Z (stft_long_core.h), then the powers of one kt ----
// The powers: 8 N2 + 2 floats a frame of the tile, slot innermost.  8 N2 + 2 = 2 mod 32.
//   stage 2 writes (ds_write_b32, 32 lanes at a time = kq 0 and 1, or kq 2 and 3): lane (j, kq) holds k2 = 16 ct + j,
//     k1l = 4 kq + r of one frame: k1l & 3 = r and k1l >> 3 = kq >> 1 are the same for a group's lanes, (k1l >> 2) & 1 = kq & 1
//     tells its two halves apart: the group writes 32 consecutive floats, 32 banks once.  (With the slot k1l N2 / 2 + k2 of
//     section 14's staging tile the two kq would lie 2 N2 floats apart, the same banks: that two-way conflict is what the
//     slot's order is there to remove; the operand's rows follow it at no cost.)
//   the GEMM reads (ds_read_b32): lane (j, kq) reads frame j, slot 4 s + kq: a group's lanes are at 2 j + (kq & 1) + const
//     modulo 32: 32 banks once.  Lanes with j >= tile (tile 8 or 4) read nothing and feed zeros.
//   There is no store loop through LDS: the GEMM's result has consecutive frames in consecutive lanes (see mel_long.hip) and
//   goes to memory from the registers.
MEL_FN int mell_p_stride(int N2) { return mell_slots(N2) + 2; }
MEL_FN unsigned mell_p_at(int fl, int slot, int N2) { return (unsigned)(fl * mell_p_stride(N2) + slot); }
MEL_FN unsigned mell_p_floats(int tile, int N2) { return (unsigned)(tile * mell_p_stride(N2)); }
// floats of the span's region: the tile's span rounded up to 4
MEL_FN unsigned mell_span_floats(int tile, int hop, int n_fft) { return (stftl_span(tile, hop, n_fft) + 3u) & ~3u; }
MEL_FN unsigned mell_lds_floats(int tile, int hop, int n_fft) {
  return mell_span_floats(tile, hop, n_fft) + stftl_z_floats(tile, stftl_n2(n_fft)) + mell_p_floats(tile, stftl_n2(n_fft));
}

}  // namespace pdmp3
#endif
