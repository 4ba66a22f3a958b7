"""Log-mel features of clips at n_fft 2048 and 4096 (include/pdmp3_bulk.h pdmp3_amd_mel_long_*) restated
with numpy alone: the plan of a workgroup of k_clip_mel_long, the order in which it meets the bins -- and the binary32 error
bound the tests hold the product to.  Nothing here is the product's code.

The definition is made of two that exist: clip_stft_ref.stft gives the spectrum X of section 14's frame (window wt with s = 1,
no `normalized`) in binary64, clip_mel_ref.filterbank gives W at K = N / 2 + 1 bins (it takes any n_fft); P = Re^2 + Im^2,
M = W P, modes 0 (M), 1 (ln max(M, floor)), 2 (log10 max(M, floor)).

The bound is section 10's chain with section 14's first link; nothing is measured here and there is no new constant.
  E  = c(N) u A            bounds Re and Im (clip_stft_long_ref.c_of; A = sum |wt y| of the frame)
  X  = 2 (|Re| + |Im|) E + 2 E^2
  dP = X + (2 u + u^2) (P + X)                       fma(Im, Im, fl(Re Re)) on a pair within E of the true one
  dM = W dP + (K_m + 2) u W (P + dP)                 K_m = the non-zero weights of row m: a chain of K_m fused steps that
                                                     matter (a zero weight's step adds an exact zero: any order, any
                                                     number of them), one rounding of each weight, one u of second order
  logs: clip_mel_ref._log_term with the project's LOG_C.
The Nyquist bin takes part in the definition (W has its column); the product never computes it, which is right because the
column is exactly zero (asserted where the filterbank is tested)."""
import math

import numpy as np

import clip_mel_ref as mref
import clip_stft_long_ref as lref
import clip_stft_ref as sref

U = sref.U
LDS_MAX = 160 * 1024 - 64
SIZES = (2048, 4096)
MODES = ["power", "log", "log10"]
PATHS = ("N2048-tile16", "N2048-tile8", "N4096-tile8", "N4096-tile4")


def plan(n_fft, hop, n_mels):
    """the plan of a workgroup of k_clip_mel_long restated: (tile, row_pad = 0, lds_bytes, launch path).  LDS: the span
    (kept), Z, the powers of one tile of k1 -- tile x (8 N2 + 2) floats; the accumulators are registers"""
    assert n_fft in SIZES and 1 <= hop <= n_fft and 1 <= n_mels <= 256
    n2 = n_fft // 64
    for tile in (16, 8, 4):
        span = ((tile - 1) * hop + n_fft + 3) // 4 * 4
        lds = (span + tile * n2 * 32 + tile * (8 * n2 + 2)) * 4
        if lds <= LDS_MAX:
            return tile, 0, lds, "N%d-tile%d" % (n_fft, tile)
    raise AssertionError("no plan")


def last_hop(n_fft, tile):
    """the largest hop that still takes `tile` frames (None where none does), by plan()'s arithmetic"""
    hops = [h for h in range(1, n_fft + 1) if plan(n_fft, h, 1)[0] == tile]
    return max(hops) if hops else None


def slot(k1l, k2, n2):
    """where bin (k1l, k2) of a tile of k1 lies among its 8 N2"""
    return 32 * (((k1l & 3) | ((k1l >> 3) << 2)) * (n2 // 32) + (k2 >> 4)) + 16 * ((k1l >> 2) & 1) + (k2 & 15)


def operand_row(k, n_fft):
    """the operand's row of bin k < N / 2: k = 16 kt + k1l + 64 k2"""
    n2 = n_fft // 64
    return 8 * n2 * ((k % 64) // 16) + slot(k % 16, k // 64, n2)


def mel_all(y, pos0, start, n_frames, n_fft, hop, w, floor=1e-10, win_length=None, window=None, modes=range(3)):
    """y: [C, T] binary32 values of the signal from position pos0 on; w: clip_mel_ref.filterbank(..) at n_fft.
    -> {mode: (out, bound)}, binary64 [C, n_mels, F]: the definition, and what the binary32 evaluation may differ from it by"""
    floor = float(np.float32(floor))
    x, b0 = sref.stft(y, pos0, start, n_frames, n_fft, hop, 0, 1e-10, win_length, window, False)      # [C, K, F, 2]
    e = b0[..., 0] * (lref.c_of(n_fft) / (n_fft + 2))                          # (clip_stft_ref's E is (N + 2) u A)
    re, im = x[..., 0], x[..., 1]
    p = re * re + im * im
    cross = 2.0 * (np.abs(re) + np.abs(im)) * e + 2.0 * e * e
    dp = cross + sref.T2 * (p + cross)
    km = (w > 0).sum(axis=1).astype(np.float64)[None, :, None]
    m = np.einsum("mk,ckf->cmf", w, p)
    dm = np.einsum("mk,ckf->cmf", w, dp) + (km + 2.0) * U * np.einsum("mk,ckf->cmf", w, p + dp)
    res = {}
    for mode in modes:
        if mode == 0:
            res[0] = (m, dm)
            continue
        base = math.e if mode == 1 else 10.0
        out = np.log(np.maximum(m, floor)) / (1.0 if mode == 1 else math.log(10.0))
        res[mode] = (out, mref._log_term(m, dm, out, base, floor))
    return res


def gemm_bound(w, p):
    """W @ p evaluated in binary32 as one fused chain a band over given binary32 powers p [.., K, F], weights rounded once:
    -> (W p in binary64, (K_m + 2) u W p)"""
    km = (w > 0).sum(axis=1).astype(np.float64)[:, None]
    m = np.einsum("mk,...kf->...mf", w, p)
    return m, (km + 2.0) * U * m
