"""The constant-Q transform of clips (include/pdmp3_bulk.h) restated in binary64 with numpy alone: the
bins, the ragged folded table, the kernel's plan, the five output modes -- and the binary32 error bound the tests hold the
product to.  Nothing here is the product's code.

Definition.
  1. Signal.  y[j] is the binary32 output of the audio call at the requested rate sr for 0 <= j < J, 0.0 outside.
  2. Bins, B = bins_per_octave, k < n_bins:  f_k = fmin 2^(k / B);  Q = filter_scale / (2^(1 / B) - 1);  L_k = Q sr / f_k;
     h_k = floor(L_k / 2);  N_k = 2 h_k + 1;  g_k[m] = 0.5 - 0.5 cos(2 pi (m + h_k) / N_k), m = -h_k .. h_k;
     s_k = n_k a_k -- n_k: norm 0: 1, 1: 1 / sum g_k, 2: 1 / sqrt(sum g_k^2); a_k: scale 0: 1, 1: sqrt(L_k), 2: L_k.
  3. C[f, k] = s_k sum_m g_k[m] y[start + f H + m] e^(-2 pi i f_k m / sr): frame f is centred on start + f H, no reflection.
     The angle: x = m f_k / sr in binary64, reduced to x - floor(x), then times 2 pi.
  4. Modes: 0 (Re, Im); 1 sqrt(Re^2 + Im^2); 2 P = Re^2 + Im^2; 3 ln max(P, floor); 4 log10 max(P, floor); floor rounded to
     binary32 first.

The bound (u = 2^-24), for Re and for Im of bin k of a frame:
  E_k = (N_k + 2) u A_k,  A_k = sum_m |s_k g_k[m] y[..]|.
  This is clip_stft_ref's E with N_k in the place of N.  The product computes the sum as binary32 fused multiply-add chains
  over rows of a table whose entries are the binary64 coefficients rounded once (relative error u each: u A_k in all).  A
  chain of n terms from +0 commits n roundings, each at most u times the partial sum's magnitude, which is at most the sum of
  the |terms| so far times (1 + u)^n: to first order a term passes at most as many roundings as there are steps after it
  enters.  The product may cut the N_k terms into P non-empty segments, run a chain from +0 over each and add the P partial
  sums in a fixed order ((p0 + p1) + p2) + ...: a term of a segment of n_s terms then passes at most n_s roundings of its own
  chain and at most P - 1 of the additions, n_s + P - 1 <= N_k since the other P - 1 segments hold a term each.  Rows outside a
  bin's own support carry an exact zero coefficient: fma(a, 0, acc) = acc exactly, no rounding.  So N_k u A_k covers the sums
  for every such plan, one u A_k the coefficients, and one more u A_k the second-order terms ((1 + u)^(N_k + 1) - 1 <=
  (N_k + 2) u for N_k u < 0.01: N_k <= 32 767 gives 0.002).  The bound does not depend on the plan.
  Modes 1 - 4 chain on E_k exactly as clip_stft_ref does: SQRT_C, T2, clip_mel_ref._log_term with the project's LOG_C.  No new
  measured constant."""
import functools
import math

import numpy as np

import clip_mel_ref as mref
import clip_stft_ref as sref

U = mref.U
LOG_C = mref.LOG_C
MODES = sref.MODES
T2 = sref.T2
SQRT_C = sref.SQRT_C
FMIN_C1 = 32.70319566257483
MAX_LEN = 32767
SPLIT_ROWS = 512
SEGMENTS = 8
PART_FLOATS = 8 * 2 * 16 * 17
LDS_SOFT = mref.LDS_SOFT
LDS_MAX = mref.LDS_MAX

valid = mref.valid


def lengths(sr, fmin=FMIN_C1, n_bins=84, bins_per_octave=12, filter_scale=1.0):
    """-> (f_k float64 [n_bins], L_k float64, h_k int64)"""
    k = np.arange(n_bins, dtype=np.float64)
    f = fmin * 2.0 ** (k / bins_per_octave)
    q = filter_scale / (2.0 ** (1.0 / bins_per_octave) - 1.0)
    L = q * float(sr) / f
    return f, L, np.floor(0.5 * L).astype(np.int64)


@functools.lru_cache(maxsize=8)
def filters(sr, fmin=FMIN_C1, n_bins=84, bins_per_octave=12, filter_scale=1.0, norm=1, scale=1):
    """-> per bin (h_k, re [N_k], im [N_k]) in binary64: s_k g_k[m] cos(2 pi f_k m / sr) and -s_k g_k[m] sin(..), m = -h_k .. h_k"""
    f, L, h = lengths(sr, fmin, n_bins, bins_per_octave, filter_scale)
    out = []
    for k in range(n_bins):
        hk = int(h[k])
        m = np.arange(-hk, hk + 1, dtype=np.float64)
        g = 0.5 - 0.5 * np.cos(2.0 * np.pi * (m + hk) / (2 * hk + 1))
        nk = 1.0 / g.sum() if norm == 1 else 1.0 / math.sqrt((g * g).sum()) if norm == 2 else 1.0
        ak = math.sqrt(L[k]) if scale == 1 else L[k] if scale == 2 else 1.0
        x = m * f[k] / float(sr)
        a = 2.0 * np.pi * (x - np.floor(x))
        w = nk * ak * g
        out.append((hk, w * np.cos(a), -w * np.sin(a)))
    return out


def tiles(sr, **kw):
    """the ragged table's tiles: (rows of each, first row of each), from the half lengths of bins 0, 16, 32, ..."""
    h = lengths(sr, **kw)[2][::16]
    rows = (2 * h + 1 + 3) // 4 * 4
    return rows, np.concatenate([[0], np.cumsum(rows)[:-1]])


def table(sr, fmin=FMIN_C1, n_bins=84, bins_per_octave=12, filter_scale=1.0, norm=1, scale=1):
    """the product's table layout in binary64: [rows, 32] and a mask of the entries that belong to a bin's own support"""
    geo = dict(fmin=fmin, n_bins=n_bins, bins_per_octave=bins_per_octave, filter_scale=filter_scale)
    rows, at = tiles(sr, **geo)
    t = np.zeros((int(rows.sum()), 32), dtype=np.float64)
    own = np.zeros(t.shape, dtype=bool)
    fl = filters(sr, norm=norm, scale=scale, **geo)
    for k, (hk, re, im) in enumerate(fl):
        ht = fl[k // 16 * 16][0]
        r0 = int(at[k // 16]) + ht - hk
        t[r0:r0 + 2 * hk + 1, k % 16] = re
        t[r0:r0 + 2 * hk + 1, 16 + k % 16] = im
        own[r0:r0 + 2 * hk + 1, [k % 16, 16 + k % 16]] = True
    return t, own, rows, at


def plan(sr, hop, **kw):
    """the plan of a workgroup of k_clip_cqt restated: (tile, row_pad, lds_bytes, split rows, segments, split tiles, launch
    path), None where no tile fits the LDS"""
    rows, _ = tiles(sr, **kw)
    pad = (2 - hop) % 32
    n_split = int((rows >= SPLIT_ROWS).sum())
    assert (np.diff(rows) <= 0).all()
    for tile in (16, 8, 4):
        span = (tile - 1) * hop + int(rows[0])
        lds = ((-(-span // hop) * (hop + pad) + 3) // 4 * 4 + PART_FLOATS) * 4
        if lds <= LDS_MAX:
            return tile, pad, lds, SPLIT_ROWS, SEGMENTS, n_split, "tile%d-%s" % (tile, "dyn" if lds <= LDS_SOFT else "static")
    return None


def segments_of(rows):
    """the rows [a, b) of the eight segments of a split tile of `rows` rows"""
    q = (-(-rows // SEGMENTS) + 3) // 4 * 4
    return [(min(s * q, rows), min((s + 1) * q, rows)) for s in range(SEGMENTS)]


def frames_of(y, pos0, start, n_frames, half, hop):
    """y[t] is the signal at position pos0 + t (0.0 everywhere else) -> [n_frames, 2 half + 1] binary64, frame f centred on
    start + f hop"""
    return mref.frames_of(y, pos0, start, n_frames, 2 * half + 1, hop)      # ((2 half + 1) // 2 = half samples lie in front of the centre)


def cqt(y, pos0, start, n_frames, sr, hop, mode, floor=1e-10, **kw):
    """y: [C, T] binary32 values of the signal from position pos0 on.  -> (out, bound), binary64: mode 0 [C, n_bins, F, 2], else
    [C, n_bins, F]: the definition on those values, and what a binary32 evaluation may differ from it by (the module's docstring)"""
    y = np.atleast_2d(np.asarray(y, dtype=np.float64))
    floor = float(np.float32(floor))
    fl = filters(sr, **kw)
    outs, bounds = [], []
    for ch in range(y.shape[0]):
        re = np.zeros((len(fl), n_frames))
        im = np.zeros((len(fl), n_frames))
        e = np.zeros((len(fl), n_frames))
        h0 = fl[0][0]
        big = frames_of(y[ch], pos0, start, n_frames, h0, hop)
        for k, (hk, cr, ci) in enumerate(fl):
            fr = big[:, h0 - hk:h0 + hk + 1]
            re[k] = fr @ cr
            im[k] = fr @ ci
            e[k] = (2 * hk + 1 + 2) * U * (np.abs(fr) @ np.hypot(cr, ci))
        if mode == 0:
            outs.append(np.stack([re, im], axis=-1))
            bounds.append(np.stack([e, e], axis=-1))
            continue
        p = re * re + im * im
        if mode == 1:
            mag = np.sqrt(p)
            r2e = math.sqrt(2.0) * e
            outs.append(mag)
            bounds.append(r2e + (mag + r2e) * SQRT_C)
            continue
        cross = 2.0 * (np.abs(re) + np.abs(im)) * e + 2.0 * e * e
        dp = cross + T2 * (p + cross)
        if mode == 2:
            outs.append(p)
            bounds.append(dp)
            continue
        base = math.e if mode == 3 else 10.0
        out = np.log(np.maximum(p, floor)) / (1.0 if mode == 3 else math.log(10.0))
        outs.append(out)
        bounds.append(mref._log_term(p, dp, out, base, floor))
    return np.stack(outs), np.stack(bounds)
