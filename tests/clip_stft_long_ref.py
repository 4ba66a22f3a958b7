"""The short-time Fourier transform of clips at n_fft 2048 and 4096 (include/pdmp3_bulk.h pdmp3_amd_stft_long_*, DESIGN.md
section 14) restated with numpy alone: the four tables of the two-stage transform in binary64, the factorisation, the plan of
a workgroup -- and the binary32 error bound the tests hold the product to.  The definition itself is section 13's on a wider
domain: clip_stft_ref.stft evaluates it in binary64 for any even N.  Nothing here is the product's code.

The arithmetic.  N = 64 N2, n = N2 n1 + n2, k = k1 + 64 k2; tables in binary64, angles reduced as integers, rounded once.
  0. wt[n] = fl(s w[n]);  xw[n] = fl(wt[n] y[n]).
  1. Y[n2][k1] = sum_n1 xw[N2 n1 + n2] e^(-2 pi i n1 k1 / 64): one fused chain of 64 terms for Re, one for Im.
  2. Z = Y T, T = fl(e^(-2 pi i n2 k1 / N)):  Zr = fma(Yr, Tr, -fl(Yi Ti)),  Zi = fma(Yr, Ti, fl(Yi Tr)).
  3. X[k1 + 64 k2] = sum_n2 Z[n2][k1] e^(-2 pi i n2 k2 / N2): one fused chain of 2 N2 terms for Re (Zr cos a, Zi sin a, n2
     ascending) and one for Im (Zr (-sin a), Zi cos a); the Nyquist bin is the chain at k1 = 0, k2 = N2 / 2.

The bound (u = 2^-24; a_n = |s w[n] y[n]|, A = sum_n a_n of the frame, A_n2 = sum_n1 a_(N2 n1 + n2), so sum_n2 A_n2 = A).
Errors are followed as complex magnitudes, so that a rotation by a factor of modulus 1 does not grow them; the error of Re or
of Im of a bin is at most the magnitude of the bin's error.  A coefficient cos or sin of a table is fl(c) of a binary64 value
within tau = 2^-49 of the true one: |c~ - c| <= u |c| + tau.  g(m) = m u / (1 - m u) is the usual constant of a chain of m
fused steps: the computed sum is sum_i x_i c~_i (1 + th_i), |th_i| <= g(m).
  step 0.  |xw[n] - s w[n] y[n]| <= e0 a_n, e0 = 2 u + u^2 (two roundings), and |xw[n]| <= (1 + u)^2 a_n.
  step 1.  The computed pair Y^ against the exact 64-point transform Y* of the computed xw: term i contributes
           xw_i ((c~ (1 + th) - c) + i (s~ (1 + th') - s)), and |c~ (1 + th) - c| <= |c| (g + u (1 + g)) + tau (1 + g); with
           c^2 + s^2 = 1 the pair's magnitude is at most e1 = g(64) + u (1 + g(64)) + 2 tau.  So |Y^ - Y*| <= e1 B_n2,
           B_n2 = sum_n1 |xw| <= (1 + u)^2 A_n2, and |Y^| <= (1 + e1) B_n2.
  step 2.  Z^ against Y^ T (T exact): the inner products' roundings are the pair (u |Yi T~i|, u |Yi T~r|), magnitude at
           most u |Y^| |T~|; the outer fused steps' roundings u |(Zr~, Zi~)| <= u |Y^| |T~| (1 + u); the coefficients'
           error |Y^| |T~ - T| <= |Y^| (u + 2 tau); |T~| <= 1 + u + 2 tau =: tm.  |Z^ - Y^ T| <= e2 |Y^|,
           e2 = u tm + u tm (1 + u) + u + 2 tau: three roundings a component.  |Z^| <= (tm + e2) |Y^|.
  step 3.  The computed X^ against the exact N2-point sum over the computed Z^: term n2 of Re contributes
           Zr (c~ (1 + th) - c) + Zi (s~ (1 + th') - s), at most |Z^| (g(2 N2) + u (1 + g(2 N2))) + 2 tau (1 + g) |Z^| by
           Cauchy-Schwarz on (|Zr|, |Zi|) . (|c|, |s|) (the issue's sqrt 2 on |Zr| + |Zi| is not needed: the coefficients
           of one n2 are a unit vector); the same for Im.  e3 = g(2 N2) + u (1 + g(2 N2)) + 4 tau.
  together.  X^ - X = [step 3's error] + sum_n2 w2 (Z^ - Y^ T) + sum_n2 w2 T (Y^ - Y*) + sum_n2 w2 T (Y* - Y), |w2| = |T| = 1:
           |X^ - X| <= sum_n2 [ e3 |Z^| + e2 |Y^| + e1 B_n2 + e0 A_n2 ]
                    <= A [ e0 + (1 + u)^2 (e1 + (1 + e1) (e2 + (tm + e2) e3)) ] =: c(N) u A = E.
  c(2048) = 135.0..., c(4096) = 199.0...: 2 + 65 + 3 + (2 N2 + 1) and second-order terms -- below section 13's N + 2 for the
  direct chain of the same length, as it must be.  The Nyquist bin's chain is step 3's with exact coefficients: inside E.
Modes 1 .. 4: clip_stft_ref's formulas on this E, with its SQRT_C, T2 and clip_mel_ref._log_term / LOG_C.  Underflow is left
out as in section 13 (the products of a frame that holds signal are far above binary32's subnormals)."""
import math

import numpy as np

import clip_mel_ref as mref
import clip_stft_ref as sref

U = sref.U
TAU = 2.0 ** -49
LDS_MAX = 160 * 1024 - 64
SIZES = (2048, 4096)


def gamma(m):
    return m * U / (1.0 - m * U)


def c_of(n_fft):
    """c(N) of the module's docstring: E = c(N) u A"""
    n2 = n_fft // 64
    e0 = 2.0 * U + U * U
    e1 = gamma(64) + U * (1.0 + gamma(64)) + 2.0 * TAU
    tm = 1.0 + U + 2.0 * TAU
    e2 = U * tm + U * tm * (1.0 + U) + U + 2.0 * TAU
    e3 = gamma(2 * n2) + U * (1.0 + gamma(2 * n2)) + 4.0 * TAU
    return (e0 + (1.0 + U) ** 2 * (e1 + (1.0 + e1) * (e2 + (tm + e2) * e3))) / U


def tables(n_fft, win_length=None, window=None, normalized=False):
    """the four tables in binary64, in the product's layouts: wt [N], D64 [64, 128], H2 [2 N2, N2], TW [N2, 128]"""
    n2 = n_fft // 64
    k2n = n2 // 2
    wt = sref.scale(n_fft, normalized) * sref.frame_window(n_fft, win_length, window)
    n1 = np.arange(64, dtype=np.int64)[:, None]
    k1 = np.arange(64, dtype=np.int64)[None, :]
    a = 2.0 * np.pi * ((n1 * k1) % 64).astype(np.float64) / 64.0
    d64 = np.concatenate([np.cos(a), -np.sin(a)], axis=1)
    m = np.arange(n2, dtype=np.int64)[:, None]
    a = 2.0 * np.pi * ((m * np.arange(k2n, dtype=np.int64)[None, :]) % n2).astype(np.float64) / n2
    h2 = np.zeros((2 * n2, n2), dtype=np.float64)
    h2[0::2, :k2n], h2[1::2, :k2n] = np.cos(a), np.sin(a)
    h2[0::2, k2n:], h2[1::2, k2n:] = -np.sin(a), np.cos(a)
    a = 2.0 * np.pi * (m * k1).astype(np.float64) / n_fft
    tw = np.concatenate([np.cos(a), -np.sin(a)], axis=1)
    return wt, d64, h2, tw


def two_stage(frames, tabs):
    """frames [F, N] binary64 (not yet windowed) through the factorisation with the binary64 tables -> complex [N / 2 + 1, F]"""
    wt, d64, h2, tw = tabs
    n_fft = wt.size
    n2 = n_fft // 64
    k2n = n2 // 2
    xw = (frames * wt[None, :]).reshape(frames.shape[0], 64, n2)             # [F, n1, n2]
    w64 = d64[:, :64] + 1j * d64[:, 64:]
    y = np.einsum("fab,ak->fbk", xw, w64)                                   # [F, n2, k1]
    z = y * (tw[:, :64] + 1j * tw[:, 64:])[None]
    zt = np.stack([z.real, z.imag], axis=2).reshape(z.shape[0], 2 * n2, 64)  # [F, t = 2 n2 + part, k1]
    re = np.einsum("ftk,tq->fqk", zt, h2[:, :k2n])                          # [F, k2, k1]
    im = np.einsum("ftk,tq->fqk", zt, h2[:, k2n:])
    x = (re + 1j * im).reshape(frames.shape[0], n_fft // 2)                  # k = 64 k2 + k1
    sign = np.where(np.arange(n2) % 2 == 0, 1.0, -1.0)
    nyq = (z[:, :, 0] * sign[None, :]).sum(axis=1)
    return np.concatenate([x, nyq[:, None]], axis=1).T


def plan(n_fft, hop, mode):
    """the plan of a workgroup of k_clip_stft_long restated: (tile, row_pad = 0, lds_bytes, launch path)"""
    n2 = n_fft // 64
    for tile in (16, 8, 4):
        span = (tile - 1) * hop + n_fft
        stage = (2 if mode == 0 else 1) * 16 * (n2 // 2) * (tile + 1)
        lds = ((max(span, stage) + 3) // 4 * 4 + tile * n2 * 32) * 4
        if lds <= LDS_MAX:
            return tile, 0, lds, "N%d-tile%d" % (n_fft, tile)
    raise AssertionError("no plan")


PATHS = ("N2048-tile16", "N2048-tile8", "N4096-tile8", "N4096-tile4")


def stft_all(y, pos0, start, n_frames, n_fft, hop, floors=None, win_length=None, window=None, normalized=False, modes=range(5)):
    """y as clip_stft_ref.stft takes it -> {mode: (out, bound)}, binary64, in clip_stft_ref.stft's shapes: the definition, and
    what the two-stage binary32 evaluation may differ from it by"""
    floors = floors or {}
    out0, b0 = sref.stft(y, pos0, start, n_frames, n_fft, hop, 0, 1e-10, win_length, window, normalized)
    e = b0[..., 0] * (c_of(n_fft) / (n_fft + 2))                             # (clip_stft_ref's E is (N + 2) u A)
    re, im = out0[..., 0], out0[..., 1]
    res = {}
    for mode in modes:
        if mode == 0:
            res[0] = (out0, np.stack([e, e], axis=-1))
            continue
        p = re * re + im * im
        if mode == 1:
            mag = np.sqrt(p)
            r2e = math.sqrt(2.0) * e
            res[1] = (mag, r2e + (mag + r2e) * sref.SQRT_C)
            continue
        cross = 2.0 * (np.abs(re) + np.abs(im)) * e + 2.0 * e * e
        dp = cross + sref.T2 * (p + cross)
        if mode == 2:
            res[2] = (p, dp)
            continue
        floor = float(np.float32(floors.get(mode, 1e-10)))
        base = math.e if mode == 3 else 10.0
        out = np.log(np.maximum(p, floor)) / (1.0 if mode == 3 else math.log(10.0))
        res[mode] = (out, mref._log_term(p, dp, out, base, floor))
    return res
