"""Kaldi-style filterbank features of clips (include/pdmp3_bulk.h) restated step by step -- never
through the folded table -- in binary64 with numpy alone: framing, DC removal, raw energy, pre-emphasis, the five windows, the
DFT without its Nyquist bin, the mel filterbank, the logarithm, the energy column, the mean subtraction -- and the binary32 error
bound the tests hold the product to.  Nothing here is the product's code.

torchaudio is not installed where this was written, so nothing independent pins this restatement to Kaldi: it was written from
the published definitions of torchaudio.compliance.kaldi.fbank, and a reader should compare it with them."""
import functools
import math

import numpy as np

U = 2.0 ** -24                                     # unit roundoff of binary32
EPS = 2.0 ** -23                                   # the floor of the logarithms: binary32's epsilon
# the device's logf: largest error in units of u * max(1, |result|), plus one ulp -- the project's own measured constant
# (profiles/clip_mel_tests.txt: tools/ubench/logf_ulp.cpp on an MI355X); only logf is used here
LOG_C = 2.81 + 2.0
# a binary32 division: correctly rounded (u) where the compiler keeps IEEE division, 2.5 ulp = 5 u where it does not
DIV_C = 5.0

WINDOWS = ("povey", "hanning", "hamming", "rectangular", "blackman")


def gamma(n):
    """Higham's gamma_n for binary32: n roundings compound to at most this relative error"""
    return n * U / (1.0 - n * U)


def dft_length(nw, round_pow2=True):
    if not round_pow2:
        return nw
    n = 2
    while n < nw:
        n *= 2
    return n


def window(kind, nw, blackman_coeff=0.42):
    t = 2.0 * np.pi * np.arange(nw, dtype=np.float64) / (nw - 1)
    if kind == "povey":
        return (0.5 - 0.5 * np.cos(t)) ** 0.85
    if kind == "hanning":
        return 0.5 - 0.5 * np.cos(t)
    if kind == "hamming":
        return 0.54 - 0.46 * np.cos(t)
    if kind == "rectangular":
        return np.ones(nw)
    if kind == "blackman":
        return blackman_coeff - 0.5 * np.cos(t) + (0.5 - blackman_coeff) * np.cos(2.0 * t)
    raise ValueError(kind)


@functools.lru_cache(maxsize=8)
def dft_matrices(nw, n):
    """(cos, -sin) of 2 pi k m / N for m < Nw, k < N / 2: [Nw, N / 2], the angle reduced as the integer k m mod N"""
    m = np.arange(nw, dtype=np.int64)[:, None]
    k = np.arange(n // 2, dtype=np.int64)[None, :]
    a = 2.0 * np.pi * ((k * m) % n).astype(np.float64) / n
    return np.cos(a), -np.sin(a)


def frame_steps(s, rho, win, remove_dc):
    """steps 1 .. 4 on frames s [F, Nw] (already scaled) -> (w p, E)"""
    a = s - s.mean(axis=1, keepdims=True) if remove_dc else s
    e = (a * a).sum(axis=1)
    p = np.empty_like(a)
    p[:, 1:] = a[:, 1:] - rho * a[:, :-1]
    p[:, 0] = a[:, 0] - rho * a[:, 0]
    return p * win[None, :], e


def folded(nw, n, rho, win, remove_dc, scale):
    """the fold of include/pdmp3_bulk.h in binary64 (for the table's test, and |T| of the bound): T [Nw, 2 * N / 2], Re then Im"""
    c, s = dft_matrices(nw, n)
    out = []
    for m in (c, s):
        cw = np.vstack([m * win[:, None], np.zeros((1, n // 2))])
        d = cw[:-1] - rho * cw[1:]
        d[0] -= rho * cw[0]
        if remove_dc:
            d = d - d.sum(axis=0, keepdims=True) / nw
        out.append(scale * d)
    return np.hstack(out)


@functools.lru_cache(maxsize=8)
def _abs_folded(nw, n, rho, window_type, blackman_coeff, remove_dc, scale):
    return np.abs(folded(nw, n, rho, window(window_type, nw, blackman_coeff), remove_dc, scale))


def mel_scale(f):
    return 1127.0 * np.log(1.0 + np.asarray(f, dtype=np.float64) / 700.0)


def filterbank(sr, n, n_mels, low_freq=20.0, high_freq=0.0):
    """W[m, k] in binary64, [n_mels, N / 2]: triangles linear in mel"""
    hi = sr / 2.0 + high_freq if high_freq <= 0.0 else high_freq
    m_lo, m_hi = float(mel_scale(low_freq)), float(mel_scale(hi))
    d = (m_hi - m_lo) / (n_mels + 1)
    mk = mel_scale(np.arange(n // 2, dtype=np.float64) * sr / n)
    w = np.zeros((n_mels, n // 2), dtype=np.float64)
    for m in range(n_mels):
        l = m_lo + m * d
        c, r = l + d, l + 2.0 * d
        w[m] = np.maximum(0.0, np.minimum((mk - l) / (c - l), (r - mk) / (r - c)))
    return w


def valid(n_out, start, nw, hop, n_frames):
    if n_out - start < nw:
        return 0
    return min(n_frames, (n_out - start - nw) // hop + 1)


def frames_of(y, pos0, start, n_frames, nw, hop):
    """y[t] is the signal at position pos0 + t (0.0 everywhere else) -> [n_frames, Nw] binary64, frame f from start + f hop on"""
    y = np.asarray(y, dtype=np.float64)
    idx = (start - pos0) + np.arange(n_frames, dtype=np.int64)[:, None] * hop + np.arange(nw, dtype=np.int64)[None, :]
    ok = (idx >= 0) & (idx < y.size)
    return np.where(ok, y[np.clip(idx, 0, max(y.size - 1, 0))] if y.size else 0.0, 0.0)


def _log_bound(v, dv, out):
    return dv / np.maximum(v - dv, EPS) + LOG_C * U * np.maximum(1.0, np.abs(out))


def fbank(y, pos0, start, n_frames, nw, hop, w, n_valid, round_pow2=True, remove_dc=True, rho=0.97, window_type="povey", blackman_coeff=0.42,
          mode=1, use_energy=False, htk_compat=False, energy_floor=0.0, subtract_mean=False, scale=1.0):
    """y: [C, T] binary32 values of the signal from position pos0 on; w: filterbank(...).  -> (out, bound), binary64
    [C, n_frames, D]: the definition on those values, and what a binary32 evaluation may differ from it by (DESIGN.md
    section 11), u = 2^-24, g_n = n u / (1 - n u):
      Re, Im:  E_k = (Nw + 2) u sum_n |T[n, k]| |y[n]|  -- a length-Nw binary32 dot product with the once-rounded folded
               coefficients, any summation order (g_Nw (1 + u) + u <= (Nw + 2) u for Nw <= 1024); |T| comes from folded() above,
               numpy's own fold, which the host test holds to the steps; the values themselves go step by step
      dP = 2 |Re| E_re + E_re^2 + 2 |Im| E_im + E_im^2 + (2 u + u^2) (P + the same cross terms)
      dM = W dP + (K_m + 2) u W (P + dP),  K_m = the non-zero weights of row m
      ln:  dM / max(M - dM, eps) + c u max(1, |out|)
      energy, with s^ = fl(scale y) (u |s|), the mean as any-order sum and one division:
        dmean = (g_(Nw-1) (1 + u) + u + DIV_C u (1 + g_Nw)) * mean|s|  (0 without DC removal)
        e_n   = (u |s_n| + dmean) (1 + u) + u |a_n|           -- the error of a^_n = fl(s^_n - mean^)
        dE    = sum (2 |a_n| e_n + e_n^2) + g_(Nw+1) sum (|a_n| + e_n)^2   -- an any-order sum of Nw fused multiply-adds
        column: dE, or dE / max(E - dE, eps) + c u max(1, |ln|) and u |ln energy_floor| for the floor's own rounding
      subtract_mean over nv = valid frames: with b the bound so far and v the value,
        dmu = (sum b + g_(nv-1) sum (|v| + b)) / nv + DIV_C u (|mu| + the former)
        final = b + dmu + u (|v - mu| + b + dmu)"""
    y = np.atleast_2d(np.asarray(y, dtype=np.float64))
    n = dft_length(nw, round_pow2)
    win = window(window_type, nw, blackman_coeff)
    c, s = dft_matrices(nw, n)
    t_abs = _abs_folded(nw, n, rho, window_type, blackman_coeff, remove_dc, scale)   # only |T| for the bound; the values go step by step
    k2 = n // 2
    km = (w > 0).sum(axis=1).astype(np.float64)[:, None]
    outs, bounds = [], []
    for ch in range(y.shape[0]):
        fr = frames_of(y[ch], pos0, start, n_frames, nw, hop)
        sc = scale * fr
        wp, en = frame_steps(sc, rho, win, remove_dc)
        re, im = wp @ c, wp @ s
        p = re * re + im * im                                               # [F, N / 2]
        e_all = (nw + 2) * U * (np.abs(fr) @ t_abs)
        e_re, e_im = e_all[:, :k2], e_all[:, k2:]
        cross = 2.0 * np.abs(re) * e_re + e_re * e_re + 2.0 * np.abs(im) * e_im + e_im * e_im
        dp = cross + (2.0 * U + U * U) * (p + cross)
        m = (w @ p.T).T                                                     # [F, n_mels]
        dm = (w @ dp.T + (km + 2.0) * U * (w @ (p + dp).T)).T
        if mode == 1:
            out = np.log(np.maximum(m, EPS))
            bound = _log_bound(m, dm, out)
        else:
            out, bound = m, dm
        if use_energy:
            a_abs = np.abs(sc - sc.mean(axis=1, keepdims=True)) if remove_dc else np.abs(sc)
            s_abs = np.abs(sc)
            dmean = ((gamma(nw - 1) * (1.0 + U) + U + DIV_C * U * (1.0 + gamma(nw))) * s_abs.mean(axis=1, keepdims=True)) if remove_dc else 0.0
            e_n = (U * s_abs + dmean) * (1.0 + U) + U * a_abs
            de = (2.0 * a_abs * e_n + e_n * e_n).sum(axis=1) + gamma(nw + 1) * ((a_abs + e_n) ** 2).sum(axis=1)
            if mode == 1:
                col = np.log(np.maximum(en, EPS))
                dcol = _log_bound(en, de, col)
                if energy_floor > 0.0:
                    lf = math.log(energy_floor)
                    col = np.maximum(col, lf)
                    dcol = dcol + U * abs(lf)
            else:
                col, dcol = en, de
            parts = ((out, col[:, None]), (bound, dcol[:, None])) if htk_compat else ((col[:, None], out), (dcol[:, None], bound))
            out, bound = np.hstack(parts[0]), np.hstack(parts[1])
        if subtract_mean and n_valid > 0:
            nv = int(n_valid)
            mu = out[:nv].mean(axis=0)
            dsum = bound[:nv].sum(axis=0) + gamma(max(nv - 1, 0)) * (np.abs(out[:nv]) + bound[:nv]).sum(axis=0)
            dmu = dsum / nv
            dmu = dmu + DIV_C * U * (np.abs(mu) + dmu)
            v = out - mu[None, :]
            bound = bound + dmu[None, :] + U * (np.abs(v) + bound + dmu[None, :])
            out = v
        outs.append(out)
        bounds.append(bound)
    return np.stack(outs), np.stack(bounds)
