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


# ---- the plan of a workgroup of k_clip_fbank restated, and the classes of a geometry ("launch forms") ----
def form(nw, n, hop, n_mels):
    """-> (tile, row_pad, lds_bytes, classes): clip_mel_ref.form with this kernel's rows (Nw rounded up to 4) and bins (N / 2
    rounded up to 16, no Nyquist bin)"""
    import clip_mel_ref as mref
    rows, kp, mp = (nw + 3) // 4 * 4, (n // 2 + 15) // 16 * 16, (n_mels + 15) // 16 * 16
    for tile in (32, 16):
        first, what = mref.plan_first(rows, hop, mp, tile)
        lds = (first + tile * (kp + 2)) * 4
        if lds <= mref.LDS_SOFT:
            break
    assert lds <= mref.LDS_MAX
    c = {mref.launch_of(tile, lds), what} | mref.shape_classes(nw, rows, hop, kp, n_mels)
    if mref.LDS_SOFT - 64 < lds <= mref.LDS_SOFT:
        c.add("edge-64k")
    return tile, (2 - hop) % 32, lds, c


def _e(win, hop, n_mels, rate, stream, channels=1, **options):
    return dict(dict(win_length=win, hop=hop, num_mel_bins=n_mels, sample_rate=rate, channels=channels, **options), stream=stream)


# the shapes whose launch forms no speech front end reaches; `stream` names one of test_gpu_clip_audio's, the rest are
# decode_clips_fbank's arguments.  (2, 1, 1) is left out on purpose: its single band has weight 0 on the only bin, so the
# definition has nothing to compare.
EDGES = {
    "taco-1024-256-80-stereo": _e(1024, 256, 80, 22050, "22k", 2),                # tile16-dyn, 52 512 B
    "551-220-80": _e(551, 220, 80, 22050, "22k"),                                 # 25 ms at 22.05 kHz, Nw odd
    "1024-450-last-dynamic": _e(1024, 450, 80, 22050, "48k"),
    "1024-451-first-static": _e(1024, 451, 80, 22050, "48k"),
    "900-hop4-exactly-64k": _e(900, 4, 80, 16000, "16k-mono"),
    "960-hop4-n-equals-nw-exactly-64k": _e(960, 4, 80, 16000, "16k-mono", round_to_power_of_two=False),
    "401-hop3-rectangular-rho-1": _e(401, 3, 20, 16000, "32k", window_type="rectangular", preemphasis_coefficient=1.0),
    "512-hop2-256-bands": _e(512, 2, 256, 16000, "32k", round_to_power_of_two=False),
    "551-hop3-256-bands-hamming": _e(551, 3, 256, 16000, "48k", window_type="hamming"),       # 59 968 B
    "18-hop1-5-bands-stereo": _e(18, 1, 5, 8000, "8k", 2, low_freq=0.0),
    # (one tap of the window is not 0: int16-scaled, as Kaldi's input is, so that a quiet stretch stays above the floors)
    "3-hop2-4-bands": _e(3, 2, 4, 8000, "8k", low_freq=0.0, scale=32768.0),
    "16-hop4-1-band": _e(16, 4, 1, 8000, "8k", low_freq=0.0, scale=32768.0),
    "64-hop5-15-bands": _e(64, 5, 15, 8000, "8k", low_freq=0.0, scale=32768.0),
    "64-hop5-17-bands-stereo": _e(64, 5, 17, 8000, "8k", 2, low_freq=0.0, scale=32768.0),
    "1024-hop1024-256-bands-own-rate": _e(1024, 1024, 256, 0, "44k-mono", round_to_power_of_two=False),
}
EXACT_EDGE = ("900-hop4-exactly-64k", "960-hop4-n-equals-nw-exactly-64k")
WITH_EVERYTHING = dict(use_energy=True, subtract_mean=True, htk_compat=True)
