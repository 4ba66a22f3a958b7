"""Log-mel features of clips (include/pdmp3_bulk.h) restated in binary64 with numpy alone: the window,
the DFT table, the mel filterbank, the samples a clip's frames read, the four output modes -- and the binary32 error bound
the tests hold the product to.  Nothing here is the product's code."""
import math

import numpy as np

U = 2.0 ** -24                                     # unit roundoff of binary32

# c: the largest error of the device's logf / log10f in units of u * max(1, |result|), plus one ulp (2 u at a result in
# [1, 2)).  ROCm's installed documentation gives no figure for them, so it was MEASURED on an MI355X with a program of its own
# (tools/ubench/logf_ulp.cpp: the two device functions against binary64, on the mode-0 values the GPU tests produce and on a
# sweep of every binade from the floor up) -- never from k_clip_mel.  profiles/clip_mel_tests.txt has the figure and its source.
LOG_C = 2.81 + 2.0

SCALES = {"slaney": 0, "htk": 1}


def window(n_fft):
    n = np.arange(n_fft, dtype=np.float64)
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * n / n_fft)


def dft_matrices(n_fft):
    """(cos, -sin) of 2 pi k n / N, [N, K], the angle reduced as the integer k n mod N; the window is not in them"""
    n = np.arange(n_fft, dtype=np.int64)[:, None]
    k = np.arange(n_fft // 2 + 1, dtype=np.int64)[None, :]
    a = 2.0 * np.pi * ((k * n) % n_fft).astype(np.float64) / n_fft
    return np.cos(a), -np.sin(a)


def dft_table(n_fft):
    """the product's table layout in binary64: [N rounded up to 4, 2 Kp], window folded in, zeros in the padding"""
    K = n_fft // 2 + 1
    Kp = (K + 15) // 16 * 16
    rows = (n_fft + 3) // 4 * 4
    c, s = dft_matrices(n_fft)
    w = window(n_fft)[:, None]
    t = np.zeros((rows, 2 * Kp), dtype=np.float64)
    t[:n_fft, :K] = w * c
    t[:n_fft, Kp:Kp + K] = w * s
    return t


def hz_to_mel(f, htk):
    if htk:
        return 2595.0 * math.log10(1.0 + f / 700.0)
    return 3.0 * f / 200.0 if f < 1000.0 else 15.0 + 27.0 * math.log(f / 1000.0) / math.log(6.4)


def mel_to_hz(m, htk):
    if htk:
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    return 200.0 * m / 3.0 if m < 15.0 else 1000.0 * math.exp(math.log(6.4) * (m - 15.0) / 27.0)


def filterbank(sr, n_fft, n_mels, f_min=0.0, f_max=0.0, scale="slaney", norm="slaney"):
    """W[m, k] in binary64, [n_mels, K]"""
    htk = SCALES[scale] if isinstance(scale, str) else int(scale)
    if not f_max:
        f_max = sr / 2.0
    m0, m1 = hz_to_mel(f_min, htk), hz_to_mel(f_max, htk)
    f = [mel_to_hz(m0 + (m1 - m0) * i / (n_mels + 1), htk) for i in range(n_mels + 2)]
    f[0], f[-1] = float(f_min), float(f_max)
    K = n_fft // 2 + 1
    fk = np.arange(K, dtype=np.float64) * sr / n_fft
    w = np.zeros((n_mels, K), dtype=np.float64)
    for m in range(n_mels):
        up = (fk - f[m]) / (f[m + 1] - f[m])
        down = (f[m + 2] - fk) / (f[m + 2] - f[m + 1])
        w[m] = np.maximum(0.0, np.minimum(up, down))
        if norm in ("slaney", 1):
            w[m] *= 2.0 / (f[m + 2] - f[m])
    return w


def span(n_fft, hop, start, n_frames):
    return start - n_fft // 2, ((n_frames - 1) * hop + n_fft if n_frames else 0)


def valid(n_out, start, hop, n_frames):
    left = n_out - start
    return 0 if left <= 0 else min(-(-left // hop), n_frames)


def frames_of(y, pos0, start, n_frames, n_fft, hop):
    """y[t] is the signal at position pos0 + t (0.0 everywhere else) -> [n_frames, N] binary64"""
    y = np.asarray(y, dtype=np.float64)
    idx = (start - n_fft // 2 - pos0) + np.arange(n_frames, dtype=np.int64)[:, None] * hop + np.arange(n_fft, dtype=np.int64)[None, :]
    ok = (idx >= 0) & (idx < y.size)
    return np.where(ok, y[np.clip(idx, 0, max(y.size - 1, 0))] if y.size else 0.0, 0.0)


def _log_term(m, dm, out, base, floor):
    return dm / (math.log(base) * np.maximum(m - dm, floor)) + LOG_C * U * np.maximum(1.0, np.abs(out))


def mel(y, pos0, start, n_frames, n_fft, hop, w, mode, floor):
    """y: [C, T] binary32 values of the signal from position pos0 on.  -> (out, bound), both binary64 [C, n_mels, n_frames]:
    the definition on those values, and what a binary32 evaluation may differ from it by:
      E  = (N + 2) u A,  A = sum |w y| of the frame                      (Re, Im: dot products of length N)
      dP = 2 (|Re| + |Im|) E + 2 E^2 + (2 u + u^2) (P + 2 (|Re| + |Im|) E + 2 E^2)
      dM = W dP + (K_m + 2) u W (P + dP),  K_m = the non-zero weights of row m
      logs: dM / (ln b max(M - dM, floor)) + c u max(1, |out|);  mode 3: see below"""
    y = np.atleast_2d(np.asarray(y, dtype=np.float64))
    floor = float(np.float32(floor))
    win = window(n_fft)
    c, s = dft_matrices(n_fft)
    km = (w > 0).sum(axis=1).astype(np.float64)[:, None]
    outs, bounds, ms, dms = [], [], [], []
    for ch in range(y.shape[0]):
        fr = frames_of(y[ch], pos0, start, n_frames, n_fft, hop) * win[None, :]
        re, im = fr @ c, fr @ s
        p = re * re + im * im                                               # [F, K]
        e = ((n_fft + 2) * U * np.abs(fr).sum(axis=1))[:, None]
        cross = 2.0 * (np.abs(re) + np.abs(im)) * e + 2.0 * e * e
        dp = cross + (2.0 * U + U * U) * (p + cross)
        m = w @ p.T                                                         # [n_mels, F]
        dm = w @ dp.T + (km + 2.0) * U * (w @ (p + dp).T)
        ms.append(m)
        dms.append(dm)
    m, dm = np.stack(ms), np.stack(dms)
    if mode == 0:
        return m, dm
    if mode in (1, 2):
        base = math.e if mode == 1 else 10.0
        out = np.log(np.maximum(m, floor)) / (1.0 if mode == 1 else math.log(10.0))
        return out, _log_term(m, dm, out, base, floor)
    # mode 3: l = log10 max(M, floor), g = log10 max(max M, floor); max is 1-Lipschitz, so g's error is at most the largest
    # of the row's log terms; then a = fl(g - 8): + u (|g| + 8); v = max(l, a); fl(v + 4): + u |v + 4|; / 4 is exact
    l = np.log10(np.maximum(m, floor))
    tl = _log_term(m, dm, l, 10.0, floor)
    g = float(l.max()) if l.size else math.log10(floor)
    tg = (float(tl.max()) if tl.size else 0.0) + U * (abs(g) + 8.0)
    v = np.maximum(l, g - 8.0)
    out = (v + 4.0) / 4.0
    bound = (np.maximum(tl, tg) + U * np.abs(v + 4.0)) / 4.0 * (1.0 + 4.0 * U)
    return out, bound
