"""The definitions of clips as float batches (include/pdmp3_bulk.h) restated in binary64 with numpy alone
-- independent of the library's table builder and of the kernel: Python / int64 integers for n L - j M, everything else float64.
Used by test_clip_audio_host.py, test_gpu_clip_audio.py and test_gpu_clip_audio_paths.py."""
from math import gcd

import numpy as np

RATES = [44100, 48000, 32000, 22050, 24000, 16000, 11025, 12000, 8000]


def ratio(rate_in, rate_out):
    g = gcd(rate_in, rate_out)
    return rate_in // g, rate_out // g               # M, L


def out_length(n_in, rate_in, rate_out):
    m, l = ratio(rate_in, rate_out)
    return -((-n_in * l) // m)                       # J = ceil(N L / M)


def taps(rate_in, rate_out, width, rolloff, js):
    """for output samples js (int64 array): (n [len(js), D] input sample numbers, h [len(js), D] float64, inside [len(js), D]
    bool: |u| < Z) -- every n with |u(n, j)| < Z is among them"""
    m, l = ratio(rate_in, rate_out)
    s = max(l, m)
    dmax = int(width * s / rolloff) // l + 2
    d = np.arange(-dmax, dmax + 1, dtype=np.int64)
    jm = np.asarray(js, dtype=np.int64) * m
    q, r = jm // l, jm % l
    t = d[None, :] * l - r[:, None]                  # n L - j M, exact
    u = rolloff * t.astype(np.float64) / s
    inside = np.abs(u) < width
    h = rolloff * min(l, m) / m * np.sinc(u) * np.cos(np.pi * u / (2.0 * width)) ** 2
    h[~inside] = 0.0
    assert not inside[:, 0].any() and not inside[:, -1].any()
    return q[:, None] + d[None, :], h, inside


def resample64(x, rate_in, rate_out, width, rolloff, start, count):
    """x: float64 [C, N] (the stream on its time line) -> (y64 [C, count], bound [C, count]): output samples start .. start +
    count of the definition, zeros from J on, and the bound (T_j + 2) 2^-24 sum |h| |x| of a binary32 evaluation"""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    c, n_in = x.shape
    y = np.zeros((c, count))
    bound = np.zeros((c, count))
    j_end = min(start + count, out_length(n_in, rate_in, rate_out))
    if rate_in == rate_out:
        if j_end > start:
            y[:, :j_end - start] = x[:, start:j_end]
        return y, bound
    m, l = ratio(rate_in, rate_out)
    step = max(1, min(4096, (1 << 23) // (2 * (int(width * max(l, m) / rolloff) // l + 2) + 1)))   # (rows a pass: 64 MB an array at most)
    for a in range(start, j_end, step):
        js = np.arange(a, min(a + step, j_end), dtype=np.int64)
        n, h, inside = taps(rate_in, rate_out, width, rolloff, js)
        ok = (n >= 0) & (n < n_in)
        xv = np.where(ok[None], x[:, np.clip(n, 0, max(n_in - 1, 0))], 0.0) if n_in else np.zeros((c,) + n.shape)
        y[:, a - start:a - start + len(js)] = (h[None] * xv).sum(axis=2)
        bound[:, a - start:a - start + len(js)] = (inside.sum(axis=1) + 2)[None] * 2.0 ** -24 * (np.abs(h)[None] * np.abs(xv)).sum(axis=2)
    return y, bound


LDS_X, LDS_TABLE, TILE, LDS_BYTES = 1, 2, 1024, 64 * 1024    # include/pdmp3_hip.h PDMP3_AUDIO_*

# (in, out, Z, rolloff) with output rates that are no MPEG rates: tables of tens of thousands of rows, of one row, of thousands
# of taps -- all three LDS plans among them (test_clip_audio_host.py pins which)
ODD_PAIRS = [(44100, 44099, 6, 0.99), (48000, 47999, 6, 0.99), (8000, 44101, 6, 0.99), (44100, 22051, 6, 0.99), (32000, 96000, 6, 0.99),
             (8000, 192000, 16, 0.99), (11025, 48000, 64, 0.99), (44100, 8000, 64, 0.99), (48000, 4000, 64, 0.5), (48000, 1000, 6, 0.99),
             (44100, 100, 6, 0.99), (22050, 7, 1, 1.0)]


def lds_plan(m, l, taps, channels):
    """pdmp3_amd/host/clip_features.c audio_lds restated: (flags, span_cap) of a clip with the ratio M : L and `taps` coefficients a row in a
    call with `channels` channels -- the input span of a tile in LDS if it fits 64 KB, the table behind it if that fits too"""
    span = ((l - 1) + (TILE - 1) * m) // l + taps
    cap = (span + 3) & ~3
    if cap * channels * 4 > LDS_BYTES:
        return 0, 0
    flags = LDS_X
    if cap * channels * 4 + ((l * taps + 3) & ~3) * 4 <= LDS_BYTES:
        flags |= LDS_TABLE
    return flags, cap


def timeline(whole, pcm_offsets, spf, stereo):
    """the whole-stream interleaved int16 output -> int64 [2, N]: l, r per sample of the time line (a mono frame's samples in both)"""
    frames = len(pcm_offsets) - 1
    out = np.zeros((2, frames * spf), dtype=np.int64)
    size = np.diff(pcm_offsets) // 2                 # int16 values per frame
    for f in range(frames):
        v = whole[pcm_offsets[f] // 2:pcm_offsets[f] // 2 + size[f]].astype(np.int64)
        if size[f] == spf:
            out[0, f * spf:(f + 1) * spf] = out[1, f * spf:(f + 1) * spf] = v
        else:
            assert size[f] == 2 * spf
            out[0, f * spf:(f + 1) * spf] = v[0::2]
            out[1, f * spf:(f + 1) * spf] = v[1::2]
    return out if stereo else out[:1]


def channels64(lr, stream_channels, channels):
    """int64 [Cs, N] -> float64 [C, N] by the channel rules (exact: the values are k / 65536 with |k| < 2^17)"""
    if stream_channels == 2 and channels == 1:
        return ((lr[0] + lr[1]) / 65536.0)[None]
    if stream_channels == 1 and channels == 2:
        return np.stack([lr[0], lr[0]]) / 32768.0
    return lr / 32768.0
