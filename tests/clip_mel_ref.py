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


# ---- the plan of a workgroup of k_clip_mel restated, and the classes of a geometry ("launch forms") ----
LDS_SOFT = 64 * 1024                               # a dynamic request ends here; above it the static-array kernel
LDS_MAX = 160 * 1024 - 64
ODD_BANDS = (1, 15, 17, 256)


def plan_first(rows, hop, n_bands16, tile):
    """the first LDS region of a tile: (floats, "span" or "mel-tile") -- the span in chunks of hop + row_pad floats, or the mel
    tile [bands16][tile + 1] where that is larger, rounded up to 4 floats"""
    pad = (2 - hop) % 32
    span = -(-((tile - 1) * hop + rows) // hop) * (hop + pad)
    mt = n_bands16 * (tile + 1)
    return (max(span, mt) + 3) // 4 * 4, "mel-tile" if mt > span else "span"


def launch_of(tile, lds):
    return "tile32" if tile == 32 else "tile16-dyn" if lds <= LDS_SOFT else "tile16-static"


def shape_classes(n, rows, hop, bins16, n_bands=None):
    """what the lane walk, the row padding, the DFT stage's waves and the band count add to a form's classes"""
    c = set()
    if hop < 4:
        c.add("hop<4")
    if rows != n:
        c.add("rows-padded")
    if bins16 // 16 < 4:
        c.add("idle-waves")
    if n_bands in ODD_BANDS:
        c.add("bands-%d" % n_bands)
    return c


def form(n_fft, hop, n_mels):
    """-> (tile, row_pad, lds_bytes, classes): 32 frames where their LDS fits 64 KB, else 16; the classes are the launch form,
    what sizes the first region, and shape_classes()"""
    rows, kp, mp = (n_fft + 3) // 4 * 4, (n_fft // 2 + 1 + 15) // 16 * 16, (n_mels + 15) // 16 * 16
    for tile in (32, 16):
        first, what = plan_first(rows, hop, mp, tile)
        lds = (first + tile * (kp + 2)) * 4
        if lds <= LDS_SOFT:
            break
    assert lds <= LDS_MAX
    c = {launch_of(tile, lds), what} | shape_classes(n_fft, rows, hop, kp, n_mels)
    if LDS_SOFT - 64 < lds <= LDS_SOFT:
        c.add("edge-64k")
    return tile, (2 - hop) % 32, lds, c


def _e(n_fft, hop, n_mels, rate, stream, channels=1, scale="slaney", norm="slaney"):
    return dict(n_fft=n_fft, hop=hop, n_mels=n_mels, sample_rate=rate, stream=stream, channels=channels, scale=scale, norm=norm)


# the shapes whose launch forms no speech front end reaches; `stream` names one of test_gpu_clip_audio's
EDGES = {
    "taco-1024-256-80-stereo": _e(1024, 256, 80, 22050, "22k", 2),                # tile16-dyn: the Tacotron / HiFi-GAN front end
    "1024-418-last-dynamic": _e(1024, 418, 80, 22050, "48k"),
    "1024-419-first-static": _e(1024, 419, 80, 22050, "48k"),
    "1024-hop3-static": _e(1024, 3, 80, 16000, "32k"),                            # chunks of 34 floats: 82 480 B
    "1024-hop4-static": _e(1024, 4, 80, 16000, "32k"),
    "958-hop4-exactly-64k": _e(958, 4, 80, 16000, "16k-mono"),
    "806-hop3-16-bands": _e(806, 3, 16, 16000, "16k-mono", scale="htk"),
    "512-hop2-256-bands": _e(512, 2, 256, 16000, "32k"),                          # first region: the mel tile
    "64-hop1-256-bands": _e(64, 1, 256, 8000, "8k", scale="htk", norm=None),
    "16-hop16-256-bands-stereo": _e(16, 16, 256, 8000, "8k", 2),
    "16-hop1-1-band": _e(16, 1, 1, 8000, "8k"),
    "398-hop3-20-bands": _e(398, 3, 20, 16000, "48k", scale="htk", norm=None),
    "1022-hop1-17-bands-own-rate": _e(1022, 1, 17, 0, "44k-mono"),
    "18-hop5-15-bands": _e(18, 5, 15, 16000, "16k-mono"),
}
EXACT_EDGE = ("958-hop4-exactly-64k",)
