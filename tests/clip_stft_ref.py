"""The short-time Fourier transform of clips (include/pdmp3_bulk.h) restated in binary64 with numpy
alone: the frame's window, the folded table, the five output modes -- and the binary32 error bound the tests hold the product
to.  Nothing here is the product's code; tests/test_clip_stft_host.py holds it against torch.stft in float64.

Definition, step by step.
  1. Signal.  y[j] is the binary32 output of the audio call at the requested rate for 0 <= j < J, 0.0 outside.
  2. Frame f of a clip at `start` reads y[start + f H - N / 2 + n], 0 <= n < N (clip_mel_ref.frames_of: the same framing).
  3. Window.  Nw = win_length (0 / None: N) values -- the caller's binary32 ones, or periodic Hann 0.5 - 0.5 cos(2 pi i / Nw)
     -- at n = (N - Nw) // 2 + i, zeros elsewhere.
  4. X[f, k] = s sum_n w[n] y[..] e^(-2 pi i k n / N), k < N / 2 + 1, s = N^(-1/2) with `normalized`, else 1; the angle is
     reduced as the integer k n mod N.
  5. Modes: 0 (Re, Im); 1 sqrt(Re^2 + Im^2); 2 P = Re^2 + Im^2; 3 ln max(P, floor); 4 log10 max(P, floor); floor rounded to
     binary32 first.

The bound (u = 2^-24), derived as DESIGN.md section 10's:
  E  = (N + 2) u A,  A = sum_n |s w[n] y[n]| of the frame: a binary32 dot product of length N -- the N roundings of the fused
       multiply-add chain, the one rounding of a coefficient (s and w are inside it), one u for the second-order terms:
       section 10's E with the scale inside A.
  mode 0: E for Re and for Im.
  mode 2: dP = 2 (|Re| + |Im|) E + 2 E^2 + (2 u + u^2) (P + 2 (|Re| + |Im|) E + 2 E^2): the computed pair (a, b) lies within E
       of (Re, Im) in each component, and fl(a^2 + b^2) as the product takes it -- b b + fl(a a), one fused step -- is
       (a^2 + b^2)(1 + t), |t| <= 2 u + u^2 =: T.
  mode 1: with Q = a^2 + b^2 exactly, the stored value is sqrt(Q (1 + t)) (1 + d), |d| <= u (a correctly rounded square
       root).  |sqrt(Q) - |X|| <= hypot(E, E) = sqrt(2) E (the pair as a vector: the triangle inequality), and
       |sqrt(1 + t) - 1| = |t| / (1 + sqrt(1 + t)) <= T / (2 - T) =: g, so
           |stored - |X|| <= sqrt(2) E + (|X| + sqrt(2) E) ((1 + g)(1 + u) - 1).
       Nothing is divided by the magnitude: the bound is finite, and 0 on silence.
  modes 3, 4: clip_mel_ref._log_term on (P, dP): dP / (ln b max(P - dP, floor)) + LOG_C u max(1, |out|), with the project's
       measured LOG_C (profiles/clip_mel_tests.txt).  No new measured constant: the square root is correctly rounded
       (profiles/clip_stft_tests.txt)."""
import math

import numpy as np

import clip_mel_ref as mref

U = mref.U
LOG_C = mref.LOG_C
MODES = {"complex": 0, "magnitude": 1, "power": 2, "log": 3, "log10": 4}
T2 = 2.0 * U + U * U
SQRT_C = (1.0 + T2 / (2.0 - T2)) * (1.0 + U) - 1.0        # mode 1's relative part: about 2 u


def frame_window(n_fft, win_length=None, window=None):
    """w[n], binary64 [N]: the caller's binary32 values (or periodic Hann of Nw) centred in N as torch.stft centres them"""
    nw = int(win_length) if win_length else n_fft
    if window is None:
        i = np.arange(nw, dtype=np.float64)
        w = 0.5 - 0.5 * np.cos(2.0 * np.pi * i / nw)
    else:
        w = np.asarray(window, dtype=np.float32).astype(np.float64)
        assert w.shape == (nw,)
    out = np.zeros(n_fft, dtype=np.float64)
    left = (n_fft - nw) // 2
    out[left:left + nw] = w
    return out


def scale(n_fft, normalized):
    return 1.0 / math.sqrt(n_fft) if normalized else 1.0


def table(n_fft, win_length=None, window=None, normalized=False):
    """the product's table layout in binary64: [N rounded up to 4, 2 Kp], s w[n] cos and -s w[n] sin, zeros in the padding"""
    K = n_fft // 2 + 1
    Kp = (K + 15) // 16 * 16
    rows = (n_fft + 3) // 4 * 4
    c, s = mref.dft_matrices(n_fft)
    w = (scale(n_fft, normalized) * frame_window(n_fft, win_length, window))[:, None]
    t = np.zeros((rows, 2 * Kp), dtype=np.float64)
    t[:n_fft, :K] = w * c
    t[:n_fft, Kp:Kp + K] = w * s
    return t


valid = mref.valid
frames_of = mref.frames_of


def tile_plan(n_fft, hop, mode):
    """the plan of a workgroup of k_clip_stft restated: (tile, row_pad, lds_bytes, launch path)"""
    rows = (n_fft + 3) // 4 * 4
    pad = (2 - hop) % 32

    def lds(tile):
        span = (tile - 1) * hop + rows
        a = (-(-span // hop) * (hop + pad) + 3) // 4 * 4
        return (a + 4 * (2 if mode == 0 else 1) * 16 * (tile + 4)) * 4
    if lds(32) <= 64 * 1024:
        return 32, pad, lds(32), "tile32"
    return 16, pad, lds(16), "tile16" if lds(16) <= 64 * 1024 else "tile16-static"


def stft(y, pos0, start, n_frames, n_fft, hop, mode, floor=1e-10, win_length=None, window=None, normalized=False):
    """y: [C, T] binary32 values of the signal from position pos0 on.  -> (out, bound), binary64: mode 0 [C, K, F, 2], else
    [C, K, F]: the definition on those values, and what a binary32 evaluation may differ from it by (the module's docstring)"""
    y = np.atleast_2d(np.asarray(y, dtype=np.float64))
    floor = float(np.float32(floor))
    w = scale(n_fft, normalized) * frame_window(n_fft, win_length, window)
    c, s = mref.dft_matrices(n_fft)
    outs, bounds = [], []
    for ch in range(y.shape[0]):
        fr = frames_of(y[ch], pos0, start, n_frames, n_fft, hop) * w[None, :]
        re, im = (fr @ c).T, (fr @ s).T                                     # [K, F]
        e = np.broadcast_to(((n_fft + 2) * U * np.abs(fr).sum(axis=1))[None, :], re.shape)
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


def power_as_the_product(re, im):
    """mel_power on binary32 (Re, Im) -> binary32, bit for bit: fma(im, im, fl(re re)).  In binary64 fl(re re) and im im (48
    bits) are exact; their sum is rounded to binary64 and then to binary32, which differs from the fused step's one rounding
    only where the binary64 sum is inexact AND lies on a binary32 tie (or below binary32's normal range): those few are
    decided with exact rational arithmetic."""
    from fractions import Fraction
    re = np.asarray(re, dtype=np.float32)
    im = np.asarray(im, dtype=np.float32)
    a = (re * re).astype(np.float64)
    b = im.astype(np.float64) * im.astype(np.float64)
    s = a + b
    out = np.ascontiguousarray(s.astype(np.float32))
    inexact = ((s - a) != b) | ((s - b) != a)
    tie = (np.ascontiguousarray(s).view(np.uint64) & np.uint64(0x1fffffff)) == np.uint64(0x10000000)
    flat_a, flat_b, flat_o = a.ravel(), b.ravel(), out.reshape(-1)
    for i in np.flatnonzero((inexact & (tie | (s < 2.0 ** -125))).ravel()):
        x = Fraction(float(flat_a[i])) + Fraction(float(flat_b[i]))
        near = (np.nextafter(flat_o[i], np.float32(-np.inf)), flat_o[i], np.nextafter(flat_o[i], np.float32(np.inf)))
        flat_o[i] = min(near, key=lambda v: (abs(Fraction(float(v)) - x), int(np.float32(v).view(np.uint32)) & 1))
    return out


# ---- the classes of a geometry of k_clip_stft ("launch forms"); the plan itself is tile_plan() above ----
def form(n_fft, hop, mode):
    """-> (tile, row_pad, lds_bytes, classes): tile_plan's launch path under the names the other feature kernels' forms have,
    and clip_mel_ref.shape_classes()"""
    tile, pad, lds, path = tile_plan(n_fft, hop, mode)
    c = {"tile16-dyn" if path == "tile16" else path} | mref.shape_classes(n_fft, (n_fft + 3) // 4 * 4, hop, (n_fft // 2 + 1 + 15) // 16 * 16)
    if mref.LDS_SOFT - 64 < lds <= mref.LDS_SOFT:
        c.add("edge-64k")
    return tile, pad, lds, c


def _edge_window(nw):
    return (np.random.default_rng(nw).random(nw, dtype=np.float32) * np.float32(1.5) - np.float32(0.25)).astype(np.float32)


def _e(n_fft, hop, rate, stream, channels=1, modes=("complex",), **options):
    return dict(dict(n_fft=n_fft, hop=hop, sample_rate=rate, channels=channels, **options), stream=stream, modes=modes)


ALL_MODES = tuple(MODES)
# the shapes whose launch forms no speech front end reaches; `stream` names one of test_gpu_clip_audio's, `modes` the modes whose
# launch form the shape is there for (the device test runs all five), the rest are decode_clips_stft's arguments
EDGES = {
    "1024-352-stereo-two-forms": _e(1024, 352, 22050, "22k", 2, ALL_MODES),       # mode 0: tile 16; modes 1 - 4: tile 32
    "1024-322-last-tile32": _e(1024, 322, 22050, "48k"),
    "1024-323-first-tile16": _e(1024, 323, 22050, "48k"),
    "1024-802-last-dynamic": _e(1024, 802, 0, "48k"),
    "1024-803-first-static": _e(1024, 803, 0, "48k"),
    "1024-386-power-last-tile32": _e(1024, 386, 22050, "48k", modes=("power",)),
    "1024-387-power-first-tile16": _e(1024, 387, 22050, "48k", modes=("power",)),
    "1024-866-power-last-dynamic": _e(1024, 866, 0, "48k", modes=("power",)),
    "1024-867-power-first-static": _e(1024, 867, 0, "48k", modes=("power",)),
    "1024-256-stereo": _e(1024, 256, 22050, "22k", 2),                            # 54 560 B, a large tile 32
    "944-hop3-64k": _e(944, 3, 16000, "16k-mono"),                                # 65 488 B
    "1022-hop2-normalized": _e(1022, 2, 16000, "32k", normalized=True),
    "398-hop3-own-window": _e(398, 3, 16000, "32k", window=_edge_window(398)),
    "1024-700-window-1000": _e(1024, 700, 0, "44k-mono", win_length=1000, window=_edge_window(1000)),
}
EXACT_EDGE = ("944-hop3-64k",)
