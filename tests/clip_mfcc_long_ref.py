"""The binary64 definition of decode_clips_mfcc_long and its derived bounds, evaluated per value: the dB
mel in numpy float32 (bit for bit the call's), the orthonormal DCT-II with librosa's lifter, the delta stencils.  u = 2^-24."""
import numpy as np

U = 2.0 ** -24
U64 = 2.0 ** -53
TINY = 2.0 ** -150                      # half the smallest denormal binary32: a result's rounding down there
MODES = ("mfcc", "db")


def halo(deltas, delta_width, out_mode="mfcc"):
    return (delta_width - 1) // 2 if deltas > 0 and out_mode == "mfcc" else 0


def valid(j_all, start, hop, f):
    """the frames of the clip (start, f) whose centres lie inside the stream's j_all samples"""
    left = j_all - start
    return 0 if left <= 0 else min(f, (left + hop - 1) // hop)


def db(l, top_db, h=0):
    """l: float32 [n_mels, F + 2 h] log10 mel -> float32 d of the same shape; the maximum is taken over the columns h .. h + F - 1.
    Every step is one binary32 operation."""
    l = np.asarray(l, dtype=np.float32)
    d0 = np.float32(10.0) * l
    assert d0.dtype == np.float32
    if top_db is None:
        return d0
    own = d0[:, h:d0.shape[1] - h] if h else d0
    thr = np.float32(own.max()) - np.float32(top_db)
    assert type(thr) is np.float32
    return np.maximum(d0, thr)


def dct(n_mels, n_mfcc, lifter=0.0):
    """T [n_mfcc, n_mels] in binary64"""
    q = np.arange(n_mfcc, dtype=np.float64)[:, None]
    m = np.arange(n_mels, dtype=np.float64)[None, :]
    t = np.cos(np.pi * q * (2.0 * m + 1.0) / (2.0 * n_mels)) * np.sqrt(2.0 / n_mels)
    t[0] = np.sqrt(1.0 / n_mels)
    if lifter > 0:
        t = t * (1.0 + (lifter / 2.0) * np.sin(np.pi * (q + 1.0) / lifter))
    return t


def cepstra(d, n_mfcc, lifter=0.0):
    """d: float32 [n_mels, cols] -> (c = T d in binary64 [n_mfcc, cols], its bound): one rounding of the table's entry, one of
    every product-and-sum of the chain of n_mels fused multiply-adds, first order (n_mels + 1) u A; (n_mels + 2) u A covers the
    higher orders for n_mels <= 256 and a denormal result's rounding"""
    d = np.asarray(d, dtype=np.float32).astype(np.float64)
    t = dct(d.shape[0], n_mfcc, lifter)
    return t @ d, (d.shape[0] + 2) * U * (np.abs(t) @ np.abs(d)) + TINY


def taps(w):
    """[2, w] binary64: the first and the second delta's taps, j = -h .. h"""
    h = (w - 1) // 2
    j = np.arange(-h, h + 1, dtype=np.float64)
    s2, s4 = float((j ** 2).sum()), float((j ** 4).sum())
    return np.stack([j / s2, 2.0 * (j ** 2 - s2 / w) / (s4 - s2 * s2 / w)])


def delta(c, w, order):
    """c: [n, F + w - 1] (float32 values or binary64) -> (the stencil in binary64 [n, F], sum_j |tap_j| |c| [n, F])"""
    c = np.asarray(c).astype(np.float64)
    t = taps(w)[order - 1]
    f = c.shape[1] - (w - 1)
    win = np.stack([c[:, j:j + f] for j in range(w)])                 # [w, n, F]
    return np.tensordot(t, win, axes=1), np.tensordot(np.abs(t), np.abs(win), axes=1)


def delta_bound(want, mass, w):
    """the kernel's own error on its binary32 c: a chain of w binary64 fused multiply-adds on binary64 taps, rounded once"""
    return U * np.abs(want) + (w + 1) * U64 * mass + TINY


def delta_chain_bound(bound_c, w, order):
    """c's bound carried through the taps: sum_j |tap_j| bound_c[q, t + j]"""
    t = np.abs(taps(w)[order - 1])
    f = bound_c.shape[1] - (w - 1)
    return np.tensordot(t, np.stack([bound_c[:, j:j + f] for j in range(w)]), axes=1)


def plan(n_mels, n_mfcc, deltas, delta_width, out_mode="mfcc"):
    """pdmp3_amd_mfcc_long_plan restated: (front, back, tile, d_pitch, c_pitch, lds_bytes)"""
    if out_mode == "db":
        return 0, 0, 1024, 0, 0, 0
    h = halo(deltas, delta_width)
    m16, c16 = (n_mels + 15) // 16 * 16, (n_mfcc + 15) // 16 * 16
    return h, h, 64, 80, 84, (m16 * 80 + c16 * 84) * 4


def mfcc(l, n_mfcc, lifter, top_db, deltas, w, f):
    """the full chain from the widened clip's log-mel l [n_mels, f + 2 h] -> (rows [(1 + deltas) n_mfcc, f] in binary64, their
    bound): c against T d, the deltas with c's bound carried through the taps plus the stencil's own term"""
    h = halo(deltas, w)
    d = db(l, top_db, h)
    c, bc = cepstra(d, n_mfcc, lifter)
    rows, bounds = [c[:, h:h + f]], [bc[:, h:h + f]]
    for order in range(1, deltas + 1):
        want, mass = delta(c, w, order)
        rows.append(want)
        chain = delta_chain_bound(bc, w, order)          # (the kernel's c differs from T d by at most bc: so do its stencil and mass)
        bounds.append(chain + delta_bound(np.abs(want) + chain, mass + chain, w))
    return np.concatenate(rows), np.concatenate(bounds)
