"""Onset strength, tempogram and tempo of clips (include/pdmp3_bulk.h pdmp3_amd_tempogram_*) restated with
numpy alone: the definition's steps 2-7 in binary64 on binary32 inputs, the plan of the launches -- and the bounds the tests
hold the product to.  Nothing here is the product's code.

The bounds (u = 2^-24, v = 2^-53):
  onset      o^ is one binary32 rounding of a binary64 sum over the bands ascending: |o^ - o| <= u |o| + (n_mels + 2) v |o| + 2^-149.
             Against the full chain: l^ within dl of l in both frames, max(0, .) and the band maximum 1-Lipschitz, so
             (10 / n_mels) sum_m (dl[m][f] + max over the neighbourhood of dl[.][f - lag]) on top of it.
  tempogram  n = 4 ceil((Wt + 15) / 4) fused steps a lag, g = n u / (1 - n u): |r^(tau) - r(tau)| <= g sum |x x| <= g r(0)
             (Cauchy-Schwarz), r^(0) = r(0) (1 + d), |d| <= g.  T^ = fl32(fl64(r^(tau) / r^(0))):
             |T^ - T| <= B = g (|T| + 1) / (1 - g) + (u + v) (|T| + g (|T| + 1) / (1 - g)) + 2^-149, at most about 2 g + u whatever
             the signal's level; where r(0) > 0 the underflow of the products adds n 2^-149 / r(0).
  tempo      s is monotone in A: |s^ - s| <= S = max(log1p(1e6 (A + dA)) - s0, s0 - log1p(1e6 max(A - dA, 0))) + 4 v (1 + |s|), s0 =
             log1p(1e6 A), at most 1e6 dA.  On mode 1's own output dA = (F + 2) v A (the same sum in the same order).  A clip is
             decided where the reference's margin exceeds 2 max S: there tau* and bpm are exact.  Elsewhere the device's tau*
             has s within 2 max S of the maximum."""
import math

import numpy as np

U = 2.0 ** -24
V = 2.0 ** -53
TINY = 2.0 ** -149
LDS_MAX = 160 * 1024 - 64


# ---- the planning calls ----
def window(wt):
    n = np.arange(wt, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * n / wt)).astype(np.float32)


def prior(sr, hop, wt, start_bpm=120.0, std_bpm=1.0, max_tempo=320.0):
    """-> (binary64 [wt], the smallest admissible lag or 0)"""
    p = np.full(wt, -np.inf)
    for tau in range(1, wt):
        bpm = 60.0 * sr / (float(hop) * tau)
        if bpm < max_tempo:
            z = (math.log2(bpm) - math.log2(start_bpm)) / std_bpm
            p[tau] = -0.5 * (z * z)
    ok = np.flatnonzero(np.isfinite(p))
    return p, (int(ok[0]) if ok.size else 0)


def plan(lag, wt, mode):
    """-> (front, back, tiles, ksteps, frames of a workgroup, LDS bytes)"""
    tiles, ksteps = (wt + 255) // 256, (wt + 18) // 4
    reach = 4 * (ksteps + 1) + 240 + 256 * (tiles - 1)
    ext = 16 + max(reach, wt)
    span = (ext + 2 * (ext >> 4) + 3) & ~3
    for frames in (8, 4, 2, 1):
        lds = (frames * (span + 256 * tiles + 8) * 4 + 15) & ~15
        if lds <= LDS_MAX:
            break
    front, back = (lag, 0) if mode == 0 else (lag + wt // 2, wt // 2 - 1)
    return front, back, tiles, ksteps, frames, lds


def geometry(wt, frames):
    """-> (ext, span floats) of a wave of k_clip_tempogram"""
    tiles, ksteps = (wt + 255) // 256, (wt + 18) // 4
    ext = 16 + max(4 * (ksteps + 1) + 240 + 256 * (tiles - 1), wt)
    return ext, (ext + 2 * (ext >> 4) + 3) & ~3


def valid(j_all, start, hop, f):
    left = j_all - start
    return 0 if left <= 0 else min((left + hop - 1) // hop, f)


# ---- steps 2 and 3 ----
def band_max(x, max_size):
    """x [n_mels, ..] -> the maximum over |m' - m| <= (max_size - 1) / 2, m' clamped"""
    h, nm = (max_size - 1) // 2, x.shape[0]
    out = x.copy()
    for d in range(1, h + 1):
        for sgn in (-1, 1):
            idx = np.clip(np.arange(nm) + sgn * d, 0, nm - 1)
            out = np.maximum(out, x[idx])
    return out


def onset(l, lag, max_size):
    """l: [n_mels, Fm] binary32 log-mel, column e + lag the frame of envelope value e -> (o [Fm - lag] binary64, its bound as one
    rounding of that sum)"""
    l = np.asarray(l, dtype=np.float64)
    nm = l.shape[0]
    d = np.maximum(0.0, l[:, lag:] - band_max(l, max_size)[:, :l.shape[1] - lag])
    o = (10.0 / nm) * np.cumsum(d, axis=0)[-1]             # (ascending in m, as the definition sums)
    return o, U * np.abs(o) + (nm + 2) * V * np.abs(o) + TINY


def onset_chain_bound(dl, lag, max_size):
    """dl [n_mels, Fm]: what every log-mel value may differ from the definition's by -> what that adds to the bound of o"""
    dl = np.asarray(dl, dtype=np.float64)
    return (10.0 / dl.shape[0]) * (dl[:, lag:] + band_max(dl, max_size)[:, :dl.shape[1] - lag]).sum(axis=0)


# ---- steps 4 and 5 ----
def frames_of(o32, wt, f):
    """the binary32 envelope [f + wt - 1] (value e is o[e - wt / 2]) -> x [f, wt] binary32: one product a sample"""
    o32 = np.asarray(o32, dtype=np.float32)
    assert o32.size == f + wt - 1
    w = window(wt)
    idx = np.arange(f)[:, None] + np.arange(wt)[None, :]
    return w[None, :] * o32[idx]


def autocorrelation(x):
    """x [wt] -> r [wt] binary64, the plain definition"""
    x = np.asarray(x, dtype=np.float64)
    wt = x.size
    return np.array([np.dot(x[:wt - t], x[t:]) for t in range(wt)])


def tempogram(o32, wt, f):
    """-> (T [wt, f] binary64, B [wt, f])"""
    x = frames_of(o32, wt, f).astype(np.float64)
    n = 4 * ((wt + 18) // 4)
    g = n * U / (1.0 - n * U)
    t = np.zeros((wt, f))
    b = np.zeros((wt, f))
    for i in range(f):
        r = autocorrelation(x[i])
        if not r[0] > 0.0:
            continue
        t[:, i] = r / r[0]
        a = np.abs(t[:, i])
        e = g * (a + 1.0) / (1.0 - g)
        b[:, i] = e + (U + V) * (a + e) + TINY + n * TINY / r[0]
    return t, b


# ---- step 6 ----
def tempo(t, pr, sr, hop, dt=None):
    """t [wt, f]: the tempogram (binary32 values or the definition's), pr: prior(), dt: what t may differ from the device's by
    (None: t is the device's own binary32 output) -> dict(tau, bpm, s [wt], margin, bounds: S [wt], bound: max S over the admissible lags)"""
    t = np.asarray(t, dtype=np.float64)
    f = t.shape[1]
    a = np.cumsum(t, axis=1)[:, -1] / f                   # (ascending in f)
    da = (f + 2) * V * np.abs(a) if dt is None else np.asarray(dt, dtype=np.float64).sum(axis=1) / f + (f + 2) * V * np.abs(a)
    s0 = np.log1p(1e6 * a)
    big = np.maximum(np.log1p(1e6 * (a + da)) - s0, s0 - np.log1p(1e6 * np.maximum(a - da, 0.0))) + 4.0 * V * (1.0 + np.abs(s0))
    assert (big <= 1e6 * da + 8.0 * V * (1.0 + np.abs(s0))).all()
    s = s0 + pr
    tau = int(np.argmax(s))                               # (the smallest argmax)
    others = np.delete(s, tau)
    margin = s[tau] - others.max() if others.size and np.isfinite(others.max()) else np.inf
    return dict(tau=tau, bpm=float(np.float32(60.0 * sr / (float(hop) * tau))), s=s, margin=float(margin),
                bound=float(big[np.isfinite(pr)].max()), bounds=big)


def check_tempo(want, got):
    """want: tempo(); got: the device's four floats -> (decided, worst error / bound)"""
    tau, b = int(got[1]), want["bound"]
    s = want["s"]
    assert float(got[1]) == tau and 1 <= tau < s.size and np.isfinite(s[tau])
    decided = want["margin"] > 2.0 * b
    if decided:
        assert tau == want["tau"] and np.float32(got[0]) == np.float32(want["bpm"]), (got, want["tau"], want["bpm"])
    else:
        assert s[tau] >= s.max() - 2.0 * b, (tau, want["tau"], s[tau], s.max(), b)
    fb = b + U * abs(s[tau]) + TINY                       # (s and the margin are returned in binary32)
    err = abs(float(got[2]) - s[tau])
    assert err <= fb, (float(got[2]), s[tau], fb)
    worst = err / fb
    if decided and np.isfinite(want["margin"]):
        mb = 2.0 * b + U * abs(want["margin"]) + TINY
        err = abs(float(got[3]) - want["margin"])
        assert err <= mb, (float(got[3]), want["margin"], mb)
        worst = max(worst, err / mb)
    return decided, worst
