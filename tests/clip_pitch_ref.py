"""The pitch of clips (include/pdmp3_bulk.h pdmp3_amd_pitch_spec) in binary64 with numpy: the lag range,
the difference function, the cumulative-mean normalisation, librosa.yin's decision and the parabolic refinement -- and, value by
value, the bound of what k_clip_pitch may return for them, derived from the binary32 chain of the matrix instruction alone (no
measured constant), the frames whose decision is undecided within those bounds, and item 7's self-consistency of the two output
modes.  The restatement of the host tests and the reference of the device tests."""
import math

import numpy as np

U = 2.0 ** -24            # binary32: half an ulp of 1
E = 2.0 ** -53            # binary64
MAX_SPAN = 8 * 2048       # samples under one workgroup's scan of the squares, at most


def defaults(frame_length=2048, win_length=None, hop=None):
    n = int(frame_length)
    return n, n // 2 if not win_length else int(win_length), n // 4 if not hop else int(hop)


def _quotient(num, den, up):
    q = num / den
    n = float(round(q))
    if abs(q - n) < 1e-9:
        from fractions import Fraction
        if Fraction(den) * int(n) != Fraction(num):
            return None
        return int(n)
    return int(math.ceil(q) if up else math.floor(q))


def lags(sr, fmin, fmax, n, w):
    """(tmin, tmax, tiles) or None where the spec is refused (item 2, and item 8's fmin / fmax / tmin >= tmax)"""
    if not (fmin > 0.0) or not (fmax > fmin) or not (fmax <= sr / 2.0):
        return None
    lo, hi = _quotient(float(sr), float(fmax), False), _quotient(float(sr), float(fmin), True)
    if lo is None or hi is None:
        return None
    tmin, tmax = max(1, lo), min(hi, n - w - 1)
    if tmin >= tmax:
        return None
    return tmin, tmax, (tmax + 256) // 256


def valid(j_all, start, hop, f):
    left = j_all - start
    return 0 if left <= 0 else min(-(-left // hop), f)


def frames(row, lead, n, hop, f):
    """row: the binary32 samples from start - n / 2 + lead on -> float64 [f, n]: frame f's z, zeros in front and behind"""
    x = np.concatenate([np.zeros(lead), np.asarray(row, dtype=np.float64), np.zeros(n + hop)])
    need = (f - 1) * hop + n
    if x.size < need:
        x = np.concatenate([x, np.zeros(need - x.size)])
    return np.lib.stride_tricks.sliding_window_view(x, n)[::hop][:f].copy()


def plain_curve(z, w, tmax):
    """d'(0 .. tmax) of one frame by the double loop over (z[j] - z[j + tau])^2"""
    d = np.array([sum((z[j] - z[j + tau]) ** 2 for j in range(w)) for tau in range(tmax + 1)])
    return _normalise(d)[0]


def _normalise(d):
    s = np.concatenate([[0.0], np.cumsum(d[1:])])
    tau = np.arange(d.size, dtype=np.float64)
    dp = np.ones_like(d)
    ok = s > 0
    ok[0] = False
    dp[ok] = d[ok] * tau[ok] / s[ok]
    return dp, s


def curve(z, w, tmax, span_energy=None):
    """one frame z (float64 [n]) -> (d' [tmax + 1], its bound [tmax + 1]; inf where the bound of the mean reaches the mean)"""
    win = np.lib.stride_tricks.sliding_window_view(z, w)[:tmax + 1]
    r = win @ z[:w]
    e = (win * win).sum(axis=1)
    a = np.abs(win) @ np.abs(z[:w])
    d = e[0] + e - 2.0 * r
    dp, s = _normalise(d)
    # r^: a chain of n fused multiply-adds in binary32 (the masked and padded steps add exact zeros)
    nk = 4 * ((w + 15 + 3) // 4)
    e_r = nk * U / (1.0 - nk * U) * a
    # e: a difference of two binary64 prefix sums of at most MAX_SPAN exact squares, whatever their fixed order
    energy = float((z * z).sum()) if span_energy is None else float(span_energy)
    e_e = 2.0 * MAX_SPAN * E * energy
    e_d = 2.0 * e_r + 2.0 * e_e + 3.0 * E * (e[0] + e + 2.0 * np.abs(r))
    e_d[0] = 0.0
    tau = np.arange(tmax + 1, dtype=np.float64)
    e_s = np.cumsum(e_d) + tau * E * np.cumsum(np.abs(d) + e_d)
    bound = np.zeros(tmax + 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        m, e_m = s[1:] / tau[1:], e_s[1:] / tau[1:]
        b = np.where(m > e_m, (e_d[1:] + np.abs(dp[1:]) * e_m) / (m - e_m), np.inf)
        b = np.where((m <= e_m) & (e_s[1:] == 0.0) & (e_d[1:] == 0.0), 0.0, b)       # (zeros so far: both sides say 1)
    with np.errstate(invalid="ignore"):
        bound[1:] = b + np.where(s[1:] > 0, (U + 4.0 * E) * (np.abs(dp[1:]) + b), 0.0)   # (the 1 of S <= 0 is not rounded)
    return dp, bound


def decide(dp, tmin, tmax, threshold):
    """rule 5 on a curve (binary64, or the device's binary32 values) -> tau*"""
    v = np.asarray(dp, dtype=np.float64)
    for tau in range(tmin, tmax):
        trough = v[tau] < v[tau + 1] if tau == tmin else (v[tau] < v[tau - 1] and v[tau] <= v[tau + 1])
        if trough and v[tau] < threshold:
            return tau
    return tmin + int(np.argmin(v[tmin:tmax + 1]))


def refine(a, b, c, tau, tmin, tmax, sr):
    """rule 6 in binary64 -> f0"""
    delta = 0.0
    if tmin < tau < tmax:
        dd = (a - 2.0 * b) + c
        if dd > 0.0:
            delta = (a - c) / (2.0 * dd)
    return sr / (tau + delta)


def undecided(dp, bound, tmin, tmax, threshold, tau):
    """could a comparison the decision made turn within the intervals?"""
    lo, hi = dp - bound, dp + bound
    if not np.isfinite(bound[tmin:tmax + 1]).all():
        return True

    def could_be_trough_under(t):
        if t == tmin:
            return lo[t] < hi[t + 1] and lo[t] < threshold
        return lo[t] < hi[t - 1] and lo[t] <= hi[t + 1] and lo[t] < threshold

    chosen_by_threshold = tau < tmax and dp[tau] < threshold and (
        dp[tau] < dp[tau + 1] if tau == tmin else (dp[tau] < dp[tau - 1] and dp[tau] <= dp[tau + 1]))
    if chosen_by_threshold:
        if any(could_be_trough_under(t) for t in range(tmin, tau)):
            return True
        sure = hi[tau] < lo[tau + 1] and hi[tau] < threshold and (tau == tmin or hi[tau] < lo[tau - 1])
        return not sure
    if any(could_be_trough_under(t) for t in range(tmin, tmax)):
        return True
    others = np.delete(lo[tmin:tmax + 1], tau - tmin)
    return bool((others <= hi[tau]).any())


def f0_interval(dp, bound, tau, tmin, tmax, sr):
    """(lowest, highest f0 over the corners of (a, b, c)'s box, one binary32 rounding added; None where D's sign could turn)"""
    if not (tmin < tau < tmax):
        f = sr / tau
        return f * (1.0 - 2.0 * U), f * (1.0 + 2.0 * U)
    vals = []
    for sa in (-1, 1):
        for sb in (-1, 1):
            for sc in (-1, 1):
                a, b, c = dp[tau - 1] + sa * bound[tau - 1], dp[tau] + sb * bound[tau], dp[tau + 1] + sc * bound[tau + 1]
                if not (a - 2.0 * b + c > 0.0):
                    return None
                vals.append(refine(a, b, c, tau, tmin, tmax, sr))
    return min(vals) * (1.0 - 2.0 * U), max(vals) * (1.0 + 2.0 * U)


def check(row, lead, sr, n, w, hop, f, tmin, tmax, threshold, got_pitch, got_curve):
    """One (clip, channel): the device's or the emulation's [3, f] and [tmax + 1, f] against the definition on `row`.
    Asserts every curve value within its bound and, on decided frames, tau* exact, plane 1 within its bound and f0 inside its
    interval.  -> (worst error / bound, undecided frames, frames that hold signal)"""
    z = frames(row, lead, n, hop, f)
    energy = float((np.asarray(row, dtype=np.float64) ** 2).sum())
    worst, und, live = 0.0, 0, 0
    for i in range(f):
        if not z[i].any():
            if got_curve is not None:
                assert (got_curve[:, i] == 1.0).all(), "the curve of a frame of zeros is not 1 (frame %d)" % i
            if got_pitch is not None:
                assert got_pitch[:, i].tolist() == [0.0, 1.0, 0.0], (i, got_pitch[:, i])
            continue
        live += 1
        dp, bound = curve(z[i], w, tmax, energy)
        fin = np.isfinite(bound)
        if got_curve is not None:
            err = np.abs(got_curve[:, i].astype(np.float64) - dp)
            assert (err[fin] <= bound[fin]).all(), "frame %d: d' beyond its bound by %g at lag %d" % (
                i, float((err - bound)[fin].max()), int(np.argmax(np.where(fin, err - bound, -np.inf))))
            assert got_curve[0, i] == 1.0
            nzb = fin & (bound > 0)
            if nzb.any():
                worst = max(worst, float((err[nzb] / bound[nzb]).max()))
        tau = decide(dp, tmin, tmax, threshold)
        iv = f0_interval(dp, bound, tau, tmin, tmax, sr) if fin[tmin:tmax + 1].all() else None
        if undecided(dp, bound, tmin, tmax, threshold, tau) or iv is None:
            und += 1
            continue
        if got_pitch is not None:
            assert got_pitch[2, i] == tau, "frame %d: tau* %g, the definition's %d (decided)" % (i, got_pitch[2, i], tau)
            e1 = abs(float(got_pitch[1, i]) - dp[tau])
            assert e1 <= bound[tau], (i, e1, bound[tau])
            if bound[tau] > 0:
                worst = max(worst, e1 / bound[tau])
            assert iv[0] <= float(got_pitch[0, i]) <= iv[1], "frame %d: f0 %r outside [%r, %r]" % (i, got_pitch[0, i], iv[0], iv[1])
    return worst, und, live


def self_consistent(row, lead, sr, n, hop, f, tmin, tmax, threshold, got_pitch, got_curve):
    """item 7 on every frame: plane 2 is rule 5 on the mode-1 output, plane 1 that curve at tau* bit for bit, plane 0 rule 6 in
    binary64 on the three binary32 values.  -> the largest distance of plane 0 from numpy's evaluation in ulps of binary32"""
    z = frames(row, lead, n, hop, f)
    ulps = 0
    for i in range(f):
        c = got_curve[:, i]
        assert c.dtype == np.float32
        if not z[i].any():
            assert got_pitch[:, i].tolist() == [0.0, 1.0, 0.0] and (c == 1.0).all()
            continue
        tau = decide(c, tmin, tmax, threshold)
        assert got_pitch[2, i] == tau, (i, got_pitch[2, i], tau)
        assert got_pitch[1, i].tobytes() == c[tau].tobytes(), (i, got_pitch[1, i], c[tau])
        a, b, cc = (float(c[tau - 1]), float(c[tau]), float(c[min(tau + 1, tmax)]))
        want = np.float32(refine(a, b, cc, tau, tmin, tmax, float(sr)))
        ulps = max(ulps, abs(int(np.float32(got_pitch[0, i]).view(np.int32)) - int(want.view(np.int32))))
    return ulps
