"""Spectral descriptors of clips at n_fft 2048 and 4096 (include/pdmp3_bulk.h pdmp3_amd_spectral_*) restated
with numpy alone: the plan of a workgroup of k_clip_spectral, the place of a bin in its plane, the six rows in binary64, the
roll-off's cumulative sum in the stated order -- and the binary32 error bounds the tests hold the product to.  Nothing here is
the product's code.

The definition.  x[n] is the frame (clip_mel_ref.frames_of), X its spectrum by clip_stft_ref.stft (section 14's frame: window wt
with s = 1), P = Re^2 + Im^2, S = sqrt(P) for k = 0 .. N / 2, f_k = k sr / N, T = sum S:
  0 rms        sqrt(sum x^2 / N)                      3 bandwidth  sqrt(sum S (f - c)^2 / T)
  1 zcr        #{n >= 1: neg(x[n]) != neg(x[n-1])} / N, neg(v) = v < -t    4 rolloff    least f_k with S_0 + .. + S_k >= r T
  2 centroid   c = sum f S / T                        5 flatness   exp(mean ln max(amin, P)) / mean max(amin, P)
T = 0: rows 2 .. 4 are 0.

The bounds (u = 2^-24, D = 2^-53); nothing is measured here and there is no new constant.
  E  = c(N) u A                       bounds Re and Im (clip_stft_long_ref.c_of; A = sum |wt x| of the frame)
  dP = X + (2 u + u^2)(P + X),  X = 2 (|Re| + |Im|) E + 2 E^2          (section 15's chain)
  dS = sqrt 2 E + (S + sqrt 2 E) SQRT_C                                  (clip_stft_ref's mode 1: the pair as a vector, then
       fma's and the correctly rounded square root's roundings).  The rule at S = 0: nothing is divided by S -- dS stays
       sqrt 2 E (1 + SQRT_C) there, and is 0 on silence, where E is.
  The computed magnitudes S^ lie in [max(S - dS, 0), S + dS], so T^ in [T - sum dS, T + sum dS].  A binary64 sum of m terms adds
  at most m D of the sum of their magnitudes; each row is rounded once to binary32: r = u + (4 K + 16) D relative covers all of
  that for every row below (K = N / 2 + 1 terms, at most four sums, a division, a square root or an exponential).
  rms        |rms| (u + (N + 4) D): the final roundings alone (x^2 is exact in binary64).
  zcr        0.
  centroid   (sum f dS + c sum dS) / (T - sum dS), plus c r; both values lie in [0, sr / 2], so the bound is at most sr / 2,
             which also is what holds where sum dS >= T.
  bandwidth  V = sum p (f - c)^2, p = S / T.  The computed V^ is the variance of p^ = S^ / T^ about its own mean c^:
             V^ - V = sum (p^ - p)(f - c)^2 - (c^ - c)^2, and sum |p^ - p| (f - c)^2 <= (sum dS (f - c)^2 + V sum dS) / (T - sum dS).
             |sqrt V^ - sqrt V| <= min(dV / sqrt V, sqrt dV); plus the roundings; at most sr / 2.
  flatness   L = sum ln max(P, amin), Q = sum max(P, amin).  A logarithm's term is clip_mel_ref._log_term (dP over
             max(P - dP, amin) -- the floor's rule -- and LOG_C u max(1, |ln|) for logf); max(., amin) moves by at most dP and
             Q^ >= K amin.  |F^ - F| <= F (exp(dL / K) Q / max(Q - dQ, K amin) - 1), plus the roundings; at most 1: the
             geometric mean is at most the arithmetic one, both values lie in (0, 1] (the computed one within the roundings).
  rolloff is a decision: with cum_k = S_0 + .. + S_k, e_k = dS_0 + .. + dS_k, bin k MEETS the threshold when
             [cum_k - e_k, cum_k + e_k] and [r (T - sum dS), r (T + sum dS)] intersect.  A frame is undecided when a bin other
             than the reference's meets it; then the product may land on any bin that meets it (or on the reference's).  Every
             other frame must give the reference's bin exactly.  A silent frame (sum dS = 0) is decided: its bin is 0.
             How wide the threshold's interval is: sum dS is about 1450 E at N 2048 (2900 E at 4096), E about 135 u A (199 u A),
             which for a noise-like frame is a third to the whole of one bin's magnitude -- at roll_percent 0.85 most frames of
             such a signal are undecided by this rule, at 0.01 (librosa's "lowest frequency" use) few are: the tests choose
             roll_percent and signal by that, as DESIGN.md section 22 records."""
import math

import numpy as np

import clip_mel_ref as mref
import clip_stft_long_ref as lref
import clip_stft_ref as sref

U = sref.U
D64 = 2.0 ** -53
LOG_C = mref.LOG_C
LDS_MAX = 160 * 1024 - 64
SIZES = (2048, 4096)
ROWS = ("rms", "zcr", "centroid", "bandwidth", "rolloff", "flatness")
PATHS = ("N2048-tile8", "N4096-tile4")
UNDECIDED_CAP = 0.1


def plan(n_fft, hop):
    """the plan of a workgroup of k_clip_spectral restated: (tile, row_pad = 0, lds_bytes, launch path).  LDS: the span (kept),
    Z, the plane of tile x (N / 2 + 1) floats, 8 x tile floats of results"""
    assert n_fft in SIZES and 1 <= hop <= n_fft
    n2 = n_fft // 64
    tile = 8 if n_fft == 2048 else 4
    span = ((tile - 1) * hop + n_fft + 3) // 4 * 4
    lds = (span + tile * n2 * 32 + tile * (n_fft // 2 + 1) + 8 * tile + 3) // 4 * 4 * 4
    assert lds <= LDS_MAX
    return tile, 0, lds, "N%d-tile%d" % (n_fft, tile)


def col(k):
    """the column of bin k in a frame's row of the plane"""
    h = k >> 5
    return k ^ (((h & 1) << 2) | ((h >> 1) & 3) | (h & 24))


def rounding(n_fft):
    return U + (4 * (n_fft // 2 + 1) + 16) * D64


def zcr_count(x32, t):
    """x32 [.., N] binary32 -> the crossings of a frame, counted directly"""
    neg = np.asarray(x32, dtype=np.float32) < -np.float32(t)
    return (neg[..., 1:] != neg[..., :-1]).sum(axis=-1)


def rolloff_stated(s, roll_percent, n_fft):
    """s [.., K] magnitudes (binary32 values) -> the bin the stated order gives: 64 lanes sum their runs of N / 128 consecutive
    bins (the last one's ends with bin N / 2) in binary64, a scan adds the lanes' totals in ascending order, a bin's cumulative
    sum is its lane's prefix plus the run's sum so far, the threshold roll_percent times the scan's last value"""
    s = np.asarray(s, dtype=np.float64)
    lead = s.shape[:-1]
    r = n_fft // 128
    runs = np.cumsum(s[..., :n_fft // 2].reshape(lead + (64, r)), axis=-1)          # (np.cumsum adds one after the other)
    tot = runs[..., -1].copy()
    tot[..., 63] = tot[..., 63] + s[..., n_fft // 2]
    scan = np.cumsum(tot, axis=-1)
    prefix = np.concatenate([np.zeros(lead + (1,)), scan[..., :-1]], axis=-1)
    cum = np.concatenate([(prefix[..., None] + runs).reshape(lead + (n_fft // 2,)), scan[..., -1:]], axis=-1)
    return np.argmax(cum >= (roll_percent * scan[..., -1])[..., None], axis=-1)


def _rows_2_to_5(s, p, sr, n_fft, roll_percent, amin):
    """binary64 [.., K] -> centroid, bandwidth, rolloff bin, flatness, and T, V, L, Q"""
    k = n_fft // 2 + 1
    f = np.arange(k, dtype=np.float64) * (sr / n_fft)
    t = s.sum(axis=-1)
    safe = np.where(t > 0, t, 1.0)
    c = np.where(t > 0, (f * s).sum(axis=-1) / safe, 0.0)
    v = np.where(t > 0, (s * (f - c[..., None]) ** 2).sum(axis=-1) / safe, 0.0)
    roll = np.argmax(np.cumsum(s, axis=-1) >= (roll_percent * t)[..., None], axis=-1)
    pm = np.maximum(p, amin)
    ln = np.log(pm)
    big_l, q = ln.sum(axis=-1), pm.sum(axis=-1)
    flat = np.exp(big_l / k) / (q / k)
    return c, np.sqrt(v), roll, flat, t, v, ln, q


def spectral(y, pos0, start, n_frames, n_fft, hop, sr, roll_percent=0.85, amin=1e-10, zcr_threshold=1e-10, win_length=None, window=None):
    """y: [C, T] binary32 values of the signal from position pos0 on.  -> dict: want, bound [C, 6, F] binary64 (row 4: the
    reference's frequency, bound 0), roll [C, F] the reference's bin, meets [C, F, K] the bins whose interval meets the
    threshold, undecided [C, F], signal [C, F] (frames that hold a sample)"""
    y32 = np.atleast_2d(np.asarray(y, dtype=np.float32))
    amin = float(np.float32(amin))
    k = n_fft // 2 + 1
    bin_hz = sr / n_fft
    f = np.arange(k, dtype=np.float64) * bin_hz
    x, b0 = sref.stft(y32, pos0, start, n_frames, n_fft, hop, 0, 1e-10, win_length, window, False)      # [C, K, F, 2]
    e = np.moveaxis(b0[..., 0] * (lref.c_of(n_fft) / (n_fft + 2)), 1, 2)                                 # [C, F, K]
    re, im = np.moveaxis(x[..., 0], 1, 2), np.moveaxis(x[..., 1], 1, 2)
    p = re * re + im * im
    s = np.sqrt(p)
    cross = 2.0 * (np.abs(re) + np.abs(im)) * e + 2.0 * e * e
    dp = cross + sref.T2 * (p + cross)
    r2e = math.sqrt(2.0) * e
    ds = r2e + (s + r2e) * sref.SQRT_C
    rnd = rounding(n_fft)
    nyq = sr / 2.0

    frames = np.stack([mref.frames_of(y32[ch], pos0, start, n_frames, n_fft, hop) for ch in range(y32.shape[0])])   # [C, F, N]
    rms = np.sqrt((frames * frames).sum(axis=-1) / n_fft)
    zcr = zcr_count(frames.astype(np.float32), zcr_threshold) / n_fft
    c, bw, roll, flat, t, v, ln, q = _rows_2_to_5(s, p, sr, n_fft, roll_percent, amin)

    sds = ds.sum(axis=-1)
    room = t - sds
    ok = room > 0
    safe = np.where(ok, room, 1.0)
    dc0 = np.where(ok, ((f * ds).sum(axis=-1) + c * sds) / safe, np.where(sds > 0, nyq, 0.0))
    dc = np.minimum(dc0 * (1.0 + U) + c * rnd, nyq)
    dv = np.where(ok, ((ds * (f - c[..., None]) ** 2).sum(axis=-1) + v * sds) / safe, nyq * nyq) + dc * dc
    dv = np.where(sds > 0, dv, 0.0)
    dbw = np.minimum(np.where(v > 0, dv / np.where(v > 0, np.sqrt(v), 1.0), np.inf), np.sqrt(dv))
    dbw = np.minimum(dbw * (1.0 + U) + bw * rnd, nyq)
    dl = mref._log_term(p, dp, ln, math.e, amin).sum(axis=-1)
    dq = dp.sum(axis=-1)
    with np.errstate(over="ignore"):
        dflat = np.minimum(flat * (np.exp(dl / k) * q / np.maximum(q - dq, k * amin) - 1.0) * (1.0 + U) + flat * rnd, 1.0)
    drms = rms * (U + (n_fft + 4) * D64)

    cum, ecum = np.cumsum(s, axis=-1), np.cumsum(ds, axis=-1)
    lo, hi = roll_percent * (t - sds), roll_percent * (t + sds)
    meets = (cum + ecum >= lo[..., None]) & (cum - ecum <= hi[..., None]) & (sds > 0)[..., None]      # (silence: nothing can move)
    other = meets.copy()
    np.put_along_axis(other, roll[..., None], False, axis=-1)
    want = np.stack([rms, zcr, c, bw, roll * bin_hz, flat], axis=1)
    bound = np.stack([drms, np.zeros_like(zcr), dc, dbw, np.zeros_like(c), dflat], axis=1)
    return dict(want=want, bound=bound, roll=roll, meets=meets, undecided=other.any(axis=-1), signal=np.abs(frames).sum(axis=-1) > 0)


def check_rolloff(got_hz, res, sr, n_fft):
    """the product's row 4 [C, F] against spectral()'s result by the undecided rule -> (undecided frames, frames).  Asserts that
    every value is a bin's frequency exactly, that a decided frame gives the reference's bin and an undecided one a bin that
    meets the threshold"""
    bin_hz = sr / n_fft
    got_bin = np.rint(np.asarray(got_hz, dtype=np.float64) / bin_hz).astype(np.int64)
    assert got_bin.shape == res["roll"].shape and (got_bin >= 0).all() and (got_bin <= n_fft // 2).all()
    assert np.array_equal((got_bin * bin_hz).astype(np.float32), np.asarray(got_hz, dtype=np.float32)), "row 4 is not a bin's frequency"
    und = res["undecided"]
    same = got_bin == res["roll"]
    assert same[~und].all(), "a decided frame off the reference's bin: %s" % (np.argwhere(~und & ~same)[:4].tolist(),)
    landed = np.take_along_axis(res["meets"], got_bin[..., None], axis=-1)[..., 0]
    assert (same | landed)[und].all(), "an undecided frame on a bin that does not meet the threshold"
    return int(und.sum()), int(und.size)


def from_spectrum(s32, p32, sr, n_fft, roll_percent=0.85, amin=1e-10):
    """s32, p32 [.., K]: the binary32 magnitudes and powers the spectrum call stores -> (want [.., 4], bound [.., 4]) for rows
    2 .. 5 from them: the same formulas in binary64, and the reductions' bound ALONE -- the roundings r, and logf's LOG_C u
    max(1, |ln|) a bin for row 5.  Row 4: the bin of rolloff_stated() times sr / N, bound 0: the order is repeated exactly"""
    amin = float(np.float32(amin))
    s, p = np.asarray(s32, dtype=np.float64), np.asarray(p32, dtype=np.float64)
    k = n_fft // 2 + 1
    c, bw, _, flat, t, v, ln, q = _rows_2_to_5(s, p, sr, n_fft, roll_percent, amin)
    rnd = rounding(n_fft)
    roll = rolloff_stated(s, roll_percent, n_fft)
    dl = (LOG_C * U * np.maximum(1.0, np.abs(ln))).sum(axis=-1)
    want = np.stack([c, bw, roll * (sr / n_fft), flat], axis=-1)
    bound = np.stack([c * rnd, bw * rnd, np.zeros_like(c), flat * ((np.exp(dl / k) - 1.0) * (1.0 + U) + rnd)], axis=-1)
    return want, bound
