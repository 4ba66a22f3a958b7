"""Median-filter harmonic-percussive separation of clips (include/pdmp3_bulk.h pdmp3_amd_hpss_*) restated
with numpy alone: the plan of a workgroup of k_clip_hpss, the reflection of the bins, the two medians by sliding windows and
np.sort, the soft masks in binary64 -- and the bounds the tests hold the product to.  Nothing here is the product's code.

The definition.  S [K, F + 2 rh] is the magnitude spectrogram of the frames -rh .. F - 1 + rh of the clip (clip_stft_ref.stft,
section 14's frame), rh = (Lh - 1) / 2, rp = (Lp - 1) / 2:
  Hm[k][f] = median of S[k][f - rh .. f + rh]                      (along time over the stream's real frames)
  Pm[k][f] = median of S[rho(i)][f], i = k - rp .. k + rp          (rho: np.pad(mode="symmetric"), scipy's "reflect")
  (X, R) = (Hm, margin_harm Pm) for the harmonic mask, (Pm, margin_perc Hm) for the percussive one
  finite power p: max(X, R) < 2^-126 -> 0.5 if both margins are 1, else 0; otherwise m = X^p / (X^p + R^p)
  power = inf:    m = 1 if X > R, else 0

The bounds (u = 2^-24); nothing is measured here and there is no new constant.
  E, dS      section 14's E = c(N) u A and section 22's dS = sqrt 2 E + (S + sqrt 2 E) SQRT_C (clip_spectral_ref.py).
  medians    every computed magnitude lies in [max(S - dS, 0), S + dS], and the k-th smallest of a window does not fall when a
             value of the window rises: the computed Hm lies in [Hm-, Hm+], the medians of the windows of S - dS and of S + dS, and
             Pm likewise.  That interval lies inside Hm -+ (the largest dS of the window), the issue's statement of it, and is
             what the tests use: a loud frame far above the median brings its large dS into the window, not into the median.
  rounding   m is evaluated in binary64 (a product, up to two squares, a sum, a quotient: below 2^-50 relative together) and
             rounded once to binary32: (2^-24 + 2^-50) m, plus 2^-150, half the spacing of binary32 below 2^-126, where the
             relative term alone is not what one rounding to that format can do.
  finite p   m = sigma(-p t), t = ln R - ln X, |sigma'| <= 1 / 4, and t stays in [ln R- - ln X+, ln R+ - ln X-]:
                 |dm| <= (p / 4) max(ln(R+ / R) + ln(X / X-), ln(R / R-) + ln(X+ / X)) + rounding      (the margin cancels in R+ / R)
             where a value that cannot move (an exact zero: silence) adds nothing; with X- = X - dX this is the issue's
             -ln(1 - dX / X).  Where X- = 0 < X+ or R- = 0 < R+, or where 2^-126 lies between max(X-, R-) and max(X+, R+) (the
             silent rule is a decision), the bound is the trivial 1.  The share of trivial elements is counted and capped.
  inf        an element is decided when X- > R+ (1) or X+ <= R- (0), or when nothing can move (silence); a decided element must
             match exactly; the undecided share has the same cap."""
import math

import numpy as np

import clip_stft_long_ref as lref
import clip_stft_ref as sref

U = sref.U
ROUND = 2.0 ** -24 + 2.0 ** -50
TINY = 2.0 ** -150
SILENT = 2.0 ** -126
SIZES = (2048, 4096)
CAP = 0.1
MODES = ("mask", "magnitude", "complex", "median")
TILE_BINS, TILE_FRAMES, MAX_KERNEL = 64, 64, 31


def plan(kernel_harm, kernel_perc):
    """the plan restated: (front, back, tile bins, tile frames, LDS row pitch, LDS bytes) -- one tile and one layout, made for the
    largest kernels, for every pair of sizes"""
    for l in (kernel_harm, kernel_perc):
        assert 3 <= l <= MAX_KERNEL and l % 2 == 1
    pitch = TILE_FRAMES + MAX_KERNEL - 1
    return kernel_harm // 2, kernel_harm // 2, TILE_BINS, TILE_FRAMES, pitch, (TILE_BINS + MAX_KERNEL - 1) * pitch * 4


def reflect(i, bins):
    return -1 - i if i < 0 else 2 * bins - 1 - i if i >= bins else i


def _windows(a, length, axis):
    return np.lib.stride_tricks.sliding_window_view(a, length, axis=axis)


def medians(s, kernel_harm, kernel_perc):
    """s [.., K, F + 2 rh] -> (Hm, Pm) [.., K, F]"""
    rh, rp = kernel_harm // 2, kernel_perc // 2
    pick = lambda w, r: np.sort(w, axis=-1)[..., r]
    hm = pick(_windows(s, kernel_harm, -1), rh)
    pad = [(0, 0)] * (s.ndim - 2) + [(rp, rp), (0, 0)]
    centre = s[..., rh:s.shape[-1] - rh]
    pm = pick(_windows(np.pad(centre, pad, mode="symmetric"), kernel_perc, -2), rp)
    return hm, pm


def mask(x, other, margin, power, unit):
    """binary64 arrays -> librosa.util.softmask(x, margin other, power) by the contract's rules"""
    x = np.asarray(x, dtype=np.float64)
    r = margin * np.asarray(other, dtype=np.float64)
    if math.isinf(power):
        return (x > r).astype(np.float64)
    big = np.maximum(x, r)
    a, b = x ** power, r ** power
    with np.errstate(invalid="ignore", divide="ignore"):
        m = a / (a + b)
    return np.where(big < SILENT, 0.5 if unit else 0.0, m)


def masks(hm, pm, margin_harm, margin_perc, power):
    """-> [.., 2, K, F] from the medians [.., K, F]"""
    unit = margin_harm == 1.0 and margin_perc == 1.0
    return np.stack([mask(hm, pm, margin_harm, power, unit), mask(pm, hm, margin_perc, power, unit)], axis=-3)


def rounding(m):
    return ROUND * np.abs(m) + TINY


def _log_ratio(num, den, moved):
    """ln(num / den) where `moved`, else 0 (the places where den is 0 are the caller's: trivial)"""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(moved & (den > 0), np.log(np.where(den > 0, num, 1.0) / np.where(den > 0, den, 1.0)), 0.0)


def _one_bound(x, xlo, xhi, o, olo, ohi, margin, power, want):
    """-> (bound, trivial) of the mask of x in [xlo, xhi] against margin o, o in [olo, ohi]; power inf: (None, undecided)"""
    r, rlo, rhi = margin * o, margin * olo, margin * ohi
    mx, mr = xhi > xlo, rhi > rlo
    if math.isinf(power):
        return None, (mx | mr) & ~((xlo > rhi) | (xhi <= rlo))
    up = _log_ratio(rhi, r, mr) + _log_ratio(x, xlo, mx)
    down = _log_ratio(r, rlo, mr) + _log_ratio(xhi, x, mx)
    straddle = (np.maximum(xlo, rlo) < SILENT) & (np.maximum(xhi, rhi) >= SILENT)
    trivial = (mx & (xlo <= 0)) | (mr & (rlo <= 0)) | (mx & (x <= 0)) | (mr & (r <= 0)) | straddle
    return np.where(trivial, 1.0, (power / 4.0) * np.maximum(up, down) * (1.0 + U) + rounding(want)), trivial


def hpss(y, pos0, start, n_frames, n_fft, hop, kernel_harm=31, kernel_perc=31, power=2.0, margin_harm=1.0, margin_perc=1.0, win_length=None,
         window=None):
    """y: [C, T] binary32 values of the signal from position pos0 on.  -> dict: s, ds [C, K, F + 2 rh] (the spectrum of the
    widened clip and its bound), hm, pm [C, K, F] and their intervals hm_lo, hm_hi, pm_lo, pm_hi, want [C, 2, K, F] the masks in
    binary64, bound [C, 2, K, F] (finite power; None at inf), loose [C, 2, K, F]: the elements whose bound is trivial (finite
    power) or that are undecided (inf)"""
    rh = kernel_harm // 2
    y32 = np.atleast_2d(np.asarray(y, dtype=np.float32))
    s, b = sref.stft(y32, pos0, start - rh * hop, n_frames + 2 * rh, n_fft, hop, 1, 1e-10, win_length, window, False)       # [C, K, F + 2 rh]
    # clip_stft_ref's bound is sqrt 2 E + (S + sqrt 2 E) SQRT_C with E = (N + 2) u A; section 14's E is c(N) u A
    r2e = (b - s * sref.SQRT_C) / (1.0 + sref.SQRT_C) * (lref.c_of(n_fft) / (n_fft + 2))
    ds = r2e + (s + r2e) * sref.SQRT_C
    hm, pm = medians(s, kernel_harm, kernel_perc)
    hm_lo, pm_lo = medians(np.maximum(s - ds, 0.0), kernel_harm, kernel_perc)
    hm_hi, pm_hi = medians(s + ds, kernel_harm, kernel_perc)
    want = masks(hm, pm, margin_harm, margin_perc, power)
    bh, lh = _one_bound(hm, hm_lo, hm_hi, pm, pm_lo, pm_hi, margin_harm, power, want[..., 0, :, :])
    bp, lp = _one_bound(pm, pm_lo, pm_hi, hm, hm_lo, hm_hi, margin_perc, power, want[..., 1, :, :])
    bound = None if bh is None else np.stack([bh, bp], axis=-3)
    return dict(s=s, ds=ds, hm=hm, pm=pm, hm_lo=hm_lo, hm_hi=hm_hi, pm_lo=pm_lo, pm_hi=pm_hi, want=want, bound=bound,
                loose=np.stack([lh, lp], axis=-3))


def check_masks(got, res, power):
    """the product's masks [C, 2, K, F] against hpss()'s result -> (worst error / bound over the elements with a real bound,
    loose elements, elements).  Every element is held: within its bound (finite power), exactly where decided (inf)"""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == res["want"].shape
    loose = res["loose"]
    if math.isinf(power):
        assert np.isin(got, (0.0, 1.0)).all(), "a mask at power inf that is neither 0 nor 1"
        off = (got != res["want"]) & ~loose
        assert not off.any(), "a decided element differs: %s" % (np.argwhere(off)[:4].tolist(),)
        return 0.0, int(loose.sum()), int(loose.size)
    err = np.abs(got - res["want"])
    assert (err <= res["bound"]).all(), "error beyond the bound by %g at %s" % (
        float((err - res["bound"]).max()), np.unravel_index(np.argmax(err - res["bound"]), err.shape))
    real = ~loose
    worst = float((err[real] / res["bound"][real]).max()) if real.any() else 0.0
    return worst, int(loose.sum()), int(loose.size)


def from_medians(hm32, pm32, margin_harm, margin_perc, power):
    """the binary32 medians the call stores in mode 3 [.., K, F] -> (want [.., 2, K, F], bound): item 4 on them in binary64 and the
    rounding's bound alone (0 at power inf: exact)"""
    want = masks(np.asarray(hm32, dtype=np.float64), np.asarray(pm32, dtype=np.float64), margin_harm, margin_perc, power)
    return want, (np.zeros_like(want) if math.isinf(power) else rounding(want))
