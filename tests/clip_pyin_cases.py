"""The many-bin shapes of pYIN and the planted curves that steer its path, for the host tests on the emulated
kernels (tests/test_clip_pyin_host.py) and the device tests (tests/test_gpu_clip_pyin_forms.py) alike: they stand here because
both read them and no test imports a test.  A helper module: no test, no fixture.

A planted curve is 1 everywhere but for one or two troughs a frame.  A trough of height `depth` alone in its frame has, by the
definition (tests/clip_pyin_ref.py observe), P = w_ij + .. + w_nt + no_trough_prob wsum[ij - 1], ij the least threshold above the
depth; its two neighbours are equal, so the parabola's vertex is the lag itself.  DEEP lies under every threshold: P = wsum[nt],
which is 1.0 in binary32 at the default beta, so v = 1 and the unvoiced states observe 0.  SHALLOW lies between the first two
thresholds of a hundred: v = 0.985 there."""
import numpy as np

import clip_pyin_ref as ref

DEEP, SHALLOW = 0.001, 0.015

# ---- shapes: more bins than threads, more states than a dynamic LDS request holds ----
BINS_1201 = ref.args(resolution=0.05)                                                                      # band 201, path LDS 79 240
BINS_2048 = ref.args(sample_rate=48000, frame_length=2048, win_length=400, hop=512, fmin=30.0, fmax=30.0 * 2 ** (2047.5 / 240),
                     resolution=0.05)                                                                      # lags 4 .. 1600, 4 frames a workgroup
BINS_2048_NT256 = dict(BINS_2048, n_thresholds=256)                                                        # 2 frames a workgroup
BINS_2048_TMAX2000 = dict(BINS_2048, win_length=32, fmin=24.0, fmax=24.0 * 2 ** (2047.5 / 240))            # lags 5 .. 2000, 2 frames
BINS_1025 = ref.args(sample_rate=16000, frame_length=1024, win_length=512, hop=256, fmin=40.0, fmax=40.0 * 2 ** (1024.5 / 240),
                     resolution=0.05)                                                                      # the first bin of a second turn
BINS_1024 = dict(BINS_1025, fmax=40.0 * 2 ** (1023.5 / 240))                                               # one bin a thread, the big form
# name -> (arguments, frames of a workgroup of the observation kernel)
MANY = {"nb1201": (BINS_1201, 8), "nb2048-obs4": (BINS_2048, 4), "nb2048-nt256-obs2": (BINS_2048_NT256, 2),
        "nb2048-tmax2000-obs2": (BINS_2048_TMAX2000, 2), "nb1025": (BINS_1025, 8), "nb1024": (BINS_1024, 8)}


def kw(a):
    return {k: v for k, v in a.items() if k not in ("sample_rate", "channels")}


# ---- planted curves ----
def curve_of(a, frames):
    """frames: per frame a list of (lag, height) -> float32 [tmax + 1, F], 1 elsewhere"""
    k = ref.numbers(a)
    c = np.ones((k["tmax"] + 1, len(frames)), dtype=np.float32)
    for f, troughs in enumerate(frames):
        for tau, height in troughs:
            assert k["tmin"] < tau < k["tmax"]
            c[tau, f] = height
    return c


def bin_of(t, tau):
    """the bin of a trough whose period is the lag itself"""
    return int((float(tau) <= t["T"]).sum())


def lag_near(a, t, want):
    """the lag whose bin lies nearest to `want`"""
    k = ref.numbers(a)
    taus = np.arange(k["tmin"] + 1, k["tmax"])
    bins = np.array([bin_of(t, tau) for tau in taus])
    return int(taus[np.argmin(np.abs(bins - want))])


def observation(curve, a, t):
    """the definition's observation [n_b + 1, F] of a curve, in binary32 as the product stores it"""
    k = ref.numbers(a)
    cols = [ref.observe(curve[:, f], k["tmin"], k["tmax"], t, a["no_trough_prob"]) for f in range(curve.shape[1])]
    return np.stack([np.concatenate([o, [v]]) for o, v, _, _ in cols], axis=1).astype(np.float32)


def decided(obs, t):
    """the definition's decode of obs -> (states [F]: bin, or n_b + bin where unvoiced; sure [F]: the margin exceeds 2 eps)"""
    _, mm, _, _, _ = ref.decode(obs, t)
    top = np.sort(mm, axis=1)
    return mm.argmax(axis=1), top[:, -1] - top[:, -2] > 2 * ref.epsilon(obs.shape[1])


def voicing(obs, t):
    """the definition's decode of obs -> (voiced [F], sure [F]: the best voiced and the best unvoiced state lie more than 2 eps apart)"""
    nb = t["n_bins"]
    _, mm, _, _, _ = ref.decode(obs, t)
    v, u = mm[:, :nb].max(axis=1), mm[:, nb:].max(axis=1)
    return v > u, np.abs(v - u) > 2 * ref.epsilon(obs.shape[1])


def glide(a, t, f, first_bin, step):
    """one SHALLOW trough a frame whose bin rises from first_bin by about `step` a frame -> (curve, the planted bins [F])"""
    lags = [lag_near(a, t, first_bin + i * step) for i in range(f)]
    return curve_of(a, [[(tau, SHALLOW)] for tau in lags]), np.array([bin_of(t, tau) for tau in lags])


def jump(a, t, f, at, bin_a, bin_b):
    """one DEEP trough a frame: near bin_a in the frames before `at`, near bin_b from there on -> (curve, the planted bins [F])"""
    la, lb = lag_near(a, t, bin_a), lag_near(a, t, bin_b)
    lags = [la] * at + [lb] * (f - at)
    return curve_of(a, [[(tau, DEEP)] for tau in lags]), np.array([bin_of(t, tau) for tau in lags])


def voiced_stretch(a, t, f, lo, hi, at_bin, height=0.035, second=(0.5, 3)):
    """no trough outside the frames [lo, hi), one of `height` near at_bin inside them, and in the middle one a second, shallower
    trough `second[1]` lags below -> (curve, the planted bin)"""
    tau = lag_near(a, t, at_bin)
    frames = [[(tau, height)] if lo <= i < hi else [] for i in range(f)]
    frames[(lo + hi) // 2].append((tau - second[1], second[0]))
    return curve_of(a, frames), bin_of(t, tau)


def top_bin(a, t, f):
    """one DEEP trough a frame whose parabola's vertex lies in the middle of the last bin, n_b - 1: with bins narrower than a lag no
    lag need fall into it, so the trough's neighbours are 1 in front and c behind (above 1 where the vertex lies in front), and the vertex lies
    (1 - c) / (2 (1 - 2 b + c)) from the lag -> (curve, the bin)"""
    nb = t["n_bins"]
    period = 0.5 * (t["T"][nb - 2] + t["T"][nb - 1])
    tau = int(round(period))
    delta, b = period - tau, DEEP
    c = (1.0 - 2.0 * delta * (1.0 - 2.0 * b)) / (1.0 + 2.0 * delta)
    assert abs(delta) < 0.45 and b < c
    return curve_of(a, [[(tau, b), (tau + 1, c)] for _ in range(f)]), nb - 1
