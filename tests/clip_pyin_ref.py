"""pYIN pitch tracking of clips (include/pdmp3_bulk.h pdmp3_amd_pyin_spec) in binary64 with numpy: the
numbers derived from the arguments, every table by librosa's own construction (scipy's triangle, numpy's pad / roll / kron,
boltzmann.pmf's and beta.cdf's formulas), the candidate stage on a binary32 curve, the Viterbi decode with max-marginals, and the
derived bounds and decisions that the host tests (on the emulated kernels) and the device tests evaluate.  No measured constant:
C_LOG is the one assumption, written down below."""
import math
from fractions import Fraction

import numpy as np

import clip_pitch_ref as pref

E = 2.0 ** -53
U32 = 2.0 ** -24
L0 = math.log(2.0 ** -1022)
TINY = 2.0 ** -1022
C_LOG = 4                 # ulps of the device's binary64 log: the ROCm installation's documents state none, so 4 is assumed
CAP = 0.1                 # the share of a test's frames that may be undecided against the binary64 chain

DEFAULTS = dict(sample_rate=22050, frame_length=2048, win_length=0, hop=0, fmin=65.406, fmax=2093.0, n_thresholds=100, beta=(2, 18),
                boltzmann=2.0, resolution=0.1, max_transition_rate=35.92, switch_prob=0.01, no_trough_prob=0.01)


def args(**kw):
    a = dict(DEFAULTS)
    a.update(kw)
    return a


def numbers(a):
    """the restatement of items 5 and 7's integers -> dict(n_s, n_b, msf, Wd, hb, H, tmin, tmax)"""
    n, w, hop = pref.defaults(a["frame_length"], a["win_length"], a["hop"])
    sr = a["sample_rate"]
    n_s = int(math.ceil(1.0 / a["resolution"]))
    n_b = int(math.floor(12 * n_s * math.log2(a["fmax"] / a["fmin"]))) + 1
    msf = int(round(a["max_transition_rate"] * 12 * hop / sr))          # (Python's round: ties to even)
    wd = msf * n_s + 1
    tmin, tmax, _ = pref.lags(sr, a["fmin"], a["fmax"], n, w)
    return dict(n_s=n_s, n_b=n_b, msf=msf, Wd=wd, hb=wd // 2, N=n, W=w, H=hop, tmin=tmin, tmax=tmax)


# ---- the tables by librosa's construction ----
def triangle(m):
    """scipy.signal.windows.triang(m, sym=True), which get_window("triangle", m, fftbins=False) returns"""
    n = np.arange(1, (m + 1) // 2 + 1)
    if m % 2 == 0:
        w = (2 * n - 1.0) / m
        return np.r_[w, w[::-1]]
    w = 2 * n / (m + 1.0)
    return np.r_[w, w[-2::-1]]


def transition_local(n_states, width):
    """librosa.sequence.transition_local(n_states, width, window="triangle", wrap=False)"""
    t = np.zeros((n_states, n_states))
    for i in range(n_states):
        win = triangle(width)
        lpad = (n_states - width) // 2
        row = np.pad(win, (lpad, n_states - width - lpad))                 # util.pad_center
        row = np.roll(row, n_states // 2 + i + 1)
        row[min(n_states, i + width // 2 + 1):] = 0
        row[:max(0, i - width // 2)] = 0
        t[i] = row
    return t / t.sum(axis=1, keepdims=True)


def transition(n_b, width, switch_prob):
    """librosa.pyin's matrix: kron(transition_loop(2, 1 - switch_prob), transition_local) [2 n_b, 2 n_b]"""
    loop = np.array([[1.0 - switch_prob, switch_prob], [switch_prob, 1.0 - switch_prob]])
    return np.kron(loop, transition_local(n_b, width))


def beta_weights(nt, a, b):
    """np.diff(beta.cdf(theta, a, b)) for integers a, b: the binomial sum in exact rational arithmetic, rounded once"""
    n = a + b - 1
    cdf = []
    for i in range(nt + 1):
        x = Fraction(i, nt)
        cdf.append(sum(math.comb(n, j) * x ** j * (1 - x) ** (n - j) for j in range(a, n + 1)))
    return np.array([float(cdf[i] - cdf[i - 1]) for i in range(1, nt + 1)])


def boltzmann_pmf(k, lam, n):
    """scipy.stats.boltzmann.pmf"""
    return (1.0 - math.exp(-lam)) / (1.0 - math.exp(-lam * n)) * np.exp(-lam * np.asarray(k, dtype=np.float64))


def log_transition(t):
    """the definition's lt [2 n_b, 2 n_b] from the product's own tables t (api.pyin_tables): ltri - lZ + l_stay / l_sw where the
    window is positive, L0 elsewhere"""
    nb, hb = t["n_bins"], t["hb"]
    local = np.full((nb, nb), -np.inf)
    for d in range(-hb, hb + 1):
        i = np.arange(max(0, -d), min(nb, nb - d))
        local[i, i + d] = t["ltri"][d + hb] - t["lZ"][i]
    out = np.full((2 * nb, 2 * nb), L0)
    for a, la in ((0, t["l_stay"]), (1, t["l_sw"])):
        blk = np.where(np.isfinite(local), local + la, L0)
        out[:nb, a * nb:(a + 1) * nb] = blk
        out[nb:, (1 - a) * nb:(2 - a) * nb] = blk
    return out


# ---- the candidate stage (items 2 - 6) on a binary32 curve ----
def troughs(c, tmin, tmax):
    v = np.asarray(c)
    tau = np.arange(tmin + 1, tmax)
    is_t = (v[tau] < v[tau - 1]) & (v[tau] <= v[tau + 1])
    out = list(tau[is_t])
    if v[tmin] < v[tmin + 1]:
        out.insert(0, tmin)
    return np.array(out, dtype=np.int64)


def observe(c, tmin, tmax, t, no_trough_prob):
    """one frame's curve c (float32 [tmax + 1]) -> (O float32 [n_b], v float32, P float64 [n_b]: the binary64 value behind every
    entry, the number of troughs)"""
    c = np.asarray(c)
    assert c.dtype == np.float32
    nb, nt = t["n_bins"], t["n_thresholds"]
    o, p64 = np.zeros(nb, dtype=np.float32), np.zeros(nb)
    taus = troughs(c, tmin, tmax)
    if taus.size == 0:
        return o, np.float32(0.0), p64, 0
    h = c[taus]
    ij = np.searchsorted(t["theta"], h.astype(np.float64), side="right") + 1       # the least i with h < theta_i; nt + 1: none
    p = np.zeros(taus.size)
    for i in range(1, nt + 1):
        inb = ij <= i
        n_i = int(inb.sum())
        if n_i == 0:
            continue
        before = np.cumsum(inb) - inb
        p[inb] += t["w"][i - 1] * (t["G"][before[inb]] * t["cN"][n_i])
    g = int(np.argmin(h))                                                           # (the first of equal ones)
    p[g] += no_trough_prob * t["wsum"][ij[g] - 1]
    for j, tau in enumerate(taus):
        if p[j] == 0.0:
            continue
        delta = 0.0
        if tau > tmin:
            a, b, cc = float(c[tau - 1]), float(c[tau]), float(c[tau + 1])
            dd = (a - 2.0 * b) + cc
            if dd > 0.0:
                delta = (a - cc) / (2.0 * dd)
        period = float(tau) + delta
        b_j = int((period <= t["T"]).sum())
        if b_j == nb:
            continue
        o[b_j], p64[b_j] = np.float32(p[j]), p[j]
    s = 0.0
    for x in o[o != 0]:
        s += float(x)
    return o, np.float32(min(1.0, s)), p64, int(taus.size)


def check_observation(curve, got, t, tmin, tmax, no_trough_prob):
    """got: the product's mode-1 output [n_b + 1, F] of the curve [tmax + 1, F] (the product's own, binary32): positions, bins and
    the set of non-zero entries exact, v bit for bit, values within (nt + 3) 2^-53 P + max(2^-24 P, 2^-150) -> (worst error / bound, the most
    troughs a frame has)"""
    nb, nt = t["n_bins"], t["n_thresholds"]
    worst, most = 0.0, 0
    assert got.dtype == np.float32 and got.shape == (nb + 1, curve.shape[1])
    for f in range(curve.shape[1]):
        o, v, p64, n = observe(curve[:, f], tmin, tmax, t, no_trough_prob)
        most = max(most, n)
        g = got[:nb, f]
        assert np.array_equal(g != 0, o != 0), "frame %d: the non-zero entries lie at %s, the definition's at %s" % (
            f, np.flatnonzero(g).tolist(), np.flatnonzero(o).tolist())
        nz = o != 0
        # (one rounding to binary32: half an ulp, which is 2^-24 P for a normal result and 2^-150 below 2^-126, where the
        # format's spacing no longer shrinks with P -- there no correctly rounded value can meet 2^-24 P)
        bound = (nt + 3) * E * p64[nz] + np.maximum(U32 * p64[nz], 2.0 ** -150)
        err = np.abs(g[nz].astype(np.float64) - p64[nz])
        assert (err <= bound).all(), (f, float((err / bound).max()))
        if nz.any():
            worst = max(worst, float((err / bound).max()))
        # v is the definition's on the product's own entries, bit for bit
        s = 0.0
        for x in g[g != 0]:
            s += float(x)
        assert got[nb, f].tobytes() == np.float32(min(1.0, s)).tobytes(), (f, got[nb, f], s)
        assert not np.signbit(g).any()
    return worst, most


def undecided_frames(row, lead, a, f, curve32, t):
    """Against the binary64 chain from the audio row (section 20's curve intervals): a frame is undecided when a trough test,
    an i_j or a bin could turn within the intervals -> bool [f].  A decided frame's troughs, thresholds and bins are those of the
    binary64 curve, which the caller asserts through check_observation on curve32 plus the equality asserted here."""
    k = numbers(a)
    z = pref.frames(row, lead, k["N"], k["H"], f)
    energy = float((np.asarray(row, dtype=np.float64) ** 2).sum())
    tmin, tmax = k["tmin"], k["tmax"]
    und = np.zeros(f, dtype=bool)
    for i in range(f):
        if not z[i].any():
            assert (curve32[:, i] == 1.0).all()
            continue
        dp, bound = pref.curve(z[i], k["W"], tmax, energy)
        if not np.isfinite(bound[tmin:tmax + 1]).all():
            und[i] = True
            continue
        lo, hi = dp - bound, dp + bound
        tau = np.arange(tmin + 1, tmax)
        could = (lo[tau] < hi[tau - 1]) & (lo[tau] <= hi[tau + 1])
        sure = (hi[tau] < lo[tau - 1]) & (hi[tau] <= lo[tau + 1])
        if (could != sure).any() or ((lo[tmin] < hi[tmin + 1]) != (hi[tmin] < lo[tmin + 1])):
            und[i] = True
            continue
        taus = troughs(dp, tmin, tmax)
        if not np.array_equal(taus, troughs(curve32[:, i], tmin, tmax)):
            raise AssertionError("frame %d is decided, and the product's troughs are not the binary64 curve's" % i)
        for tau_j in taus:
            if np.searchsorted(t["theta"], lo[tau_j], side="right") != np.searchsorted(t["theta"], hi[tau_j], side="right"):
                und[i] = True
            if tau_j > tmin:
                per = []
                for sa in (-1, 1):
                    for sb in (-1, 1):
                        for sc in (-1, 1):
                            x, y, w = dp[tau_j - 1] + sa * bound[tau_j - 1], dp[tau_j] + sb * bound[tau_j], dp[tau_j + 1] + sc * bound[tau_j + 1]
                            dd = (x - 2.0 * y) + w
                            per.append(tau_j + (x - w) / (2.0 * dd) if dd > 0.0 else np.nan)
                if np.isnan(per).any() or int((min(per) * (1 - 4 * E) <= t["T"]).sum()) != int((max(per) * (1 + 4 * E) <= t["T"]).sum()):
                    und[i] = True
    return und


# ---- the path (items 7 - 9) ----
def log_observation(obs, t):
    """obs: mode 1's output [n_b + 1, F] (binary32) -> lo [F, 2 n_b]"""
    nb = t["n_bins"]
    o = obs[:nb].astype(np.float64).T
    v = obs[nb].astype(np.float64)
    u = (1.0 - v) / nb
    with np.errstate(divide="ignore"):
        lov = np.where(o != 0, np.log(np.where(o != 0, o, 1.0)), L0)
        lou = np.where(u > 0, np.log(np.where(u > 0, u, 1.0)), L0)
    return np.concatenate([lov, np.repeat(lou[:, None], nb, axis=1)], axis=1)


def epsilon(f):
    return f * (3 * C_LOG + 4) * E * abs(L0)


def decode(obs, t):
    """the definition's Viterbi on obs -> (best S, max-marginals [F, 2 n_b], lt, lo, lp0)"""
    nb = t["n_bins"]
    lt, lo = log_transition(t), log_observation(obs, t)
    f = lo.shape[0]
    lp0 = np.concatenate([np.full(nb, L0), np.full(nb, -math.log(nb))])
    fwd = np.empty((f, 2 * nb))
    fwd[0] = lp0 + lo[0]
    for i in range(1, f):
        fwd[i] = (fwd[i - 1][:, None] + lt).max(axis=0) + lo[i]
    bwd = np.zeros((f, 2 * nb))
    for i in range(f - 2, -1, -1):
        bwd[i] = (lt + (lo[i + 1] + bwd[i + 1])[None, :]).max(axis=1)
    return float(fwd[-1].max()), fwd + bwd, lt, lo, lp0


def score(path, lt, lo, lp0):
    """S(path), added in ascending f"""
    s = lp0[path[0]] + lo[0][path[0]]
    for i in range(1, len(path)):
        s = s + (lt[path[i - 1], path[i]] + lo[i][path[i]])
    return float(s)


def check_path(obs, planes, t, fill=float("nan"), use_bin=False):
    """planes: the product's mode-0 output [4, F] for the observation obs [n_b + 1, F] (the product's own mode-1 output): the
    score rule on every path, the max-marginal rule wherever the best state's margin exceeds 2 eps, planes 0, 1, 3 from the
    path's states and plane 2 the observation's v bit for bit -> (frames without the margin, S of the path, the best S)"""
    nb = t["n_bins"]
    f = obs.shape[1]
    assert planes.shape == (4, f) and planes.dtype == np.float32
    b = planes[3].astype(np.int64)
    assert (planes[3] == b).all() and (b >= 0).all() and (b < nb).all() and np.isin(planes[1], (0.0, 1.0)).all()
    voiced = planes[1] == 1.0
    path = np.where(voiced, b, nb + b)
    best, mm, lt, lo, lp0 = decode(obs, t)
    eps = epsilon(f)
    s = score(path, lt, lo, lp0)
    assert s >= best - eps, "S(device path) = %r, max S = %r, eps = %g" % (s, best, eps)
    top = np.sort(mm, axis=1)
    margin = top[:, -1] - top[:, -2]
    sure = margin > 2 * eps
    want = mm.argmax(axis=1)
    assert np.array_equal(path[sure], want[sure]), "frames %s: the state is not the decided one" % np.flatnonzero(sure & (path != want)).tolist()
    assert planes[2].tobytes() == obs[nb].tobytes(), "plane 2 is not the observation's v bit for bit"
    f0 = t["f0"][b]
    want0 = f0 if use_bin else np.where(voiced, f0, np.float32(fill)).astype(np.float32)
    assert want0.tobytes() == planes[0].tobytes() or (np.array_equal(np.isnan(want0), np.isnan(planes[0])) and
                                                       np.array_equal(want0[~np.isnan(want0)], planes[0][~np.isnan(want0)]))
    return int((~sure).sum()), s, best
