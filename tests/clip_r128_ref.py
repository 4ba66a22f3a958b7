"""True peak, short-term loudness and loudness range of clips (include/pdmp3_bulk.h pdmp3_amd_bulk_decode_clips_r128; DESIGN.md
section 19) in binary64 with numpy, on top of tests/clip_loudness_ref.py: the interpolator restated, the definition as plain
convolutions and sorts, the derived bounds of the device's binary32 products evaluated from the reference's own quantities, and
the rule for clips whose range gates are undecided.  Shared by tests/test_clip_r128_host.py and tests/test_gpu_clip_r128.py."""
import math

import numpy as np

import clip_loudness_ref as lref

U = lref.U
N_CHAIN = 28               # fused multiply-adds of a phase output's chain: 7 steps of 4, whatever the band leaves zero
WINDOW, EVERY, MAX_RANGE = 30, 10, 4096
SUM_ABS = (1.0, 1.63118, 1.86418, 1.63118)


def _kweight_blocks(x, fs, state=None, states_every=0):
    """clip_loudness_ref.kweight's sample loop run by scipy.signal.lfilter (the same transposed direct form II, in C): the rows
    of the device tests are hundreds of thousands of samples long.  tests/test_clip_loudness_host.py holds the two to 1e-12"""
    from scipy.signal import lfilter
    (b1, a1), (b2, a2) = lref.coefficients(fs)
    x = np.asarray(x, dtype=np.float64)
    lead = x.shape[:-1]
    s = np.zeros(lead + (4,)) if state is None else np.array(state, dtype=np.float64).reshape(lead + (4,))
    z1, z2 = s[..., :2].copy(), s[..., 2:].copy()
    T = x.shape[-1]
    y = np.empty_like(x)
    kept = []
    step = states_every or max(T, 1)
    for t0 in range(0, T, step):
        kept.append(np.concatenate([z1, z2], axis=-1))
        v, z1 = lfilter(b1, a1, x[..., t0:t0 + step], axis=-1, zi=z1)
        y[..., t0:t0 + step], z2 = lfilter(b2, a2, v, axis=-1, zi=z2)
    if states_every:
        return y, (np.stack(kept, axis=-2) if kept else np.zeros(lead + (0, 4)))
    return y


def _loudness_measure(*args):
    """clip_loudness_ref.measure, with the sample loop in C where scipy is there"""
    try:
        import scipy.signal  # noqa: F401
    except ImportError:
        return lref.measure(*args)
    loop = lref.kweight
    lref.kweight = _kweight_blocks
    try:
        return lref.measure(*args)
    finally:
        lref.kweight = loop


def taps():
    """h[49]: libebur128's interpolator at factor 4"""
    h = np.zeros(49)
    for j in range(49):
        m = j - 24
        c = (1.0 if m == 0 else math.sin(m * math.pi / 4.0) / (m * math.pi / 4.0)) * 0.5 * (1.0 - math.cos(2.0 * math.pi * j / 48.0))
        h[j] = 0.0 if abs(c) < 1e-6 else c
    return h


def phases():
    """c[4][12]: c_p[d] = h[4 d + p] (phase 0's thirteenth tap h[48] is 0)"""
    h = taps()
    return np.array([[h[4 * d + p] for d in range(12)] for p in range(4)])


def plan(fs, n_samples):
    p = lref.plan(fs, n_samples)
    p["Js"] = max(0, p["I"] - (WINDOW - 1))
    p["Jr"] = (p["Js"] + EVERY - 1) // EVERY
    p["Jsmax"] = p["Js"]
    return p


def hi_index(n):
    return (19 * (n - 1) + 10) // 20


def lo_index(n):
    return (n + 4) // 10


def oversample(x, cuts=()):
    """x [C, T] -> (y [C, T, 4], e [C, T, 4]): y_c[4 t + p] = sum_d c_p[d] x_c[t - d] from rest, and the bound of the device's
    binary32 chain for it, (N u / (1 - N u) + u) sum_d |c_p[d]| |x_c[t - d]|.  cuts: sample positions at which the history is
    thrown away (what a kernel that forgot the samples in front of a wave or a chunk would compute)"""
    x = np.asarray(x, dtype=np.float64)
    C, T = x.shape
    c = phases()
    y, a = np.zeros((C, T, 4)), np.zeros((C, T, 4))
    edges = [0] + sorted(b for b in cuts if 0 < b < T) + [T]
    for ch in range(C):
        for lo, hi in zip(edges[:-1], edges[1:]):
            for p in range(4):
                y[ch, lo:hi, p] = np.convolve(x[ch, lo:hi], c[p])[:hi - lo]
                a[ch, lo:hi, p] = np.convolve(np.abs(x[ch, lo:hi]), np.abs(c[p]))[:hi - lo]
    return y, (N_CHAIN * U / (1.0 - N_CHAIN * U) + U) * a


def true_peak(x, cuts=()):
    """-> (TP, its bound, the place (c, t, p) of the largest |y|)"""
    if x.shape[1] == 0:
        return 0.0, 0.0, (0, 0, 0)
    y, e = oversample(x, cuts)
    at = np.unravel_index(int(np.argmax(np.abs(y))), y.shape)
    return float(np.abs(y).max()), float(e.max()), tuple(int(i) for i in at)


def measure(x, fs, dual_mono=False, target=None, peak_limit=0.0, limit_true_peak=True):
    """x [C, T]: binary32 values -> clip_loudness_ref.measure's numbers and bounds with, on top, TP / dTP, the short-term curve S /
    dS, Smax / dSmax, the range's Gamma_r / dGamma_r, counts, LRA / dLRA, r_undecided and r_margin (dB) / r_margin_bounds (the
    smallest distance of a window of the range to one of its gates, in dB and in bounds), and the gain under the peak PM."""
    x = np.asarray(x)
    C, T = x.shape
    m = _loudness_measure(x, fs, dual_mono, None if limit_true_peak else target, 0.0 if limit_true_peak else peak_limit)
    p = plan(fs, T)
    q, Js, Jr = p["q"], p["Js"], p["Jr"]
    m.Js, m.Jr = Js, Jr
    m.TP, m.dTP, m.tp_at = true_peak(x)
    m.TP = max(m.TP, m.P)
    G = np.ones(C)
    if dual_mono:
        G[0] = 2.0
    w = np.array([(G[:, None] * m.s[:, j:j + WINDOW]).sum() for j in range(Js)]) / (WINDOW * q)
    ew = np.array([(G[:, None] * m.es[:, j:j + WINDOW]).sum() for j in range(Js)]) / (WINDOW * q)
    m.w, m.ew = w, ew
    m.S, m.dS = lref._l(w), lref._dl(w, ew)
    m.Smax = float(m.S.max()) if Js else -np.inf
    if Js and np.isfinite(m.Smax):
        jm = int(np.argmax(m.S))
        m.dSmax = float(m.dS[m.S + m.dS >= m.Smax - m.dS[jm]].max())
    else:
        m.dSmax = 0.0
    # the range
    R = np.arange(0, Js, EVERY)
    wr, er, Sr = w[R], ew[R], m.S[R]
    lo, hi = lref._l(np.maximum(wr - er, 0.0)), lref._l(wr + er)
    undecided = bool(((lo <= -70.0) & (hi > -70.0)).any()) if Jr else False
    dist, bounds = [np.inf], [np.inf]
    if Jr:
        d = np.minimum(np.abs(lo + 70.0), np.abs(hi + 70.0))
        dist.append(float(d.min()))
        dr = lref._dl(wr, er)                           # (inf next to silence: such a window is decided by its interval's upper end)
        with np.errstate(divide="ignore", invalid="ignore"):
            b = np.where(np.isfinite(Sr) & np.isfinite(dr), np.abs(Sr + 70.0) / np.maximum(dr, 1e-300), np.inf)
        bounds.append(float(b.min()))
    inA = Sr > -70.0
    m.nAr = int(inA.sum())
    m.LRA, m.dLRA, m.nGr = 0.0, 0.0, 0
    if m.nAr:
        m.gamma_r = float(lref._l(wr[inA].mean()) - 20.0)
        m.dgamma_r = float(lref._dl(wr[inA].mean(), er[inA].mean()))
        undecided |= bool(((lo[inA] <= m.gamma_r + m.dgamma_r) & (hi[inA] >= m.gamma_r - m.dgamma_r)).any())
        dist.append(float(np.minimum(np.abs(lo[inA] - m.gamma_r), np.abs(hi[inA] - m.gamma_r)).min() - m.dgamma_r))
        bounds.append(float((np.abs(Sr[inA] - m.gamma_r) / (lref._dl(wr[inA], er[inA]) + m.dgamma_r)).min()))
        inG = inA & (Sr > m.gamma_r)
        m.nGr = n = int(inG.sum())
        if n:
            v = np.sort(Sr[inG])
            m.LRA = float(v[hi_index(n)] - v[lo_index(n)])
            m.dLRA = 2.0 * float(lref._dl(wr[inG], er[inG]).max())
    else:
        m.gamma_r, m.dgamma_r = -np.inf, 0.0
    m.r_undecided = bool(undecided)
    m.r_margin, m.r_margin_bounds = float(min(dist)), float(min(bounds))
    # the gain under PM = TP
    m.PM = m.TP if limit_true_peak else m.P
    m.tp_limited = False
    if limit_true_peak:
        if target is None or not np.isfinite(m.L):
            m.g, m.dg = 1.0, 0.0
        else:
            g = 10.0 ** ((target - m.L) / 20.0)
            dg = g * (10.0 ** (m.dL / 20.0) - 1.0) + 2.0 * U * g
            if peak_limit > 0.0:
                if abs(g * m.TP - peak_limit) <= dg * m.TP + g * m.dTP:
                    m.undecided = True
                if g * m.TP > peak_limit:
                    m.tp_limited = True
                    g = peak_limit / m.TP
                    dg = (peak_limit * m.dTP / (m.TP * (m.TP - m.dTP)) if m.dTP < m.TP else np.inf) + 2.0 * U * g
            m.g, m.dg = g, dg
    return m


def check_stats(m, stats, momentary=None, short_term=None):
    """the device's stats row [16] (and momentary, short-term rows) against the reference m -> the worst error / bound met;
    AssertionError on a miss.  A clip whose loudness gates or gain are undecided is held in fields 0-7 as clip_loudness_ref holds
    it; one whose range gates are undecided is not held to LRA, Gamma_r, |Ar|, |Gr|.  TP, Smax, the short-term curve, Js and Jr
    hold for every clip."""
    stats = np.asarray(stats, dtype=np.float64)
    assert stats.shape == (16,)
    first = stats[:8].copy()
    worst = 0.0

    def near(got, want, bound, what):
        nonlocal worst
        if not np.isfinite(want):
            assert got == want, (what, got, want)
            return
        b = bound + abs(want) * 2.0 ** -23
        assert abs(got - want) <= b, (what, got, want, b)
        if b > 0.0:
            worst = max(worst, abs(got - want) / b)

    if m.tp_limited and not m.undecided:               # (held to the true peak: within TP's bound, not an exact quotient)
        near(stats[3], m.g, m.dg, "g")
        first[3] = np.float32(m.g)
        was = (m.limited, m.dg)
        m.limited, m.dg = True, 0.0
        worst = max(worst, lref.check_stats(m, first, momentary))
        m.limited, m.dg = was
    else:
        worst = max(worst, lref.check_stats(m, first, momentary))
    assert stats[12] == m.Js and stats[13] == m.Jr, ("Js, Jr", stats[12:14], m.Js, m.Jr)
    assert stats[8] >= stats[2], ("TP < P", stats[8], stats[2])
    near(stats[8], m.TP, m.dTP, "TP")
    near(stats[9], m.Smax, m.dSmax, "Smax")
    if short_term is not None:
        st = np.asarray(short_term, dtype=np.float64)
        assert st.shape == (m.Js,)
        for j in range(m.Js):
            if m.ew[j] < 0.5 * m.w[j]:
                near(st[j], m.S[j], m.dS[j], "S[%d]" % j)
            else:                                      # (next to silence: no more than the bound allows)
                assert st[j] <= float(lref._l(m.w[j] + m.ew[j])) + 1e-5, ("S[%d]" % j, st[j], m.w[j], m.ew[j])
    if m.r_undecided:
        return worst
    assert stats[14] == m.nAr and stats[15] == m.nGr, ("range counts", stats[14:16], m.nAr, m.nGr)
    near(stats[11], m.gamma_r, m.dgamma_r, "Gamma_r")
    near(stats[10], m.LRA, m.dLRA, "LRA")
    return worst


LEAD_SECONDS = 2


def measure_from(x, fs, t0, lead=LEAD_SECONDS, dual_mono=False):
    """measure()'s momentary and short-term values and their bounds for the windows that begin at or behind sample t0 of
    x [C, T], from x[:, a:] alone with the filters started from rest at a = the last multiple of q at least `lead` seconds in
    front of the first such window (0 where the row is shorter).  The K-weighting's memory decays: at 8 kHz a start from rest
    0.5 s before is bit-equal in binary64 to the full run, at 48 kHz it agrees to 2e-13 of max |y| after 0.5 s and is
    bit-equal after 2 s (tests/test_clip_r128_host.py holds this helper to 1e-12 of measure() behind a loud history).  The
    bounds are the cut row's: all of measure()'s terms but the states' binary64 chain are local to a block, and that one is
    proportional to max |x| of the cut row alone -- a rounding committed in front of the cut decays as the states do.
    -> (j0, m): the first window is number j0 of the whole row's, m.l / m.dl / m.z / m.ez and m.S / m.dS / m.w / m.ew are cut
    to the windows j0, j0 + 1, ... of the whole row (m.J, m.Js: how many); the other fields of m speak of the cut row"""
    x = np.asarray(x)
    q = (fs + 5) // 10
    j0 = (int(t0) + q - 1) // q
    a = max(0, j0 - (int(lead * fs) + q - 1) // q) * q
    m = measure(x[:, a:], fs, dual_mono)
    k = j0 - a // q
    m.l, m.dl, m.z, m.ez = m.l[k:], m.dl[k:], m.z[k:], m.ez[k:]
    m.S, m.dS, m.w, m.ew = m.S[k:], m.dS[k:], m.w[k:], m.ew[k:]
    m.J, m.Js = len(m.l), len(m.S)
    return j0, m


def check_curves_from(j0, m, momentary, short_term):
    """the tails of a call's momentary and short-term rows from window j0 on against measure_from's m, as check_stats holds the
    whole rows -> the worst error / bound met"""
    worst = 0.0
    for name, row, val, dval, z, ez in (("l", momentary, m.l, m.dl, m.z, m.ez), ("S", short_term, m.S, m.dS, m.w, m.ew)):
        got = np.asarray(row, dtype=np.float64)[j0:]
        assert got.shape == val.shape, (name, got.shape, val.shape)
        for j in range(len(val)):
            if ez[j] < 0.5 * z[j]:
                b = dval[j] + abs(val[j]) * 2.0 ** -23
                assert abs(got[j] - val[j]) <= b, ("%s[%d]" % (name, j0 + j), got[j], val[j], b)
                worst = max(worst, abs(got[j] - val[j]) / b)
            else:
                assert got[j] <= float(lref._l(z[j] + ez[j])) + 1e-5, ("%s[%d]" % (name, j0 + j), got[j], z[j], ez[j])
    return worst


def gates_on_curves(momentary, short_term):
    """The gated numbers of a call from its own curves: the momentary row and the short-term row as the call stores them
    (binary32 dB values) -> a Measured with L / dL, gamma / dgamma, nA, nGt, undecided (clip_loudness_ref.curve_gates on the
    momentary row: relative gate -10) and gamma_r / dgamma_r, nAr, nGr, LRA / dLRA, r_undecided, Jr (the same on every tenth
    short-term value: relative gate -20), margin_bounds.  What a call's stats must be where the curves are right: it is the
    check of a clip too long for measure().

    The bounds of L, Gamma and Gamma_r are curve_gates' (derived there from the rows' rounding alone, |dl| <= 2^-24 |l|).
    LRA = v_(hi) - v_(lo), two order statistics of the gated values v_i, of which the row holds v'_i with |v'_i - v_i| <= d_i.
    An order statistic is monotone in every value, so the k-th smallest of the v_i lies between the k-th smallest of the
    v'_i - d_i and the k-th smallest of the v'_i + d_i -- the spread of the values whose rank can change, and d_k itself where
    no neighbour is that near.  dLRA is the sum of the two statistics' largest distances from v'_(hi) and v'_(lo)."""
    g = lref.curve_gates(momentary)
    m = lref.Measured()
    m.L, m.dL, m.gamma, m.dgamma, m.nA, m.nGt, m.undecided = g.level, g.dlevel, g.gamma, g.dgamma, g.n_abs, g.n_rel, g.undecided
    r = lref.curve_gates(short_term, every=EVERY, relative=-20.0)
    m.Jr = len(r.values)
    m.gamma_r, m.dgamma_r, m.nAr, m.nGr, m.r_undecided = r.gamma, r.dgamma, r.n_abs, r.n_rel, r.undecided
    m.LRA, m.dLRA = 0.0, 0.0
    if m.nGr:
        v, d = r.values[r.inside], r.dv[r.inside]
        mid, dn, up = np.sort(v), np.sort(v - d), np.sort(v + d)
        hi, lo = hi_index(m.nGr), lo_index(m.nGr)
        m.LRA = float(mid[hi] - mid[lo])
        m.dLRA = float(max(up[hi] - mid[hi], mid[hi] - dn[hi]) + max(up[lo] - mid[lo], mid[lo] - dn[lo]))
    m.margin_bounds = min(g.margin_bounds, r.margin_bounds)
    return m


def check_stats_on_curves(g, stats):
    """the call's stats row [16] against gates_on_curves' g -> the worst error / bound met; the counts are exact"""
    stats = np.asarray(stats, dtype=np.float64)
    assert not g.undecided and not g.r_undecided
    assert (stats[6], stats[7], stats[13], stats[14], stats[15]) == (g.nA, g.nGt, g.Jr, g.nAr, g.nGr), (stats[[6, 7, 13, 14, 15]], g.nA, g.nGt, g.Jr, g.nAr, g.nGr)
    worst = 0.0
    for got, want, bound, what in ((stats[0], g.L, g.dL, "L"), (stats[4], g.gamma, g.dgamma, "Gamma"), (stats[11], g.gamma_r, g.dgamma_r, "Gamma_r"),
                                   (stats[10], g.LRA, g.dLRA, "LRA")):
        if not np.isfinite(want):
            assert got == want, (what, got, want)
            continue
        b = bound + abs(want) * 2.0 ** -23            # (the value's own rounding to binary32)
        assert abs(got - want) <= b, (what, got, want, b)
        if b > 0.0:
            worst = max(worst, abs(got - want) / b)
    return worst
