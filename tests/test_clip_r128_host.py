"""True peak, short-term loudness and loudness range of clips on the host, no GPU: the interpolator's taps
against the definition and the reference's restatement, the reference against scipy's polyphase filter and Tech 3341's sines,
the range's two indices against libebur128's binary64 expressions, the refusals of the planning calls, and the kernels' own
indexing and arithmetic (pdmp3_amd/csrc/loudness_core.h and r128_core.h, compiled here with g++ into
tests/host_emul/r128_emul.cpp's loops) against the binary64 definition within the derived bound -- with limit_true_peak = 0 bit
for bit what the loudness call's emulation gives."""
import ctypes as C
import functools

import numpy as np
import pytest

import clip_loudness_ref as lref
import clip_r128_ref as ref
import test_clip_cqt_host as tch
import test_clip_loudness_host as tlh
from clip_host import build_emul, run_sanitizer_program

RATES = [8000, 22050, 48000]


class R128Params(C.Structure):                     # include/pdmp3_hip.h pdmp3_r128_params
    _fields_ = [("loud", tlh.LoudParams), ("n_st", C.c_int32), ("n_rng", C.c_int32), ("limit_true_peak", C.c_int32), ("reserved", C.c_int32)]


def _api():
    from pdmp3_amd import api
    return api


def _emul():
    lib = build_emul("r128")
    lib.emul_clip_r128.argtypes = [C.c_void_p] + [C.c_int] + [C.c_void_p] * 6
    lib.emul_clip_loudness.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.emul_r128_indices.argtypes = [C.c_longlong, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    assert lib.emul_r128_params_bytes() == C.sizeof(R128Params)
    return lib


def emulate(x, fs, dual_mono=False, target=None, peak_limit=0.0, limit_true_peak=True, loudness_call=False):
    """x float32 [C, T] -> (audio [C, T], stats [16], momentary [J], short-term [Js]) of the emulated kernels; loudness_call: the
    loudness call's emulation in the same library (stats [8], no short-term)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    Cn, T = x.shape
    b, chunk, lds, q, nc, I, J, Js, Jr, Jsmax = _api().r128_plan(fs, T)
    assert Jsmax == Js
    L = tlh.LoudParams(T, Cn, q, nc, I, J, int(dual_mono), float("nan") if target is None else target, peak_limit)
    P = R128Params(L, Js, Jr, int(limit_true_peak), 0)
    Ts = (T + 3) & ~3
    src = np.full((Cn, Ts), 7e29, dtype=np.float32)               # (the floats behind a row's end are not the kernel's to read)
    src[:, :T] = x
    out = np.full((Cn, T + 8), -5.0, dtype=np.float32)
    d = tch.MelDesc(src.ctypes.data, out.ctypes.data, Ts, T + 8, 0, 0)
    n = 8 if loudness_call else 16
    stats, mom, st = np.full(n + 2, -5.0, dtype=np.float32), np.full(J + 2, -5.0, dtype=np.float32), np.full(Js + 2, -5.0, dtype=np.float32)
    tab = tlh._tables_blob(fs)
    if loudness_call:
        assert _emul().emul_clip_loudness(C.byref(d), 1, tab.ctypes.data, C.byref(L), stats.ctypes.data, mom.ctypes.data) == 0
    else:
        taps = _api().r128_taps()[1]
        assert _emul().emul_clip_r128(C.byref(d), 1, tab.ctypes.data, taps.ctypes.data, C.byref(P), stats.ctypes.data, mom.ctypes.data, st.ctypes.data) == 0
    assert (out[:, T:] == -5.0).all() and (stats[n:] == -5.0).all() and (mom[J:] == -5.0).all() and (st[Js:] == -5.0).all()
    return out[:, :T].copy(), stats[:n].copy(), mom[:J].copy(), st[:Js].copy()


# ---- 1. the taps ----
def test_the_taps():
    h, ph = _api().r128_taps()
    want = ref.taps()
    assert np.abs(h - want).max() <= 1e-15
    assert int((h != 0).sum()) == 37 and h[24] == 1.0
    assert (h[0::4] == np.eye(13)[6]).all(), "phase 0 is not a pure delay of 6 samples"
    c = ref.phases()
    for p in range(4):
        assert abs(np.abs(c[p]).sum() - ref.SUM_ABS[p]) <= 1e-5
    assert np.abs(c.sum(axis=1) - np.array([1.0, 1.00048, 1.00090, 1.00048])).max() <= 1e-5
    assert ph.dtype == np.float32 and ph.shape == (3, 12) and (ph == c[1:].astype(np.float32)).all()
    assert (np.abs(ph).sum(axis=1) > 1.6).all()
    # m = +-4 k: the sinc's zeros come out as rounding noise and are cut to exact zeros
    assert (h[[4, 8, 12, 16, 20, 28, 32, 36, 40, 44]] == 0).all()


# ---- 2. the reference ----
def test_the_reference_is_scipys_upfirdn():
    sig = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(7)
    x = rng.standard_normal((2, 501))
    y, _ = ref.oversample(x)
    for c in range(2):
        want = sig.upfirdn(ref.taps(), x[c], 4)[:4 * 501]
        assert np.abs(y[c].reshape(-1) - want).max() <= 1e-13


def test_tech_3341_sines():
    fs = 48000
    t = np.arange(fs // 2)
    x = np.sin(2.0 * np.pi * t / 4.0 + np.pi / 4.0)[None, :].astype(np.float32)      # fs / 4, 45 degrees: the samples miss the crests
    tp, _, _ = ref.true_peak(x)
    assert abs(np.abs(x).max() - 0.7071) <= 1e-4
    db = 20.0 * np.log10(tp)
    assert -0.4 <= db <= 0.2, db
    print("fs / 4 at 45 degrees: P %.4f, TP %.4f (%.2f dBTP)" % (np.abs(x).max(), tp, db))
    x = np.sin(2.0 * np.pi * 5000.0 * t / fs)[None, :].astype(np.float32)
    tp, _, _ = ref.true_peak(x)
    assert 0.0 <= 20.0 * np.log10(max(tp, np.abs(x).max()) / np.abs(x).max()) < 0.01


def test_the_percentile_indices_are_libebur128s():
    lib = _emul()
    hi, lo = C.c_longlong(0), C.c_longlong(0)
    for n in range(1, 10001):
        lib.emul_r128_indices(n, C.byref(hi), C.byref(lo))
        assert hi.value == int((n - 1) * 0.95 + 0.5) == ref.hi_index(n) and lo.value == int((n - 1) * 0.1 + 0.5) == ref.lo_index(n), n
        assert 0 <= lo.value <= hi.value < n


def test_the_plan_is_the_restatement():
    for fs in RATES + [44100, 192000]:
        q = (fs + 5) // 10
        for T in (0, 1, 30 * q - 1, 30 * q, 40 * q + 35, 39 * q + 5, 123457):
            got = _api().r128_plan(fs, T)
            want = ref.plan(fs, T)
            assert got == (want["B"], want["chunk"], want["lds_bytes"], want["q"], want["n_chunks"], want["I"], want["J"], want["Js"], want["Jr"], want["Jsmax"])
            assert got[:7] == _api().loudness_plan(fs, T)


# ---- 3. the emulation within the bound ----
def _check(x, fs, **kw):
    m = ref.measure(x, fs, **kw)
    audio, stats, mom, st = emulate(x, fs, **kw)
    worst = ref.check_stats(m, stats, mom, st)
    assert (audio.view(np.uint32) == (x * np.float32(stats[3])).astype(np.float32).view(np.uint32)).all()
    return m, stats, worst


IMPULSES = [0, 5, 11, 63, 1023, 1024, 1029, 4095, 4096, 4101]


def test_an_impulse_at_every_history_path():
    """T % 4 != 0; a single impulse never overshoots (every |c_p[d]| < 1): TP = P exactly, whatever the history path"""
    fs, T = 8000, 5127
    assert T % 4
    for t0 in IMPULSES + [T - 1]:
        x = np.zeros((1, T), dtype=np.float32)
        x[0, t0] = -0.9
        m, stats, _ = _check(x, fs)
        assert stats[8] == stats[2] == np.float32(0.9) and m.TP == m.P


def test_a_pair_across_every_history_path():
    """two equal samples side by side overshoot between them (TP > 1.1 P); the interpolated maximum lies six samples behind
    them, in the next block, wave or chunk, and needs the first of them from the history.  Forgetting the history at that
    boundary moves TP by far more than four bounds"""
    fs, T = 8000, 5127
    worst = 0.0
    for t0 in (5, 63, 1023, 4095, 1087, T - 3, T - 2):
        x = np.zeros((1, T), dtype=np.float32)
        x[0, t0] = x[0, t0 + 1] = 0.8
        m, stats, w = _check(x, fs)
        worst = max(worst, w)
        if t0 + 7 < T:
            assert m.TP > 1.1 * m.P and m.tp_at[1] > t0 + 1
            cut, _, _ = ref.true_peak(x, cuts=(t0 + 1,))
            assert m.TP - max(cut, m.P) > 4.0 * m.dTP
        else:                                                    # (no flush behind T: the overshoot is never reached)
            assert m.TP < 1.1 * m.P
    assert 0.0 < worst <= 1.0
    print("pairs: worst error / bound %.3g" % worst)


@pytest.mark.parametrize("kind", ["noise", "sine", "silence"])
def test_signals_within_the_bound(kind):
    fs = 8000
    T = 40 * 800 + 35
    for Cn in (1, 2):
        x = tlh._signal(kind, Cn, T, fs, 21 + Cn)
        m, stats, worst = _check(x, fs)
        print("%s C=%d: TP %.4f P %.4f Smax %.3f LRA %.3f worst error / bound %.3g" % (kind, Cn, m.TP, m.P, m.Smax, m.LRA, worst))
        if kind == "silence":
            assert (stats[8:] == np.array([0, -np.inf, 0, -np.inf, m.Js, m.Jr, 0, 0], dtype=np.float32)).all()
        else:
            assert 0.0 < worst <= 1.0 and not m.r_undecided and stats[8] >= stats[2] and m.nGr == m.Jr == 2


@pytest.mark.parametrize("fs", RATES)
def test_lengths_channels_and_rates(fs):
    q = (fs + 5) // 10
    for i, (T, Cn, dual) in enumerate([(30 * q - 1, 1, False), (30 * q, 2, False), (40 * q + 35, 1, True), (40 * q + 35, 2, False)]):
        x = tlh._signal("noise", Cn, T, fs, 300 + i)
        m, stats, worst = _check(x, fs, dual_mono=dual)
        assert stats[12] == max(0, T // q - 29) and stats[13] == (stats[12] + 9) // 10 and 0.0 < worst <= 1.0
        if T < 30 * q:
            assert (stats[8:] == np.array([stats[8], -np.inf, 0, -np.inf, 0, 0, 0, 0], dtype=np.float32)).all() and stats[8] > 0
        else:
            assert not m.r_undecided and np.isfinite(stats[9])
        if dual:
            mono = ref.measure(x, fs)
            assert abs(float(stats[9]) - (mono.Smax + 10.0 * np.log10(2.0))) <= m.dSmax + 2e-6 * abs(m.Smax)


def _segments(fs, seconds, levels_db, seed):
    """noise in segments of equal length at the levels given"""
    rng = np.random.default_rng(seed)
    T = int(seconds * fs)
    x = 0.5 * rng.standard_normal((1, T))
    edges = np.linspace(0, T, len(levels_db) + 1).astype(int)
    for lo, hi, db in zip(edges[:-1], edges[1:], levels_db):
        x[:, lo:hi] *= 10.0 ** (db / 20.0)
    return np.clip(x, -1.0, 1.0).astype(np.float32)


def test_a_range_of_five_segments():
    """14 s of five segments 10 dB apart: twelve windows a second apart, the relative gate of the range takes the quietest"""
    fs = 8000
    x = _segments(fs, 14.0, [-50, -40, -30, -20, -10], 5)
    m, stats, worst = _check(x, fs)
    assert m.Jr == 12 and m.nAr == 12 and 0 < m.nGr < 12 and ref.hi_index(m.nGr) != ref.lo_index(m.nGr)
    assert m.LRA > 10.0 and not m.r_undecided and m.r_margin_bounds > 10.0 and 0.0 < worst <= 1.0
    print("five segments: Jr %d |Ar| %d |Gr| %d LRA %.3f Gamma_r %.3f margin %.3g dB = %.3g bounds" %
          (m.Jr, m.nAr, m.nGr, m.LRA, m.gamma_r, m.r_margin, m.r_margin_bounds))


def test_a_silent_tail_is_gated_out_of_the_range():
    fs = 8000
    x = _segments(fs, 16.0, [-20, -14, -20, -26], 6)
    x[:, -3 * fs - 400:] = 0.0
    m, stats, worst = _check(x, fs)
    assert m.nAr < m.Jr and not m.r_undecided and 0.0 < worst <= 1.0
    assert m.S[-1] < -100.0 and stats[14] == m.Jr - 1     # (the filters' decay alone is in the last window)


# ---- 3b. more than 256 blocks, windows and range values: every stride loop of k_loud_gate makes a second trip ----
DRAWN_DB = (-12, -18, -24, -30, -36, -42, -80)         # of noise with sigma 0.5: the last one lies under the absolute gate
LONG = {
    # name: (seconds, channels, seed) at 8000 Hz -- the seeds were chosen on the reference alone (both gates of the range bite,
    # nothing undecided, every window of the range more than 10 bounds from its gates)
    "27s-mono": (27.0, 1, 2705),
    "27s-stereo": (27.0, 2, 2751),
    "300s-mono": (300.05, 1, 30005),
}


def _drawn_segments(fs, seconds, Cn, seed):
    """noise in segments of 3 .. 5 s end to end, each at a level drawn from DRAWN_DB"""
    rng = np.random.default_rng(seed)
    T = int(round(seconds * fs))
    x = 0.5 * rng.standard_normal((Cn, T))
    t = 0
    while t < T:
        n, db = int(rng.integers(3 * fs, 5 * fs + 1)), DRAWN_DB[int(rng.integers(len(DRAWN_DB)))]
        x[:, t:t + n] *= 10.0 ** (db / 20.0)
        t += n
    return np.clip(x, -1.0, 1.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _long_case(name):
    """(x, the reference, the emulation's (audio, stats, momentary, short-term)) -- made once"""
    seconds, Cn, seed = LONG[name]
    x = _drawn_segments(8000, seconds, Cn, seed)
    return x, ref.measure(x, 8000), emulate(x, 8000)


@pytest.mark.parametrize("name", sorted(LONG))
def test_more_than_256_blocks_windows_and_range_values(name):
    """27 s: J = 267 and Js = 241, n_sub = 270 -- the loops over the sub-blocks and the momentary blocks (both passes) make a
    second trip, in threads 0 .. 13 alone; 300.05 s: Jr = 298 and 586 chunks, so the loops over the waves' partial peaks, the
    short-term windows (twelve trips), the gated range values and the ranking do too, and the chain takes ten steps.  Every
    field and both curves against the binary64 definition"""
    x, m, (audio, stats, mom, st) = _long_case(name)
    worst = ref.check_stats(m, stats, mom, st)
    print("%s: J %d Js %d Jr %d |A| %d |Gt| %d |Ar| %d |Gr| %d L %.3f LRA %.3f worst error / bound %.3g, range margin %.3g dB = %.3g bounds" %
          (name, m.J, m.Js, m.Jr, m.nA, m.nGt, m.nAr, m.nGr, m.L, m.LRA, worst, m.r_margin, m.r_margin_bounds))
    n_chunks = ref.plan(8000, x.shape[1])["n_chunks"]
    assert m.J > 256 and ((m.Jr > 256 and m.Js > 256 and n_chunks > 64 * 9) if name.startswith("300s") else (m.J, m.Js) == (267, 241))
    assert 0 < m.nGr < m.nAr < m.Jr and 0 < m.nGt < m.nA < m.J
    assert 0.0 < worst <= 1.0 and not m.undecided and not m.r_undecided and m.r_margin_bounds > 10.0
    assert (audio.view(np.uint32) == (x * np.float32(stats[3])).astype(np.float32).view(np.uint32)).all()
    assert stats[8] >= stats[2] == np.abs(x).max()


def test_a_shorter_clip_is_a_prefix_of_the_longer_one():
    """the 300 s signal cut to 27 s and five samples: its momentary and short-term rows are the first values of the long
    clip's rows, bit for bit -- every sum has one fixed order, nothing behind a block enters it, and the scans hand states
    upwards only"""
    x, m, (audio, stats, mom, st) = _long_case("300s-mono")
    _, s2, mom2, st2 = emulate(x[:, :27 * 8000 + 5], 8000)
    assert (len(mom2), len(st2)) == (267, 241) and np.isfinite(mom2).any() and s2[13] == 25
    assert (mom2.view(np.uint32) == mom[:267].view(np.uint32)).all() and (st2.view(np.uint32) == st[:241].view(np.uint32)).all()


# ---- 3c. the helpers of the device tests of long clips ----
def test_measure_from_is_measure_behind_a_loud_history():
    """12 s at 8000 and 48 000 Hz stereo: 6 s near full scale, then 40 dB less.  The windows from 8 s on (t0 not a multiple of
    q), from a restart 2 s in front of them, against the whole run's: 1e-12 relative, the bar of the lfilter pin"""
    for fs in (8000, 48000):
        q = (fs + 5) // 10
        x = tlh._signal("noise", 2, 12 * fs + 77, fs, 12)
        x[:, :6 * fs] *= np.float32(8.0)
        x[:, 6 * fs:] *= np.float32(0.08)
        m = ref.measure(x, fs)
        t0 = 8 * fs - q // 3
        j0, c = ref.measure_from(x, fs, t0)
        assert j0 == 80 and (j0 - 1) * q < t0 <= j0 * q and c.J == m.J - j0 > 30 and c.Js == m.Js - j0 > 5
        for got, want in ((c.z, m.z[j0:]), (c.w, m.w[j0:])):
            assert got.shape == want.shape and (np.abs(got - want) <= 1e-12 * np.abs(want)).all()
        for got, want in ((c.ez, m.ez[j0:]), (c.ew, m.ew[j0:])):     # (the bounds: the cut row's peak in the states' term, not the history's)
            assert got.shape == want.shape and (got <= want * (1.0 + 1e-12)).all() and (got >= 0.5 * want).all()
        assert np.abs(c.l - m.l[j0:]).max() <= 1e-11 and np.abs(c.S - m.S[j0:]).max() <= 1e-11
        assert m.z[:40].min() > 1000.0 * m.z[j0:].max()              # (the history is loud)
        # the emulation's own rows, held from j0 on
        _, stats, mom, st = emulate(x, fs)
        worst = ref.check_curves_from(j0, c, mom, st)
        assert 0.0 < worst <= 1.0
    j0, c = ref.measure_from(x, fs, 5)                                # (a start nearer to the row's than the lead: the whole run)
    assert j0 == 1 and c.J == m.J - 1 and (c.z == m.z[1:]).all()


def test_the_gates_on_the_calls_own_curves():
    """the 300 s signal: L, Gamma, Gamma_r, LRA and the counts from the emulation's stored rows alone, against measure() within
    the two bounds together and against the emulation's stats within the rows' own rounding"""
    x, m, (audio, stats, mom, st) = _long_case("300s-mono")
    g = ref.gates_on_curves(mom, st)
    assert not g.undecided and not g.r_undecided and g.margin_bounds > 10.0
    assert (g.nA, g.nGt, g.Jr, g.nAr, g.nGr) == (m.nA, m.nGt, m.Jr, m.nAr, m.nGr) and 0 < g.nGr < g.nAr < g.Jr
    for got, dgot, want, dwant in ((g.L, g.dL, m.L, m.dL), (g.gamma, g.dgamma, m.gamma, m.dgamma), (g.gamma_r, g.dgamma_r, m.gamma_r, m.dgamma_r),
                                   (g.LRA, g.dLRA, m.LRA, m.dLRA)):
        assert abs(got - want) <= dgot + dwant and 0.0 < dgot < 1e-4, (got, dgot, want, dwant)
    worst = ref.check_stats_on_curves(g, stats)
    print("gates on the curves: worst error / bound %.3g; dL %.3g dGamma_r %.3g dLRA %.3g; margin %.3g bounds" % (worst, g.dL, g.dgamma_r, g.dLRA, g.margin_bounds))
    assert 0.0 <= worst <= 1.0
    # a value moved across a gate moves a count, and one put within its rounding of a gate makes the clip undecided
    moved = st.copy()
    moved[10 * int(np.argmax(st[::10] > g.gamma_r))] = np.float32(-71.0)
    h = ref.gates_on_curves(mom, moved)
    assert h.nAr == g.nAr - 1
    moved[0] = np.float32(-70.0)
    assert ref.gates_on_curves(mom, moved).r_undecided
    with pytest.raises(AssertionError):
        ref.check_stats_on_curves(h, stats)


# ---- 4. the loudness call, bit for bit ----
@pytest.mark.parametrize("kw", [dict(), dict(target=-14.0), dict(target=-14.0, peak_limit=0.3), dict(dual_mono=True)])
def test_without_the_true_peak_limit_the_first_eight_are_the_loudness_calls(kw):
    fs = 8000
    T = 33 * 800 + 3
    for Cn in (1, 2):
        if Cn == 2 and kw.get("dual_mono"):
            continue
        x = tlh._signal("step", Cn, T, fs, 40 + Cn)
        a0, s0, m0, _ = emulate(x, fs, loudness_call=True, **kw)
        a1, s1, m1, _ = emulate(x, fs, limit_true_peak=False, **kw)
        assert (s0.view(np.uint32) == s1[:8].view(np.uint32)).all() and (m0.view(np.uint32) == m1.view(np.uint32)).all()
        assert (a0.view(np.uint32) == a1.view(np.uint32)).all()
        assert (tlh.emulate(x, fs, **kw)[1].view(np.uint32) == s0.view(np.uint32)).all()


def test_the_gain_is_held_to_the_true_peak():
    fs, T = 8000, 10 * 800
    x = (0.05 * np.random.default_rng(9).standard_normal((1, T))).astype(np.float32)
    x[0, 4000] = x[0, 4001] = 0.5                       # TP about 0.57, P = 0.5
    m, stats, _ = _check(x, fs, target=-14.0, peak_limit=0.9, limit_true_peak=True)
    assert m.tp_limited and not m.undecided and stats[3] * stats[8] <= 0.9 * (1 + 2.0 ** -22) + stats[3] * m.dTP
    ms, ss, _ = _check(x, fs, target=-14.0, peak_limit=0.9, limit_true_peak=False)
    assert ms.limited and ss[3] == np.float32(0.9 / 0.5) and stats[3] < ss[3]
    m, stats, _ = _check(x, fs, target=-40.0, peak_limit=0.9)
    assert not m.tp_limited and not m.undecided


# ---- 5. refusals ----
def test_refusals_of_the_planning_calls():
    api = _api()
    assert api.r128_check(48000, 1) and api.r128_check(8000, 2, target=-70.0, limit_true_peak=False)
    assert api.r128_check(192000, 1, target=0.0, dual_mono=True, n_samples=19200 * 100)
    for kw in (dict(target=-70.1), dict(target=0.1), dict(target=float("inf")), dict(peak_limit=-0.1), dict(peak_limit=float("nan")),
               dict(dual_mono=2), dict(limit_true_peak=2), dict(limit_true_peak=-1)):
        assert not api.r128_check(48000, 1, **kw), kw
    assert not api.r128_check(7999, 1) and not api.r128_check(192001, 1) and not api.r128_check(48000, 3) and not api.r128_check(48000, 2, dual_mono=True)
    # Jr = 4096 is taken, Jr = 4097 is not: Js = 10 * 4096 + 1, I = Js + 29
    q = 800
    last = (10 * 4096 + 29) * q
    assert api.r128_plan(8000, last + q - 1)[8] == 4096 and api.r128_check(8000, 1, n_samples=last + q - 1)
    assert not api.r128_check(8000, 1, n_samples=last + q) and ref.plan(8000, last + q)["Jr"] == 4097
    with pytest.raises(ValueError):
        api.r128_plan(8000, last + q)
    for fs, T in ((7999, 100), (192001, 100), (48000, -1), (48000, 2 ** 31 - 3)):
        with pytest.raises(ValueError):
            api.r128_plan(fs, T)
    lib = api.load_library()
    js = C.c_longlong(-9)
    assert lib.pdmp3_amd_r128_plan(8000, last + q, None, None, None, None, None, None, None, C.byref(js), None, None) == -1 and js.value == -9
    assert lib.pdmp3_amd_r128_plan(8000, 30 * q, None, None, None, None, None, None, None, C.byref(js), None, None) == 0 and js.value == 1
    assert lib.pdmp3_amd_r128_check(None, 48000, 1) == -1 and lib.pdmp3_amd_r128_taps(None, None) == 0


# ---- 6. the sanitizer program ----
def test_the_sanitizer_program_of_the_planning_calls(tmp_path):
    """tools/sanitize/r128_plan.c: pdmp3_amd/host/clip_r128.c's check, taps and plan over the edge lengths under AddressSanitizer
    and UBSan, a stand-alone program on the CPU"""
    run_sanitizer_program(tmp_path, "r128_plan", ("clip_r128.c", "clip_loudness.c"))
