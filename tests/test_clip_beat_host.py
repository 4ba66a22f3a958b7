"""Beat tracking of clips on the host, no GPU: the numpy restatement (tests/clip_beat_ref.py) against a
plain transliteration of librosa's loops; the product's tables against numpy's within section 26's bound; the kernels' own phases
(pdmp3_amd/csrc/beat_core.h, compiled here with g++ into tests/host_emul/beat_emul.cpp and run thread by thread, the programme's
step on wave_emul.h's fibers, over a poisoned LDS) bit for bit against the restatement on the product's own tables -- periods
that round h down, exactly and up, 2 P > n, n = 2 and 3, n no multiple of h or of 64, the empty cases, a tie planted in cum; the
check, the plan and the refusals; the sanitizer program."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.signal

import clip_beat_cases as bc
import clip_beat_ref as ref
from clip_host import build_emul, run_sanitizer_program

PERIODS = (1, 2, 7, 21, 22, 23, 45, 200)
TIGHTNESS = 100.0


def _api():
    from pdmp3_amd import api
    return api


def _emul():
    lib = build_emul("beat")
    vp = C.c_void_p
    lib.emul_beat_score.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_uint, vp, vp]
    lib.emul_beat_dp.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_uint, vp, vp]
    lib.emul_beat_pick.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
    lib.emul_beat_table_at.restype = C.c_longlong
    lib.emul_beat_work_doubles.restype = lib.emul_beat_score_lds.restype = lib.emul_beat_dp_lds.restype = C.c_uint
    return lib


def envelope(period, n, seed, noise=0.3):
    """a noisy impulse train: what an onset envelope of a steady beat looks like (binary32, non-negative)"""
    rng = np.random.default_rng(seed)
    o = noise * rng.random(n)
    o[(seed % max(period, 1))::period] += 1.0 + 0.2 * rng.random(len(o[(seed % max(period, 1))::period]))
    return o.astype(np.float32)


def bpm_of(period, sample_rate=22050, hop=512):
    return 60.0 * sample_rate / (hop * period)


@functools.lru_cache(maxsize=None)
def product_tables(period, tightness=TIGHTNESS):
    return _api().beat_tables(period, tightness=tightness)


# ---- librosa 0.10's tracker, loop for loop (librosa/beat.py: __beat_tracker and what it calls) ----
def librosa_tracker(onset, period, tightness, trim):
    onset = np.asarray(onset, dtype=np.float64)
    norm = onset.std(ddof=1)                                             # __normalize_onsets
    window = np.exp(-0.5 * (np.arange(-period, period + 1) * 32.0 / period) ** 2)
    localscore = scipy.signal.convolve(onset / norm, window, "same")    # __beat_local_score
    n = len(localscore)
    backlink, cumscore = np.zeros(n, dtype=int), np.zeros(n)            # __beat_track_dp
    score_thresh = 0.01 * localscore.max()
    first_beat = True
    for i, score_i in enumerate(localscore):
        best_score, beat_location = -np.inf, -1
        for loc in range(i - int(np.round(period / 2)), i - 2 * period - 1, -1):
            if loc < 0:
                break
            with np.errstate(divide="ignore"):
                score = cumscore[loc] - tightness * (np.log(i - loc) - np.log(period)) ** 2
            if score > best_score:
                best_score, beat_location = score, loc
        cumscore[i] = score_i + best_score if beat_location >= 0 else score_i
        if first_beat and score_i < score_thresh:
            backlink[i] = -1
        else:
            backlink[i] = beat_location
            first_beat = False
    mask = np.zeros(n, dtype=bool)                                       # util.localmax
    mask[1:-1] = (cumscore[1:-1] > cumscore[:-2]) & (cumscore[1:-1] >= cumscore[2:])
    mask[-1] = cumscore[-1] > cumscore[-2]
    threshold = 0.5 * np.median(cumscore[mask])                          # __last_beat
    tail = int(np.nonzero(mask & (cumscore >= threshold))[0].max())
    beats = [tail]
    while backlink[beats[-1]] >= 0:
        beats.append(backlink[beats[-1]])
    beats = np.array(beats[::-1], dtype=int)
    smooth_boe = scipy.signal.convolve(localscore[beats], np.array([0.0, 0.5, 1.0, 0.5, 0.0]), "same")   # __trim_beats, hann(5)
    threshold = 0.5 * ((smooth_boe ** 2).mean() ** 0.5) if trim else 0.0
    keep = np.nonzero(smooth_boe > threshold)[0]
    return localscore, beats[keep.min():keep.max() + 1]


@pytest.mark.parametrize("period", PERIODS)
def test_the_restatement_is_librosas_algorithm(period):
    """The restatement with numpy's own tables against the transliteration: the same beats, with and without the trim, and a local
    score within 1e-12 of its largest magnitude (two summation orders of at most 2 P + 1 <= 401 products of similar size in
    binary64, or scipy's FFT path: either is far below)."""
    n = 261
    o = envelope(period, n, seed=period)
    g, tx = ref.tables(period, TIGHTNESS)
    for trim in (True, False):
        ls64, ls = ref.local_score(o, period, g)
        cum, back = ref.programme(ls, period, tx)
        got = ref.pick(ls, cum, back, trim)["beats"]
        want_ls, want = librosa_tracker(o, period, TIGHTNESS, trim)
        assert np.abs(ls64 - want_ls).max() <= 1e-12 * np.abs(want_ls).max()
        assert np.array_equal(got, want), (period, trim, got, want)
    if period in (2, 7, 22, 45) and n > 4 * period:
        assert np.median(np.diff(got)) == period, (period, np.diff(got))        # (the clip's end may cut the last interval short)


def test_h_rounds_down_exactly_and_up():
    assert [ref.half(p) for p in (1, 2, 3, 5, 21, 22, 23, 45, 200, 1023)] == [1, 1, 2, 2, 10, 11, 12, 22, 100, 512]
    assert all(_emul().emul_beat_half(p) == ref.half(p) for p in range(1, 1024))


@pytest.mark.parametrize("period", PERIODS + (1023,))
def test_the_products_tables_against_numpy(period):
    """g: the argument -0.5 (32 k / P)^2 is the same binary64 value on both sides (three operations, each rounded once), and two
    correctly working libraries' exponentials lie within an ulp of the true value each: 2 ulp apart, 4 allowed.  tx: a logarithm
    within an ulp of ln v, so x = ln d - ln P is off by at most E = 2^-52 (ln d + ln P) + 2^-53 |x| on either side, and
    t x^2 by t (2 |x| E + E^2) plus two roundings: twice that between the two."""
    g, tx = product_tables(period)
    ng, ntx = ref.tables(period, TIGHTNESS)
    assert g.shape == ng.shape and tx.shape == ntx.shape
    assert np.all(np.abs(g - ng) <= 4 * 2.0 ** -52 * ng)
    d = np.arange(2 * period + 1, dtype=np.float64)
    h = ref.half(period)
    assert np.all(tx[:h] == 0.0)
    x = np.abs(np.log(d[h:] / period))
    e = 2.0 ** -52 * (np.log(d[h:]) + np.log(period)) + 2.0 ** -53 * x
    bound = 2 * (TIGHTNESS * (2 * x * e + e * e) + 2 * 2.0 ** -53 * np.abs(ntx[h:]))
    assert np.all(np.abs(tx[h:] - ntx[h:]) <= bound)
    assert tx[period] == 0.0 and g[0] == 1.0


# ---- the emulated kernels ----
def emul_score(o, n_frames, period, p_max=None):
    lib, p_max = _emul(), p_max or period
    g = product_tables(period)[0]
    o = np.ascontiguousarray(o, dtype=np.float32)
    ls = np.full(n_frames, np.nan, dtype=np.float32)
    norm = C.c_double(0.0)
    rc = lib.emul_beat_score(o.ctypes.data, o.size, n_frames, period, p_max, g.ctypes.data, lib.emul_beat_score_lds(p_max, n_frames), ls.ctypes.data,
                             C.byref(norm))
    assert rc >= 0, "the emulated kernel read LDS it must not read"
    return rc, ls, norm.value


def emul_dp(ls, n, n_frames, period, tx, p_max=None):
    lib, p_max = _emul(), p_max or period
    ls = np.ascontiguousarray(ls, dtype=np.float32)
    tx = np.ascontiguousarray(tx, dtype=np.float64)
    cum, back = np.full(n_frames, np.nan), np.full(n_frames, -7, dtype=np.int32)
    assert lib.emul_beat_dp(ls.ctypes.data, n, n_frames, period, p_max, tx.ctypes.data, lib.emul_beat_dp_lds(p_max), cum.ctypes.data, back.ctypes.data) == 0
    return cum[:n], back[:n]


def emul_pick(ls, cum, back, n_frames, trim):
    n = cum.size
    ls, cum, back = np.ascontiguousarray(ls, dtype=np.float32), np.ascontiguousarray(cum), np.ascontiguousarray(back, dtype=np.int32)
    lmv, bt = np.full(n_frames, np.nan), np.full(n_frames, -7, dtype=np.int32)
    rows, res = np.full((2, n_frames), np.nan, dtype=np.float32), np.zeros(5)
    assert _emul().emul_beat_pick(ls.ctypes.data, cum.ctypes.data, back.ctypes.data, n, n_frames, 1 if trim else 0, lmv.ctypes.data, bt.ctypes.data,
                                  rows.ctypes.data, res.ctypes.data) == 0
    return rows, res


def emul_track(o, n_frames, period, trim=True, p_max=None):
    """the three emulated kernels in the call's order -> the same dict as ref.track"""
    n = len(o)
    g, tx = product_tables(period)
    run, ls, norm = emul_score(o, n_frames, period, p_max)
    dp = np.stack([np.zeros(n_frames, dtype=np.float32), np.full(n_frames, -1.0, dtype=np.float32)])
    rows = dp.copy()
    stats = [0.0, -1.0, -1.0, np.float32(norm) if run else -1.0, -1.0, float(n)]
    if run:
        cum, back = emul_dp(ls, n, n_frames, period, tx, p_max)
        with np.errstate(over="ignore"):
            dp[0, :n], dp[1, :n] = cum.astype(np.float32), back.astype(np.float32)
        rows, res = emul_pick(ls, cum, back, n_frames, trim)
        if res[4]:
            stats[0], stats[1], stats[2], stats[4] = res[0], res[1], res[2], np.float32(res[3])
    return dict(score=ls, dp=dp, beats=rows, stats=np.array(stats, dtype=np.float32))


def same(got, want, what):
    for key in ("score", "dp", "beats", "stats"):
        assert np.array_equal(got[key].view(np.uint32), want[key].view(np.uint32)), (what, key, got[key], want[key])


CASES = [(p, n, f) for p in PERIODS for n, f in ((261, 261), (250, 261))] + [(22, 675, 675), (7, 2, 11), (7, 3, 11), (2, 11, 11), (1, 65, 70),
                                                                            (45, 129, 129), (200, 300, 300), (1023, 2100, 2100), (383, 700, 700)]
# the lane counts 32 and 4 of a frame of the programme's step, h = 256 (the last one-pass step) and h = 258 (the first of two
# passes), each with more than 2 P + 3 h frames: whole windows over more than two steps
CASES += [(12, 261, 261), (12, 250, 261), (100, 512, 520), (513, 1800, 1800), (515, 1810, 1811)]


@pytest.mark.parametrize("period,n,n_frames", CASES)
def test_the_emulated_kernels_are_the_restatement_bit_for_bit(period, n, n_frames):
    """ls, fl32(cum), back, the mask, the list, kept / beats / tail, and norm and thr as binary32, on the product's tables"""
    o = envelope(period, n, seed=period + n)
    g, tx = product_tables(period)
    for trim in (True, False):
        want = ref.track(o, n_frames, period, g, tx, trim)
        same(emul_track(o, n_frames, period, trim), want, (period, n, trim))
    if n > 4 * period:
        assert want["stats"][0] > 0, "a steady beat must give beats"
    # the same with the LDS planned for a larger period, as when the tempo is estimated
    same(emul_track(o, n_frames, period, True, p_max=max(period, 383)), ref.track(o, n_frames, period, g, tx, True), (period, n, "p_max"))


def test_random_envelopes():
    rng = np.random.default_rng(5)
    for period, n in ((3, 200), (22, 517), (31, 400), (100, 450)):
        o = rng.random(n).astype(np.float32) ** 4
        g, tx = product_tables(period)
        same(emul_track(o, n + 5, period), ref.track(o, n + 5, period, g, tx), (period, n))


@pytest.mark.parametrize("o", [np.zeros(0), np.ones(1), np.zeros(40), np.full(40, 0.25), np.array([1.0, 1.0])], ids=["n0", "n1", "silent", "constant", "two_equal"])
def test_the_empty_cases(o):
    """n < 2 and a norm that is not positive: no beats, ls and cum 0, back -1, kept 0 and -1 for what is not reached"""
    o = o.astype(np.float32)
    g, tx = product_tables(7)
    got = emul_track(o, 48, 7) if len(o) else ref.track(o, 48, 7, g, tx)      # (n = 0 launches nothing worth emulating: the definition alone)
    same(got, ref.track(o, 48, 7, g, tx), "empty")
    assert not got["score"].any() and not got["dp"][0].any() and np.all(got["dp"][1] == -1) and not got["beats"][0].any() and np.all(got["beats"][1] == -1)
    assert list(got["stats"][:5]) == [0, -1, -1, -1, -1] and got["stats"][5] == len(o)


def test_no_local_maximum_and_no_tail():
    """a falling cum has no local maximum; negative maxima lie below half their median"""
    n, F = 30, 32
    ls = -np.arange(n, dtype=np.float32)
    tx = np.zeros(15)
    tx[:4] = 0.0
    cum, back = ref.programme(ls, 7, tx)
    ecum, eback = emul_dp(ls, n, F, 7, tx)
    assert np.array_equal(cum, ecum) and np.array_equal(back, eback)
    assert not ref.local_maxima(cum).any()
    rows, res = emul_pick(ls, ecum, eback, F, True)
    assert list(res) == [0, -1, -1, -1, 0] and not rows[0].any() and np.all(rows[1] == -1)
    cum = -10.0 - (np.arange(n) % 3 != 1)
    back = np.full(n, -1)
    want = ref.pick(ls, cum, back, True)
    assert want["maxima"] > 0 and want["tail"] == -1 and want["q"] == 0
    rows, res = emul_pick(ls, cum, back, F, True)
    assert list(res) == [0, 0, -1, -1, want["maxima"]] and not rows[0].any()


TIE_PERIODS = (2, 7, 12, 22, 45, 100, 200, 300, 515)


def test_the_tie_periods_reach_every_form_of_the_step():
    """64, 32, 16, 8, 4, 2 lanes a frame and one, and the step of two passes (h > 256)"""
    plans = [_api().beat_plan(22050, n_frames=3 * p + 41, bpm=bpm_of(p)) for p in TIE_PERIODS]
    assert [q["period"] for q in plans] == list(TIE_PERIODS)
    assert [q["lanes"] for q in plans] == [64, 64, 32, 16, 8, 4, 2, 1, 1] and [q["h"] > 256 for q in plans] == [False] * 8 + [True]


@pytest.mark.parametrize("period", TIE_PERIODS)
def test_a_tie_planted_in_cum(period):
    """a flat transition cost and small integer scores make many candidates of a frame equal: the smallest d wins in the programme,
    whichever lane held it, and equal local maxima rank as the median's rule says"""
    n = 3 * period + 41
    rng = np.random.default_rng(period)
    ls = rng.integers(0, 2, n).astype(np.float32)
    ls[0] = 1.0
    tx = np.zeros(2 * period + 1)
    cum, back = ref.programme(ls, period, tx)
    h = ref.half(period)
    ties = sum(1 for i in range(2 * period, n) if np.sum(cum[i - 2 * period:i - h + 1] == cum[i - 2 * period:i - h + 1].max()) > 1)
    assert ties > n // 4, "the case must hold ties"
    ecum, eback = emul_dp(ls, n, n, period, tx)
    assert np.array_equal(cum, ecum) and np.array_equal(back, eback)
    for trim in (True, False):
        want = ref.pick(ls, cum, back, trim)
        rows, res = emul_pick(ls, ecum, eback, n, trim)
        b = want["beats"]
        assert np.array_equal(np.nonzero(rows[0])[0], b) and np.array_equal(rows[1, :b.size], b) and np.all(rows[1, b.size:] == -1)
        assert list(res[:3]) == [b.size, want["q"], want["tail"]] and np.float32(res[3]) == np.float32(want["thr"])


@pytest.mark.parametrize("period", TIE_PERIODS)
def test_a_tie_from_a_planted_envelope(period):
    """the same from an envelope, as the device test hands it to the three kernels (tests/clip_beat_cases.py tie_envelope): the
    product's g, a flat transition cost, and stretches where the local score is exactly 0"""
    n = 3 * period + 41
    o = bc.tie_envelope(period, n)
    g, tx = product_tables(period)[0], np.zeros(2 * period + 1)
    run, ls, norm = emul_score(o, n, period)
    want = ref.track(o, n, period, g, tx, True)
    assert run and np.array_equal(ls.view(np.uint32), want["score"].view(np.uint32)) and (ls == 0).sum() > period // 4
    cum, back = ref.programme(ls, period, tx)
    assert bc.tied_frames(cum, period) > n // 8, "the case must hold ties"
    ecum, eback = emul_dp(ls, n, n, period, tx)
    assert np.array_equal(cum, ecum) and np.array_equal(back, eback)
    rows, res = emul_pick(ls, ecum, eback, n, True)
    assert np.array_equal(rows.view(np.uint32), want["beats"].view(np.uint32)) and list(res[:3]) == [want["stats"][0], want["stats"][1], want["stats"][2]]


# ---- the check, the plan, the refusals ----
def test_check_and_plan():
    api = _api()
    assert api.beat_check(22050, n_frames=1292)
    p = api.beat_plan(22050, n_frames=1292, bpm=120.0)
    assert (p["period"], p["h"], p["p_min"], p["p_max"], p["threads"], p["steps"], p["lanes"], p["frames"]) == (22, 11, 22, 22, 256, 118, 16, 16)
    assert p["score_lds"] == _emul().emul_beat_score_lds(22, 1292) and p["dp_lds"] == _emul().emul_beat_dp_lds(22)
    assert p["work_bytes"] == 8 * _emul().emul_beat_work_doubles(1292) and p["table_bytes"] == 8 * (3 * 22 + 2)
    p = api.beat_plan(22050, n_frames=1292)
    first = api.tempogram_prior(22050, out_mode="tempo")[1]
    assert (p["period"], p["p_min"], p["p_max"], p["h"]) == (0, first, 383, 192)
    assert p["table_bytes"] == 8 * sum(3 * q + 2 for q in range(first, 384)) == 8 * _emul().emul_beat_table_at(first, 384)
    assert p["score_lds"] == _emul().emul_beat_score_lds(383, 1292) and p["dp_lds"] == _emul().emul_beat_dp_lds(383)
    for period in PERIODS + (1023,):
        assert api.beat_plan(22050, n_frames=10, bpm=bpm_of(period))["period"] == period
    assert api.beat_plan(16000, n_frames=10, bpm=100.0, hop=256)["period"] == ref.period_of(100.0, 16000, 256)
    # P = round-half-even(60 sr / (hop bpm)): 60 * 16000 / (256 * 100) = 37.5 -> 38
    assert api.beat_plan(16000, n_frames=10, bpm=150.0, hop=256)["period"] == 25 and api.beat_plan(16000, n_frames=10, bpm=100.0, hop=256)["period"] == 38


@pytest.mark.parametrize("kw", [dict(bpm=-1.0), dict(bpm=float("nan")), dict(bpm=float("inf")), dict(bpm=1e-3), dict(bpm=1e6), dict(tightness=0.0),
                                dict(tightness=-1.0), dict(tightness=float("nan")), dict(tightness=float("inf")), dict(out_mode=3), dict(out_mode=-1),
                                dict(n_frames=32769), dict(n_frames=-1), dict(win_length=383), dict(lag=0), dict(max_size=2), dict(n_fft=1024),
                                dict(max_tempo=1.0), dict(start_bpm=0.0)])
def test_refusals(kw):
    api = _api()
    a = dict(n_frames=100)
    a.update(kw)
    assert not api.beat_check(22050, **a)
    with pytest.raises(ValueError):
        api.beat_plan(22050, **a)
    assert api.beat_check(22050, n_frames=32768) and api.beat_check(22050, n_frames=0, bpm=120.0)


def test_tables_refuse_a_bad_period():
    api = _api()
    for period in (0, -1, 1024):
        with pytest.raises(ValueError):
            api.beat_tables(period)


# ---- the sanitizer program ----
def test_the_sanitizer_program_of_the_planning_calls(tmp_path):
    """tools/sanitize/beat_plan.c: pdmp3_amd/host/clip_beat.c's check, tables and plan over the refusals and the edge cases under
    AddressSanitizer and UBSan, a stand-alone program on the CPU"""
    run_sanitizer_program(tmp_path, "beat_plan", ("clip_beat.c", "clip_tempogram.c", "clip_mel_long.c", "clip_mel.c", "clip_stft_long.c", "clip_stft.c"))
