"""The loudness and R128 calls on long clips on the GPU, up to the limit of 4096 range windows (csrc/loudness.hip; DESIGN.md
sections 18 and 19): k_loud_chain at the edges of its steps of 64 chunks, every stride loop of k_loud_gate past its first
trip (more than 256 sub-blocks, waves, momentary blocks, short-term windows and range values), the ranking over thousands of
values, and one clip of Jr = 4096.

References as in tests/test_gpu_clip_loudness.py and tests/test_gpu_clip_r128.py, through the same helpers (tests/clip_gpu_calls.py): the audio
call's rows measured in binary64 with the derived bounds.  The clip at the limit is 68 minutes long and is not measured whole:
its first 300 s are held bit for bit to the same clip cut to 300 s (which is measured whole), its last 60 s to a reference
restarted 2 s in front of them (clip_r128_ref.measure_from), and its gated numbers to the gates evaluated on its own curves
(clip_r128_ref.gates_on_curves).  Every test asserts the shape it is there for."""
import contextlib
import functools

import numpy as np
import pytest

import clip_gpu as cg
import clip_gpu_calls as calls
import clip_loudness_ref as lref
import clip_r128_ref as ref
from clip_gpu import SENT
from clip_streams import ISO_LSF

pytestmark = pytest.mark.gpu
FS, Q = 8000, 800
GAINS = (152, 149, 146, 143, 140, 128, 90)          # global_gain of a segment: loud ones 4.5 dB apart, one 36 dB down, one under -70 LUFS
R128 = dict(target=-23.0, peak_limit=10 ** (-1 / 20))
LIMIT_T = (10 * 4096 + 29) * Q + Q - 1               # the largest n_samples the r128 call takes at 8 kHz: Jr = 4096
LIMIT_COUNTS = (32518, 8473, 3721, 2940)             # |A|, |Gt|, |Ar|, |Gr| of that clip: the binary64 reference on the CPU oracle's PCM


def _drawn_stream(frames, mode, seed):
    """segments of 62 .. 84 frames of MPEG-2.5 at 8 kHz end to end (like test_gpu_clip_r128._range_stream), at least `frames`
    frames in all, each segment's global_gain drawn from GAINS"""
    from pdmp3_amd import api
    from pdmp3_amd.packer import packer
    rng = np.random.default_rng(seed)
    parts, n = [], 0
    while n < frames:
        k, g = int(rng.integers(62, 85)), GAINS[int(rng.integers(len(GAINS)))]
        parts.append(packer.generate(n_frames=k, seed=1000 * seed + len(parts), version=2, sfreq=2, mode=mode, bitrate_index=6, iso_strict=True, gain=(g, g)))
        n += k
    mp3 = b"".join(parts)
    return mp3, api.StreamIndex(mp3, ISO_LSF)


@functools.lru_cache(maxsize=None)
def _long300_stream():
    """stereo, 4192 frames = 2 414 592 samples (301.8 s).  With the CPU oracle's PCM, the whole stream as one clip: J = 3015,
    Js = 2989, Jr = 299, |A| = 2433, |Gt| = 993, L = -8.59; |Ar| = 262 (37 windows of the range lie under -70), |Gr| = 228 (34
    more under Gamma_r = -32.82), LRA = 16.23; the window of the range nearest to a gate is 0.57 dB = 1680 bounds away from it.
    Downmixed to mono: |A| = 2385, |Ar| = 261, |Gr| = 228, L = -14.61, 1630 bounds.  No clip the tests below take from it is
    undecided"""
    return _drawn_stream(4180, 0, 300)


@functools.lru_cache(maxsize=None)
def _limit_stream():
    """mono, 57 003 frames = 32 833 728 samples (4104 s).  With the CPU oracle's PCM, its first LIMIT_T samples as one clip:
    J = 40 986, Js = 40 960, Jr = 4096, |A| = 32 518, |Gt| = 8473, L = -9.60; |Ar| = 3721, |Gr| = 2940, Gamma_r = -36.00,
    LRA = 21.18; the window of the range nearest to a gate is 0.027 dB = 94 bounds away from it.  Cut to 300 s and five
    samples: Jr = 298, |Ar| = 264, |Gr| = 207, LRA = 20.01, 567 bounds"""
    return _drawn_stream(56960, 3, 4096)


cg.STREAMS["long300"] = _long300_stream
cg.STREAMS["limit"] = _limit_stream


@contextlib.contextmanager
def _sample_loop_in_c():
    """clip_loudness_ref.measure's sample loop run by scipy's lfilter where scipy is there, as clip_r128_ref.measure runs it
    (tests/test_clip_loudness_host.py holds the two to 1e-12): the rows here are half a million samples long"""
    try:
        import scipy.signal  # noqa: F401
    except ImportError:
        yield
        return
    loop = lref.kweight
    lref.kweight = ref._kweight_blocks
    try:
        yield
    finally:
        lref.kweight = loop


def _same(a, b):
    return np.array_equal(cg.bits(a), cg.bits(b))


def _moved_without_the_state(x, fs, at, m):
    """how far the reference's momentary powers move, in their bounds, when the filters' state in front of sample `at` is
    forgotten (what a chain that lost its carry there would compute) -> (the largest move / bound, its window)"""
    q = m.q
    y = m.y.copy()
    y[:, at:] = ref._kweight_blocks(x[:, at:].astype(np.float64), fs)
    s = (y[:, :m.I * q] ** 2).reshape(x.shape[0], m.I, q).sum(axis=2)
    zc = np.array([s[:, j:j + 4].sum() for j in range(m.J)]) / (4.0 * q)
    r = np.abs(m.z - zc) / np.maximum(m.ez, 1e-300)
    return float(r.max()), int(np.argmax(r))


@pytest.mark.parametrize("fs,t", [(48000, 64 * 4096), (48000, 64 * 4096 + 1), (48000, 128 * 4096 + 1), (47670, 128 * 4096 + 1)])
def test_the_chain_at_the_edges_of_its_steps(fs, t):
    """the loudness call on the 48k stream as mono: 64 chunks, 64 chunks and a sample, 128 chunks and a sample -- one step of
    k_loud_chain exactly, a step of one chunk behind it (the guards), and the same behind two steps.  Two clips: from the
    stream's start, and from where the stream ends one sample in front of the clip's chunk 64, so that the zero tail behind it
    holds the decay of the state carried out of lane 63 and nothing else.  At 48 000 Hz no momentary block begins within the
    2000 samples behind chunk 64 in which that decay is above the bound (the stream has little below 40 Hz): those cases hold
    the chain's indexing and guards, and a wrong carry would move them by less than a bound.  At 47 670 Hz (q = 4767) block 55
    begins 41 samples behind chunk 64 and is that decay alone: forgetting the state there moves the reference by more than
    four bounds, asserted first.  (The carry's way into the step's other lanes, Phi^64 times it, is beyond any signal an MP3
    stream gives: tests/test_clip_loudness_host.py holds it at 192 000 Hz with an offset in the signal.)  Every number
    against binary64"""
    import clip_audio_ref
    dec = cg.decoder()
    try:
        ix = cg.source("48k")[1]
        n_all = clip_audio_ref.out_length(int(ix.samples), 48000, fs)
        assert ix.rate == 48000 and n_all > 64 * 4096
        end = 64 * 4096 - 1
        clips = [("48k", 0), ("48k", n_all - end)]
        q, n_chunks = lref.plan(fs, t)["q"], lref.plan(fs, t)["n_chunks"]
        assert n_chunks == {64 * 4096: 64, 64 * 4096 + 1: 65, 128 * 4096 + 1: 129}[t]
        x, valid = calls.audio_rows(dec, clips, t, fs, 1, 1)
        assert valid[1] == end and (x[1, :, end:] == 0).all() and valid[0] == min(t, n_all)
        got = calls.loudness_run(dec, "device", clips, t, fs, 1)
        with _sample_loop_in_c():
            refs, worst, margin, undecided = calls.loudness_check(x, valid, got, fs)
        m = refs[1]
        print("chain edges: fs %d t %d, %d chunks, J %d, valid %s, worst error / bound %.3g" % (fs, t, n_chunks, m.J, list(valid), worst))
        assert 0.0 < worst <= 1.0 and not undecided and all(0 < r.nGt <= r.nA for r in refs) and m.J == t // q - 3
        if fs == 47670:
            moved, k = _moved_without_the_state(x[1], fs, 64 * 4096, m)
            print("chain edges: without the state in front of chunk 64 block %d moves by %.3g bounds" % (k, moved))
            assert k == 55 and 0 < k * q - 64 * 4096 < 64 and moved > 4.0 and np.isfinite(m.l[k]) and m.ez[k] < 0.1 * m.z[k] and np.isfinite(got[2][1, k])
    finally:
        dec.close()


@functools.lru_cache(maxsize=None)
def _long300_length():
    return int(_long300_stream()[1].samples)


LENGTHS = {"27s": 27 * FS + 5, "30s": 30 * FS + 5, "whole": None}


@pytest.mark.parametrize("length", sorted(LENGTHS))
@pytest.mark.parametrize("channels", [2, 1])
def test_more_than_256_blocks_windows_and_range_values(channels, length):
    """both calls on long300, stereo and downmixed to mono.  27 s (J = 267, Js = 241) and 30 s (the bench's length: J = 297) from
    the stream's start and from a start that is no multiple of q; the whole stream's length (Jr = 299, 590 chunks, ten steps of
    the chain) as one batch of clips whose rows end at different places: from the start, from 40 s in, and two that begin 27 s
    and 1.5 s in front of the stream's end.  Every field and both curves against binary64, device and numpy destinations
    bit-equal; with limit_true_peak off fields 0-7, the momentary rows and the audio are the loudness call's"""
    all_t = _long300_length()
    t = LENGTHS[length] or all_t
    starts = [0, 40 * FS + 333] if t < all_t else [0, 40 * FS + 333, all_t - 27 * FS - 5, all_t - 3 * FS // 2]
    clips = [("long300", s) for s in starts]
    p = ref.plan(FS, t)
    dec = cg.decoder()
    try:
        x, valid = calls.audio_rows(dec, clips, t, 0, channels, channels)
        got = calls.r128_run(dec, "device", clips, t, 0, channels, **R128)
        refs, worst, margin, undecided = calls.r128_check(x, valid, got, FS, **R128)
        m = refs[0]
        print("long300 c=%d t=%d: J %d Js %d Jr %d chunks %d |A| %d |Gt| %d |Ar| %d |Gr| %d LRA %.2f worst error / bound %.3g margin %.3g bounds" %
              (channels, t, m.J, m.Js, m.Jr, p["n_chunks"], m.nA, m.nGt, m.nAr, m.nGr, m.LRA, worst, m.r_margin_bounds))
        assert 0.0 < worst <= 1.0 and m.J > 256 and p["I"] > 256 and not m.undecided and not m.r_undecided and m.r_margin_bounds > 10.0
        if length == "27s":
            assert (m.J, m.Js) == (267, 241)
        if length == "30s":
            assert (m.J, m.Js) == (297, 271) and p["n_chunks"] == 59
        if length == "whole":
            assert m.Js > 256 and m.Jr > 256 and p["n_chunks"] > 9 * 64 and 0 < m.nGr < m.nAr < m.Jr and 0 < m.nGt < m.nA < m.J
            assert list(valid) == [all_t, all_t - 40 * FS - 333, 27 * FS + 5, 3 * FS // 2]
        host = calls.r128_run(dec, "numpy", clips, t, 0, channels, **R128)
        for a, b in zip(got, host):
            assert _same(a, b)
        kw = dict(target=-14.0, peak_limit=0.5)
        audio, stats, mom, st, v = calls.r128_run(dec, "device", clips, t, 0, channels, limit_true_peak=False, **kw)
        want = calls.loudness_run(dec, "device", clips, t, 0, channels, **kw)
        assert _same(audio, want[0]) and _same(stats[:, :8], want[1]) and _same(mom, want[2]) and np.array_equal(v, want[3])
        assert _same(mom, got[2]) and _same(st, got[3]) and (stats[:, 3] != 1.0).any()
    finally:
        dec.close()


def test_a_shorter_clip_is_a_prefix_of_the_longer_one():
    """clips with one start: the momentary and the short-term rows of the 27 s clip are the first values of the 300 s clip's
    rows, bit for bit -- every sum has one fixed order and nothing behind a block enters it (the host build shows the same:
    tests/test_clip_r128_host.py)"""
    all_t = _long300_length()
    dec = cg.decoder()
    try:
        for start in (0, 40 * FS + 333):
            short = calls.r128_run(dec, "device", [("long300", start)], 27 * FS + 5, c=2, **R128)
            whole = calls.r128_run(dec, "device", [("long300", start)], all_t, c=2, **R128)
            J, Js = short[2].shape[1], short[3].shape[1]
            assert (J, Js) == (267, 241) and whole[2].shape[1] > 2900 and whole[3].shape[1] > 2900
            assert _same(short[2], whole[2][:, :J]) and _same(short[3], whole[3][:, :Js])
            assert np.isfinite(short[2]).any() and short[1][0, 13] == 25 and whole[1][0, 13] > 256
    finally:
        dec.close()


def test_windows_behind_the_streams_end_do_not_count():
    """a clip of long300 whose last 40 s lie behind the stream's end: those windows of the range are silence, gated out and
    skipped by the ranking, whose loop still walks them.  |Ar| is the reference's, every field within its bound"""
    all_t = _long300_length()
    start = 40 * FS + 123
    dec = cg.decoder()
    try:
        clips = [("long300", start)]
        x, valid = calls.audio_rows(dec, clips, all_t, 0, 0, 2)
        assert valid[0] == all_t - start and (x[0, :, valid[0]:] == 0).all()
        got = calls.r128_run(dec, "device", clips, all_t, c=2, **R128)
        refs, worst, margin, undecided = calls.r128_check(x, valid, got, FS, **R128)
        m = refs[0]
        silent = int((got[3][0, ::10] < -150.0).sum())
        print("ties: Jr %d |Ar| %d |Gr| %d, %d windows of the range in silence, worst error / bound %.3g" % (m.Jr, m.nAr, m.nGr, silent, worst))
        assert m.Jr > 256 and silent >= 35 and (got[3][0, -350:] < -150.0).all() and not undecided and not m.r_undecided
        assert got[1][0, 14] == m.nAr <= m.Jr - silent and 0 < got[1][0, 15] == m.nGr < m.nAr and 0.0 < worst <= 1.0
    finally:
        dec.close()


class _Limit:
    pass


_LIMIT = {}


def _limit_case():
    """the run at the limit, made once -- a run that failed is not made again: the tests that need it fail with it"""
    if "error" in _LIMIT:
        pytest.fail("the run at the limit failed in an earlier test: %r" % (_LIMIT["error"],))
    if "case" not in _LIMIT:
        try:
            _LIMIT["case"] = _run_the_limit()
        except BaseException as e:
            _LIMIT["error"] = e
            raise
    return _LIMIT["case"]


def _run_the_limit():
    """one clip of the limit stream from sample 0 with the largest n_samples the call takes (Jr = 4096: 32 791 999 samples, 8006
    chunks, 126 steps of the chain, sixteen trips of every thread through the ranking), run once: the audio call's row and the
    r128 call with both curves.  Of the two rows of 131 MB only what the tests below look at is kept"""
    t = LIMIT_T
    clips = [("limit", 0)]
    dec = cg.decoder()
    try:
        ix = _limit_stream()[1]
        assert ix.rate == FS and ix.channels == 1 and int(ix.samples) >= t
        x, valid = calls.audio_rows(dec, clips, t, 0, 0, 1)
        audio, stats, mom, st, v = calls.r128_run(dec, "device", clips, t, c=1, **R128)
    finally:
        dec.close()
    c = _Limit()
    c.valid, c.v, c.stats, c.mom, c.st = valid, v, stats[0], mom[0], st[0]
    c.peak = np.abs(x[0]).max()
    c.at = (0, t // 2 - 50001, t - 100003)
    c.x = [x[0, :, lo:lo + 100003].copy() for lo in c.at]
    c.audio = [audio[0, :, lo:lo + 100003].copy() for lo in c.at]
    c.head = x[:, :, :300 * FS + 5].copy()
    c.tail_from = ((t - 60 * FS) // Q - 25) * Q          # (a multiple of q, and more than measure_from's lead in front of the last 60 s)
    c.tail = x[0, :, c.tail_from:].copy()
    return c


def test_the_limit_of_4096_range_windows():
    """what is exact at Jr = 4096: J, Js, Jr, the sample peak (the audio call's row), TP >= P, M and Smax (the largest values of
    the curves), audio = row times g on three slices of 100 003 samples -- head, middle and tail"""
    p = ref.plan(FS, LIMIT_T)
    assert p["Jr"] == 4096 and p["Js"] == 40960 and p["J"] == 40986 and p["n_chunks"] == 8006 and ref.plan(FS, LIMIT_T + 1)["Jr"] == 4097
    c = _limit_case()
    assert c.valid[0] == c.v[0] == LIMIT_T and (c.stats[5], c.stats[12], c.stats[13]) == (p["J"], p["Js"], 4096)
    assert c.mom.shape == (p["J"],) and c.st.shape == (p["Js"],)
    assert np.float32(c.stats[2]) == c.peak and c.stats[8] >= c.stats[2] > 0
    assert c.stats[1] == np.float32(c.mom.max()) and c.stats[9] == np.float32(c.st.max())
    g = np.float32(c.stats[3])
    assert g != 1.0 and np.isfinite(c.stats).all()
    for lo, x, audio in zip(c.at, c.x, c.audio):
        assert np.abs(x).max() > 0 and _same(audio, (x * g).astype(np.float32)), "audio is not x * g from %d on" % lo


def test_the_limits_first_300_s_are_the_clip_cut_there():
    """the curves' first 300 s are the rows of the same clip cut to 300 s and five samples, bit for bit (the prefix property
    once more, over 126 steps of the chain against 10); the cut clip is held to binary64 whole"""
    c = _limit_case()
    cut = c.head.shape[2]
    dec = cg.decoder()
    try:
        got = calls.r128_run(dec, "device", [("limit", 0)], cut, c=1, **R128)
    finally:
        dec.close()
    refs, worst, margin, undecided = calls.r128_check(c.head, np.array([cut]), got, FS, **R128)
    m = refs[0]
    print("limit, cut to 300 s: Jr %d |Ar| %d |Gr| %d LRA %.2f worst error / bound %.3g margin %.3g bounds" % (m.Jr, m.nAr, m.nGr, m.LRA, worst, m.r_margin_bounds))
    assert 0.0 < worst <= 1.0 and not undecided and m.Jr > 256 and 0 < m.nGr < m.nAr < m.Jr and m.r_margin_bounds > 10.0
    assert _same(got[2][0], c.mom[:m.J]) and _same(got[3][0], c.st[:m.Js])


def test_the_limits_last_60_s_from_a_restart():
    """the last 60 s of both curves within their bounds of a reference restarted 2 s in front of them"""
    c = _limit_case()
    p = ref.plan(FS, LIMIT_T)
    t0 = LIMIT_T - 60 * FS
    k0, tail = ref.measure_from(c.tail, FS, t0 - c.tail_from)
    j0 = k0 + c.tail_from // Q
    assert c.tail_from % Q == 0 and j0 == (t0 + Q - 1) // Q and j0 + tail.J == p["J"] and j0 + tail.Js == p["Js"]
    assert tail.J > 590 and tail.Js > 560 and np.isfinite(tail.l).sum() > 100
    worst = ref.check_curves_from(j0, tail, c.mom, c.st)
    print("limit, last 60 s: windows from %d on, worst error / bound %.3g" % (j0, worst))
    assert 0.0 < worst <= 1.0


def test_the_limits_gated_numbers_are_the_gates_on_its_own_curves():
    """L, Gamma, Gamma_r, LRA and the four counts from the 40 986 momentary and 40 960 short-term values the call stored, within
    the bound those values' own rounding gives -- and the counts are those of the binary64 reference on the CPU oracle's PCM"""
    c = _limit_case()
    g = ref.gates_on_curves(c.mom, c.st)
    assert g.Jr == 4096 and 0 < g.nGr < g.nAr < g.Jr and 0 < g.nGt < g.nA < len(c.mom) and g.margin_bounds > 10.0
    worst = ref.check_stats_on_curves(g, c.stats)
    print("limit: |A| %d |Gt| %d |Ar| %d |Gr| %d L %.3f Gamma_r %.3f LRA %.3f; gates on the curves: worst error / bound %.3g, margin %.3g bounds" %
          (g.nA, g.nGt, g.nAr, g.nGr, g.L, g.gamma_r, g.LRA, worst, g.margin_bounds))
    assert 0.0 <= worst <= 1.0 and g.LRA > 3.0 and (g.nA, g.nGt, g.nAr, g.nGr) == LIMIT_COUNTS


def test_one_sample_more_than_the_limit_is_refused():
    t = LIMIT_T + 1
    p = ref.plan(FS, LIMIT_T)
    dec = cg.decoder()
    try:
        import torch
        big, view = cg.destination("device", 1, 1, (t,))
        mom, st = cg.filled("device", (1, p["J"])), cg.filled("device", (1, p["Js"]))
        src = cg.src([("limit", 0)])
        with pytest.raises(RuntimeError):
            dec.decode_clips_r128(src, t, 0, 1, out=view, momentary=mom, short_term=st, **R128)
        with pytest.raises(RuntimeError):
            dec.decode_clips_r128(src, t, 0, 1, out=view, **R128)
        torch.cuda.synchronize()
        assert bool((big == float(SENT)).all()) and bool((mom == float(SENT)).all()) and bool((st == float(SENT)).all())
    finally:
        dec.close()
