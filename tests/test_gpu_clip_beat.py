"""Beat tracking of clips on the device: decode_clips_beats's three modes, each bit for bit against the
numpy restatement (tests/clip_beat_ref.py, on the product's own tables) evaluated on what the product itself returns one stage
earlier -- the local score on decode_clips_tempogram's onset envelope of the same clips, the programme on mode "score"'s output,
the beats on that programme (the restatement's binary64 cum, whose binary32 rounding and back-links are mode "dp"'s) -- and mode
"beats" alone against the chain; the estimated tempo against decode_clips_tempogram's; clips that run over their stream's end; a
periodic stream whose answer the reference (the CPU oracle's decode through the binary64 definition) gives first; determinism,
batches, destinations, empty calls and refusals."""
import functools

import numpy as np
import pytest

import clip_beat_ref as ref
import clip_gpu as cg
import clip_gpu_calls as cc
import clip_mel_long_ref as mlref
import clip_mel_ref as mref
import clip_streams
import clip_tempogram_ref as tref
from clip_gpu import GUARD, SENT
from clip_streams import ISO_LSF

pytestmark = pytest.mark.gpu
P0 = cc.BEAT_P0


@functools.lru_cache(maxsize=None)
def _periodic():
    """test_gpu_clip_tempogram.py's recipe, rebuilt: one chunk of twenty MPEG-1 frames at 44.1 kHz, mono, no bit reservoir,
    fifteen times; once the first chunk's overlap has settled the decoded row repeats every 23 040 samples = 45 hops of 512"""
    from pdmp3_amd import api
    from pdmp3_amd.packer import packer
    chunk = packer.generate(n_frames=20, seed=7, sfreq=0, mode=3, bitrate_index=7, reservoir=False)
    mp3 = b"".join([chunk] * 15)
    return mp3, api.StreamIndex(mp3, ISO_LSF)


cg.STREAMS["beat/periodic-44k"] = _periodic


tables, bpm_of = cc.beat_tables, cc.beat_bpm_of
_run, _onset, _same, _check_chain = cc.beat_run, cc.beat_onset, cc.beat_same, cc.beat_check_chain


CASES = {"mono-resampled": ("44k-mono", dict(P0)), "stereo-own-rate": ("48k", dict(P0, sample_rate=0, channels=2))}


@pytest.mark.parametrize("period", [2, 21, 22, 23, 200])
@pytest.mark.parametrize("case", sorted(CASES))
def test_every_stage_against_the_restatement_on_the_stage_before(case, period):
    """F = 261: more than one tile of the score and one block of the sums, no multiple of either; the third clip runs over its
    stream's end.  Period 200 is more than F / 2: the window reaches in front of frame 0 at every frame."""
    name, p = CASES[case]
    f, hop = 261, p["hop"]
    clips = [(name, s) for s in (p["lag"] * hop, 12345, cg.j_all(p, name) - 200 * hop - 3)]
    dec = cg.decoder()
    try:
        res, valid = _check_chain(dec, clips, f, p, period)
        assert valid[0] == f and 0 < valid[2] < f
        beats, stats = res[True]
        print("%s, P %d: kept %s of %s beats, tails %s" % (case, period, stats[:, :, 2].ravel(), stats[:, :, 3].ravel(), stats[:, :, 4].ravel()))
        assert (stats[:, :, 3] >= 1).all(), "noise has local maxima: a tail and a walk"
    finally:
        dec.close()


def test_short_clips_at_a_streams_start_and_end_and_a_long_one():
    """F = 11 at sample 0 and over the stream's end (fewer frames than 2 P, than h, than a block), F = 675 (three tiles, eleven
    blocks) -- on host destinations too"""
    name, p = "44k-mono", dict(P0)
    j_all = cg.j_all(p, name)
    dec = cg.decoder()
    try:
        for period in (2, 22):
            res, valid = _check_chain(dec, [(name, 0), (name, j_all - 4 * p["hop"] - 7)], 11, p, period, kind="numpy")
            assert valid[0] == 11 and valid[1] == 5
        res, valid = _check_chain(dec, [(name, 3000)], 675, p, 22)
        assert 100 < valid[0] < 675 and res[True][1][0, 0, 2] >= 2
    finally:
        dec.close()


def test_the_estimated_tempo_is_the_tempo_calls_and_its_lag_the_period():
    dec = cg.decoder()
    try:
        for name, p, f in (("44k-mono", dict(P0), 261), ("48k", dict(P0, sample_rate=0, channels=2, win_length=64), 57)):
            hop, sr = p["hop"], cg.rate(p, name)
            clips = [(name, s) for s in ((p["win_length"] // 2 + 16) * hop, (p["win_length"] // 2) * hop + 60001)]
            q = {a: p[a] for a in P0}
            tempo, vt = dec.decode_clips_tempogram(cg.src(clips), f, out_mode="tempo", **q)
            tempo = cg.host(tempo)
            beats, stats, valid = _run(dec, "device", clips, f, p, "beats")
            assert np.array_equal(valid, vt)
            _same(stats[:, :, :2], tempo[:, :, :2], "bpm and lag")
            for i in range(len(clips)):
                for c in range(p["channels"]):
                    tau = int(tempo[i, c, 1])
                    one, s1, _ = _run(dec, "device", [clips[i]], f, p, "beats", bpm=bpm_of(tau, sr, hop))
                    _same(beats[i, c], one[0, c], (name, i, c, tau))
                    _same(stats[i, c, 1:], s1[0, c, 1:], (name, i, c, "stats"))
            # the other two modes at the estimated period: the chain's
            score, _, _ = _run(dec, "device", clips, f, p, "score")
            dp, _, _ = _run(dec, "device", clips, f, p, "dp")
            env, _ = _onset(dec, clips, f, p)
            for i in range(len(clips)):
                for c in range(p["channels"]):
                    tau = int(tempo[i, c, 1])
                    g, tx = tables(tau)
                    whole = ref.track(env[i, c, :int(valid[i])], f, tau, g, tx, True)
                    _same(score[i, c], whole["score"], "score at the estimated period")
                    _same(dp[i, c], whole["dp"], "dp at the estimated period")
                    _same(beats[i, c], whole["beats"], "beats at the estimated period")
    finally:
        dec.close()


def test_padding_behind_the_stream():
    """a clip that runs over its stream's end: its first `valid` columns are those of a call with n_frames = valid, everything behind
    is 0 / -1; a clip with fewer than two valid frames gives no beats"""
    name, p, f, period = "44k-mono", dict(P0), 64, 7
    hop, sr = p["hop"], 22050
    j_all = cg.j_all(p, name)
    bpm = bpm_of(period, sr, hop)
    dec = cg.decoder()
    try:
        clips = [(name, j_all - 40 * hop - 3), (name, j_all - 5)]
        for mode in ("score", "dp", "beats"):
            got, stats, valid = _run(dec, "device", clips, f, p, mode, bpm=bpm)
            assert list(valid) == [41, 1]
            short, s1, v1 = _run(dec, "device", clips[:1], 41, p, mode, bpm=bpm)
            assert v1[0] == 41
            _same(got[0, 0][..., :41], short[0, 0], mode)
            _same(stats[0], s1[0], mode)
            if mode == "score":
                assert not got[0, 0, 41:].any() and not got[1:].any()
            else:
                assert not got[0, 0, 0, 41:].any() and (got[0, 0, 1, short[0, 0, 1].size:] == -1).all()
                assert not got[1:, :, 0].any() and (got[1:, :, 1] == -1).all()
            _same(stats[1, 0], [np.float32(bpm), period, 0, -1, -1, -1, -1, 1], mode)
        assert stats[0, 0, 2] >= 1
    finally:
        dec.close()


def test_beats_of_a_periodic_stream_are_its_period_apart():
    """The stream repeats every 45 hops of 512 at 44.1 kHz.  First the reference alone, on the CPU: the oracle's decode of the
    bytes, the binary64 log-mel and envelope of section 21's definition rounded to binary32, the restatement at P = 45 (the lag
    test_gpu_clip_tempogram.py's docstring reports the reference's tempo decided at: margin 0.614 against a bound of 3e-14).
    The reference does NOT give 45 at every interval: over frames 0 .. 260 it walks back from the clip's last frame, which is a
    local maximum by the one-sided rule, and keeps 5, 50, 95, 140, 185, 221 -- four intervals of 45 and a last one of 36 that
    the clip's end cuts short (the trim drops frame 260 itself).  That is librosa's rule, not a rounding matter (section 26), so
    what is asserted is what the reference gives: every interval but the last is 45, the last is shorter.  Then the device: the
    estimated period is 45 and its beats are the reference's."""
    from oracle.oracle import Oracle
    name = "beat/periodic-44k"
    mp3, ix = cg.source(name)
    assert ix.rate == 44100 and ix.channels == 1
    p = dict(P0, sample_rate=0)
    f, start, hop, n_fft, lag = 261, 200 * 512, 512, 2048, 1
    pcm = np.frombuffer(Oracle().decode_buffer_like_cli(mp3), dtype=np.int16)
    y = (pcm.astype(np.float64) / 32768.0).astype(np.float32)[None, :]
    w = mref.filterbank(44100, n_fft, 128, 0.0, 0.0, "slaney", "slaney")
    first = start - lag * hop
    s0 = first - n_fft // 2
    t = (f + lag - 1) * hop + n_fft
    l, _ = mlref.mel_all(y[:, s0:s0 + t], s0, first, f + lag, n_fft, hop, w, 1e-10, modes=(2,))[2]
    o = tref.onset(l[0].astype(np.float32), lag, 1)[0].astype(np.float32)
    g, tx = tables(45)
    want = ref.track(o, f, 45, g, tx, True)
    wb = np.nonzero(want["beats"][0])[0]
    print("the reference: beats %s" % wb)
    assert wb.size >= 5 and set(np.diff(wb)[:-1]) == {45} and 0 < np.diff(wb)[-1] < 45, "the reference's beats are not 45 frames apart up to the last"
    dec = cg.decoder()
    try:
        beats, stats, valid = _run(dec, "device", [(name, start)], f, p, "beats")
        b = np.nonzero(beats[0, 0, 0])[0]
        print("the device: %.4f bpm, P %d, beats %s" % (stats[0, 0, 0], stats[0, 0, 1], b))
        assert valid[0] == f and stats[0, 0, 1] == 45 and stats[0, 0, 0] == np.float32(114.84375)
        assert np.array_equal(b, wb) and np.array_equal(beats[0, 0, 1, :b.size], b) and stats[0, 0, 2] == b.size
        given, s1, _ = _run(dec, "device", [(name, start)], f, p, "beats", bpm=114.84375)
        _same(given, beats, "bpm given")
    finally:
        dec.close()


def test_twice_the_same_and_alone_as_in_a_batch():
    name, p, f = "48k", dict(P0, sample_rate=0, channels=2), 57
    batch = [(name, x) for x in (1000, 50000, 7, 123456, 90000)]
    dec = cg.decoder()
    try:
        for kw in (dict(bpm=0.0, win_length=64), dict(bpm=bpm_of(22, 48000, 512))):
            for mode in ("score", "dp", "beats"):
                one, s1, v1 = _run(dec, "device", batch, f, p, mode, **kw)
                two, s2, v2 = _run(dec, "device", batch, f, p, mode, **kw)
                _same(one, two, mode)
                _same(s1, s2, mode)
                assert np.array_equal(v1, v2)
                for i in (0, 3):
                    alone, sa, va = _run(dec, "device", [batch[i]], f, p, mode, **kw)
                    _same(alone[0], one[i], (mode, i))
                    _same(sa[0], s1[i], (mode, i))
                    assert va[0] == v1[i]
    finally:
        dec.close()


def test_a_refused_clip_in_the_middle_of_a_batch_and_bad_arguments():
    from pdmp3_amd import api
    p, f = dict(P0), 30
    bad = clip_streams.replay_stream()
    bix = api.StreamIndex(bad, ISO_LSF)
    assert bix.replay
    mix = cg.ref("mixed/mpeg1-lsf")[0]
    assert not mix.one_format
    s = cg.streams()
    good = [("48k", 100), ("22k", 3000)]
    dec = cg.decoder()
    try:
        want, wstats, valid = _run(dec, "device", good, f, p, "beats", bpm=120.0)
        for kind in ("device", "numpy"):
            for mid, exc, code in (((s["mixed/mpeg1-lsf"], mix, 0), api.MixedFormat, -3), ((bad, bix, 10), api.RingReplay, -2)):
                big, view = cg.destination(kind, 3, 1, (2, f))
                stats = cg.filled(kind, (3, 1, 8))
                src = [cg.source("48k") + (100,), mid, cg.source("22k") + (3000,)]
                with pytest.raises(exc) as e:
                    dec.decode_clips_beats(src, f, out=view, stats=stats, bpm=120.0, **p)
                host = cg.host(big).reshape(3, 1, 2 * f + GUARD)
                st = cg.host(stats)
                assert e.value.valid[1] == code and (host[1] == SENT).all() and (host[:, :, 2 * f:] == SENT).all() and (st[1] == SENT).all()
                _same(host[[0, 2], :, :2 * f].reshape(2, 1, 2, f), want, kind)
                _same(st[[0, 2]], wstats, kind)
                assert np.array_equal(e.value.valid[[0, 2]], valid) and e.value.stats is stats
        # bad arguments: nothing is written
        src = [cg.source("48k") + (0,)]
        big, view = cg.destination("device", 1, 1, (2, f))
        stats = cg.filled("device", (1, 1, 8))
        for bad_a in (dict(bpm=-1.0), dict(bpm=float("nan")), dict(bpm=float("inf")), dict(bpm=1e-3), dict(bpm=1e6), dict(tightness=0.0),
                      dict(tightness=float("nan")), dict(win_length=383), dict(lag=0), dict(max_size=2), dict(n_fft=1024), dict(max_tempo=1.0), dict(width=65)):
            with pytest.raises(RuntimeError):
                dec.decode_clips_beats(src, f, out=view, stats=stats, **dict(p, **bad_a))
            assert (cg.host(big) == SENT).all() and (cg.host(stats) == SENT).all(), bad_a
        for bad_mode in ("tempo", 3, -1):
            with pytest.raises(RuntimeError):
                dec.decode_clips_beats(src, f, out=view, stats=stats, out_mode=bad_mode, **p)
        with pytest.raises(RuntimeError):
            dec.decode_clips_beats([cg.source("48k") + (-1,)], f, out=view, stats=stats, **p)
        long_big, long_view = cg.destination("device", 1, 1, (2, 32769), guard=0)
        with pytest.raises(RuntimeError):
            dec.decode_clips_beats(src, 32769, out=long_view, stats=stats, bpm=120.0, **p)
        assert (cg.host(big) == SENT).all() and (cg.host(stats) == SENT).all() and (cg.host(long_big) == SENT).all()
    finally:
        dec.close()
        bix.close()


def test_return_types_defaults_and_empty_calls():
    import torch
    from pdmp3_amd import api
    src = [cg.source("22k") + (30000,)]
    dec = cg.decoder()
    try:
        out, stats, valid = dec.decode_clips_beats(src, 100)
        assert tuple(out.shape) == (1, 1, 2, 100) and out.is_cuda and out.dtype == torch.float32 and valid[0] == 100 and valid.dtype == np.int64
        assert tuple(stats.shape) == (1, 1, 8) and stats.is_cuda and len(api.BEAT_STATS) == 8
        plain, st, _ = _run(dec, "device", [("22k", 30000)], 100, dict(P0), "beats", bpm=0.0, tightness=100.0, trim=True)   # (the defaults, spelled out)
        _same(cg.host(out), plain, "defaults")
        _same(cg.host(stats), st, "defaults")
        host = cg.host(out)[0, 0]
        k = int(st[0, 0, 2])
        assert np.isin(host[0], (0.0, 1.0)).all() and host[0].sum() == k and (np.diff(host[1, :k]) > 0).all() and (host[1, k:] == -1).all()
        out, stats, valid = dec.decode_clips_beats(src, 100, out_mode="score", channels=2, out=np.zeros((1, 2, 100), dtype=np.float32))
        assert isinstance(out, np.ndarray) and isinstance(stats, np.ndarray) and stats.shape == (1, 2, 8) and (stats[0, :, 7] == 100).all()
        out, stats, valid = dec.decode_clips_beats([], 10)
        assert tuple(out.shape) == (0, 1, 2, 10) and tuple(stats.shape) == (0, 1, 8) and valid.size == 0
        for mode, shape in (("score", (1, 1, 0)), ("dp", (1, 1, 2, 0)), ("beats", (1, 1, 2, 0))):
            out, stats, valid = dec.decode_clips_beats(src, 0, out_mode=mode)
            assert tuple(out.shape) == shape and valid[0] == 0 and torch.isnan(stats).all()
    finally:
        dec.close()
