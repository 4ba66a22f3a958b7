"""The pitch of clips on the device: decode_clips_pitch in both output modes against the binary64
definition evaluated on the product's own decode_clips_audio rows, every curve value within its derived bound, every decided
frame's lag exact, its aperiodicity within its bound and its f0 inside its interval, at most one frame in ten undecided; item
7's self-consistency of the two modes on every frame; a periodic stream, so that the threshold branch runs; determinism, batches,
refusals, more clips than one grid, types and empty calls."""
import functools

import numpy as np
import pytest

import clip_audio_ref as aref
import clip_gpu as cg
import clip_pitch_ref as ref
import clip_streams
from clip_gpu import GUARD, SENT, signal as _signal
from clip_streams import ISO_LSF

pytestmark = pytest.mark.gpu
CAP = 0.1                                          # the share of a test's frames that may be undecided


def geometry(sr, n, w, hop, tmin, tmax, threshold=0.1, channels=1):
    """decode_clips_pitch's arguments that give these lags at sr: the quotients lie half a sample from an integer"""
    from pdmp3_amd import api
    g = dict(sample_rate=sr, frame_length=n, win_length=w, hop=hop, fmin=sr / (tmax - 0.5), fmax=sr / (tmin + 0.5), threshold=threshold,
             channels=channels)
    if tmax == n - w - 1:
        g["fmin"] = sr / (tmax + 10.5)               # (the frame's own limit is what holds)
    assert api.pitch_lags(sr, frame_length=n, win_length=w, hop=hop, fmin=g["fmin"], fmax=g["fmax"])[:2] == (tmin, tmax)
    return g


DEFAULTS = dict(sample_rate=22050, frame_length=2048, win_length=1024, hop=512, fmin=65.406, fmax=2093.0, threshold=0.1, channels=1)


@functools.lru_cache(maxsize=None)
def _periodic():
    """one chunk of two MPEG-2 frames at 16 kHz, mono, no bit reservoir, forty times: once the first chunk's overlap has
    settled the decoded row repeats every 1152 samples exactly (checked with the CPU oracle; the test asserts it on the
    product's own row)"""
    from pdmp3_amd import api
    from pdmp3_amd.packer import packer
    chunk = packer.generate(n_frames=2, seed=7, version=1, sfreq=2, mode=3, bitrate_index=6, iso_strict=True, reservoir=False)
    mp3 = b"".join([chunk] * 40)
    return mp3, api.StreamIndex(mp3, ISO_LSF)


cg.STREAMS["periodic/16k"] = _periodic


def _lags(g):
    from pdmp3_amd import api
    return api.pitch_lags(g["sample_rate"], frame_length=g["frame_length"], win_length=g["win_length"], hop=g["hop"], fmin=g["fmin"], fmax=g["fmax"])


def _run(dec, kind, clips, f, g, out_mode):
    """clips: (stream name, start) -> (host copy [k, c, rows, f], valid)"""
    rows = 3 if out_mode == "pitch" else _lags(g)[1] + 1
    return cg.run(dec, "decode_clips_pitch", kind, clips, f, g["channels"], (rows, f), out_mode=out_mode, **g)


def _check(clips, sig, pitch, curve, valid, f, g):
    """every row against the definition on `sig` and against item 7 -> (worst error / bound, undecided, frames with signal,
    the largest distance of plane 0 from numpy's evaluation in ulps: the device's binary64 division is correctly rounded and
    nothing is contracted, so the callers assert 0)"""
    n, w, hop, sr = g["frame_length"], g["win_length"], g["hop"], g["sample_rate"]
    tmin, tmax, _ = _lags(g)
    worst, und, live, ulps = 0.0, 0, 0, 0
    for i, (name, s) in enumerate(clips):
        ix = cg.source(name)[1]
        j_all = aref.out_length(ix.samples, ix.rate, sr)
        assert int(valid[i]) == ref.valid(j_all, s, hop, f), (name, s, valid[i])
        s0, y = sig[i]
        lead = s0 - (s - n // 2)
        for c in range(g["channels"]):
            a, b, l = ref.check(y[c], lead, float(sr), n, w, hop, f, tmin, tmax, g["threshold"], pitch[i, c], curve[i, c])
            worst, und, live = max(worst, a), und + b, live + l
            ulps = max(ulps, ref.self_consistent(y[c], lead, sr, n, hop, f, tmin, tmax, g["threshold"], pitch[i, c], curve[i, c]))
    return worst, und, live, ulps


def _starts(name, g, f):
    """a positive lead, the middle of the stream, frames past its end"""
    ix = cg.source(name)[1]
    j_all = aref.out_length(ix.samples, ix.rate, g["sample_rate"])
    return [g["frame_length"] // 2 - 7, j_all // 3 + 11, j_all - (f // 2) * g["hop"] - 3]


CASES = {
    "n64-8k-one-tile": (lambda c: geometry(8000, 64, 32, 16, 2, 31, channels=c), "8k", 11),
    "n1024-16k-tile-edge": (lambda c: geometry(16000, 1024, 512, 256, 2, 256, channels=c), "32k", 11),
    "n1024-16k-two-tiles": (lambda c: geometry(16000, 1024, 512, 256, 2, 511, channels=c), "22k", 13),
    "defaults-22k-from-44k": (lambda c: dict(DEFAULTS, channels=c), "44k-mono", 11),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_against_binary64_on_the_products_own_signal(case):
    from pdmp3_amd import api
    make, name, f = CASES[case]
    assert f % 8 != 0
    if case == "defaults-22k-from-44k":
        assert cg.source(name)[1].rate == 44100 and _lags(make(1)) == (10, 338, 2)
    dec = cg.decoder()
    try:
        for channels in (1, 2):
            g = make(channels)
            clips = [(name, s) for s in _starts(name, g, f)]
            assert len(clips) == 3
            sig = _signal(dec, clips, f, g)
            pitch, valid = _run(dec, "device", clips, f, g, "pitch")
            curve, valid1 = _run(dec, "device", clips, f, g, "curve")
            assert np.array_equal(valid, valid1) and valid[0] == f and 0 < valid[2] < f
            worst, und, live, ulps = _check(clips, sig, pitch, curve, valid, f, g)
            frames = api.pitch_plan(g["sample_rate"], frame_length=g["frame_length"], win_length=g["win_length"], hop=g["hop"], fmin=g["fmin"],
                                    fmax=g["fmax"])[0]
            print("%s, %d channel(s) (%d frames a workgroup, %d lag tiles): worst error / bound %.4f, %d of %d frames undecided, plane 0 "
                  "within %d ulp of numpy's" % (case, channels, frames, _lags(g)[2], worst, und, live, ulps))
            assert 0.0 < worst <= 1.0 and live >= 2 * channels * (f // 2) and und <= CAP * live and ulps == 0
            for mode, dev in (("pitch", pitch), ("curve", curve)):
                host, valid2 = _run(dec, "numpy", clips, f, g, mode)
                assert np.array_equal(host.view(np.uint32), dev.view(np.uint32)) and np.array_equal(valid, valid2)
    finally:
        dec.close()


def test_a_periodic_stream_runs_the_threshold_branch():
    """N = 2048, W = 512, fmin = 10 Hz at 16 kHz: tmax = 1535 holds the period of 1152 samples, six lag tiles.  With the
    threshold at 1e-3 the only trough under it is the period itself (the CPU oracle's row: the next smallest d' is 1.5e-3)."""
    g = dict(sample_rate=16000, frame_length=2048, win_length=512, hop=512, fmin=10.0, fmax=4000.0, threshold=1e-3, channels=1)
    tmin, tmax, tiles = _lags(g)
    assert (tmin, tmax, tiles) == (4, 1535, 6)
    f, start = 11, 4608
    clips = [("periodic/16k", start)]
    dec = cg.decoder()
    try:
        (s0, y), = _signal(dec, clips, f, g)
        row = y[0]
        assert s0 == start - 1024 and np.abs(row).max() > 0.01
        assert np.array_equal(row[:-1152].view(np.uint32), row[1152:].view(np.uint32)), "the product's row is not periodic in 1152 samples"
        z = ref.frames(row, 0, 2048, 512, f)
        energy = float((row.astype(np.float64) ** 2).sum())
        for i in range(f):
            dp, bound = ref.curve(z[i], 512, tmax, energy)
            assert ref.decide(dp, tmin, tmax, g["threshold"]) == 1152 and dp[1152] == 0.0 and dp[1152] < dp[1151] and dp[1152] < dp[1153]
            assert not ref.undecided(dp, bound, tmin, tmax, g["threshold"], 1152)
        pitch, valid = _run(dec, "device", clips, f, g, "pitch")
        curve, _ = _run(dec, "device", clips, f, g, "curve")
        worst, und, live, ulps = _check(clips, [(s0, y)], pitch, curve, valid, f, g)
        print("periodic stream: worst error / bound %.4f, %d of %d frames undecided, plane 0 within %d ulp; aperiodicity %s"
              % (worst, und, live, ulps, pitch[0, 0, 1, :4]))
        assert und == 0 and live == f and 0.0 < worst <= 1.0 and ulps == 0
        assert (pitch[0, 0, 2] == 1152).all() and (np.abs(pitch[0, 0, 0] - 16000.0 / 1152.0) < 1e-3).all()
        # the same frames with librosa's threshold: an earlier trough under 0.1 is taken, as the definition takes it
        g1 = dict(g, threshold=0.1)
        pitch1, _ = _run(dec, "device", clips, f, g1, "pitch")
        worst, und, live, ulps = _check(clips, [(s0, y)], pitch1, curve, valid, f, g1)
        print("periodic stream, threshold 0.1: %d of %d frames undecided, lags %s" % (und, live, pitch1[0, 0, 2].astype(int).tolist()))
        assert und <= CAP * live and (pitch1[0, 0, 2] < 1152).all() and (pitch1[0, 0, 1] < 0.1).all()
    finally:
        dec.close()


def test_twice_the_same_and_alone_as_in_a_batch():
    g = dict(DEFAULTS, channels=2)
    f = 9
    name = "22k"
    batch = [(name, s) for s in (1000, 50000, 7, 123456, 90000)]
    dec = cg.decoder()
    try:
        for mode in ("pitch", "curve"):
            a, va = _run(dec, "device", batch, f, g, mode)
            b, vb = _run(dec, "device", batch, f, g, mode)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(va, vb)
            for i in (0, 2, 4):
                one, v1 = _run(dec, "device", [batch[i]], f, g, mode)
                assert np.array_equal(one[0].view(np.uint32), a[i].view(np.uint32)) and v1[0] == va[i]
            assert np.unique(a[:, 0, 0 if mode == "pitch" else 50, 3]).size == 5
    finally:
        dec.close()


def test_a_refused_clip_in_the_middle_of_a_batch_and_bad_arguments():
    from pdmp3_amd import api
    g = geometry(16000, 1024, 512, 256, 2, 256)
    f = 9
    bad = clip_streams.replay_stream()
    bix = api.StreamIndex(bad, ISO_LSF)
    assert bix.replay
    mix = cg.ref("mixed/mpeg1-lsf")[0]
    assert not mix.one_format
    s = cg.streams()
    good = [("48k", 100), ("22k", 3000)]
    dec = cg.decoder()
    try:
        sig = _signal(dec, good, f, g)
        want_p, _ = _run(dec, "device", good, f, g, "pitch")
        want_c, valid = _run(dec, "device", good, f, g, "curve")
        _check(good, sig, want_p, want_c, valid, f, g)
        for kind, mode, want in (("device", "pitch", want_p), ("numpy", "curve", want_c)):
            rows = want.shape[2]
            for mid, exc, code in (((s["mixed/mpeg1-lsf"], mix, 0), api.MixedFormat, -3), ((bad, bix, 10), api.RingReplay, -2)):
                big, view = cg.destination(kind, 3, 1, (rows, f))
                src = [cg.source("48k") + (100,), mid, cg.source("22k") + (3000,)]
                with pytest.raises(exc) as e:
                    dec.decode_clips_pitch(src, f, out_mode=mode, out=view, **g)
                host = cg.host(big).reshape(3, 1, rows * f + GUARD)
                assert e.value.valid[1] == code and (host[1] == SENT).all() and (host[:, :, rows * f:] == SENT).all()
                got = host[[0, 2], :, :rows * f].reshape(2, 1, rows, f)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and np.array_equal(e.value.valid[[0, 2]], valid)
        # bad arguments: nothing is written
        big, view = cg.destination("device", 1, 1, (3, f))
        src = [cg.source("48k") + (0,)]
        for bad_g in (dict(frame_length=1023), dict(frame_length=4096), dict(frame_length=62), dict(win_length=3), dict(win_length=1023),
                      dict(hop=1025), dict(hop=-2), dict(fmin=0.0), dict(fmax=g["fmin"]), dict(fmax=8000.5), dict(threshold=0.0),
                      dict(threshold=1.01), dict(fmin=100.0 * (1 + 1e-13), fmax=4000.0), dict(width=65)):
            with pytest.raises(RuntimeError):
                dec.decode_clips_pitch(src, f, out=view, **dict(g, **bad_g))
            assert (cg.host(big) == SENT).all(), bad_g
        for mode in ("contour", 2, -1):
            with pytest.raises(RuntimeError):
                dec.decode_clips_pitch(src, f, out_mode=mode, out=view, **g)
        with pytest.raises(RuntimeError):
            dec.decode_clips_pitch([cg.source("48k") + (-1,)], f, out=view, **g)
        with pytest.raises(RuntimeError):            # (rate 0 and clips of different rates)
            dec.decode_clips_pitch(src + [cg.source("32k") + (0,)], f, **dict(g, sample_rate=0))
        assert (cg.host(big) == SENT).all()
    finally:
        dec.close()
        bix.close()


def test_more_clips_than_one_grid():
    """32 768 + 5 one-frame clips at N = 64 in one call: pdmp3_hip_clip_pitch launches the kernel twice (a grid's y extent), the
    second time from descriptor 32 768 on.  Sixty-four distinct clips are held against the definition, every row is bit-equal
    to its twin among them; the last five are other clips than rows 0 .. 4, one of them behind the end"""
    g = geometry(8000, 64, 32, 16, 2, 31)
    name, k, f = "8k", 32768 + 5, 1
    mp3, ix = cg.source(name)
    assert ix.rate == 8000
    j_all = aref.out_length(ix.samples, ix.rate, ix.rate)
    starts = [1000 + 3001 * i for i in range(62)] + [j_all + 64 + 9, j_all - 5]
    assert starts[61] + 64 < j_all
    twin = (np.arange(k, dtype=np.int64) * 7) % 62
    twin[32768:] = [62, 63, 61, 60, 59]
    assert not np.any(twin[32768:] == twin[:5])
    dec = cg.decoder()
    try:
        first = [(name, s) for s in starts]
        sig = _signal(dec, first, f, g)
        base, valid64 = _run(dec, "device", first, f, g, "pitch")
        curve, _ = _run(dec, "device", first, f, g, "curve")
        worst, und, live, ulps = _check(first, sig, base, curve, valid64, f, g)
        print("sixty-four one-frame clips: worst error / bound %.4f, %d of %d frames undecided" % (worst, und, live))
        assert 0.0 < worst <= 1.0 and und <= CAP * live and ulps == 0 and live >= 40
        assert list(valid64[61:]) == [1, 0, 1] and base[62, 0, :, 0].tolist() == [0.0, 1.0, 0.0]
        big, view = cg.destination("device", k, 1, (3, f))
        out, valid = dec.decode_clips_pitch([(mp3, ix, int(starts[t])) for t in twin], f, out=view, **g)
        host = cg.host(big).reshape(k, 3 * f + GUARD)
        assert (host[:, 3 * f:] == SENT).all(), "written behind a row's floats"
        assert np.array_equal(valid, valid64[twin]) and list(valid[32768:]) == [0, 1, 1, 1, 1]
        same = (host[:, :3 * f].view(np.uint32) == base[twin].reshape(k, 3 * f).view(np.uint32)).all(axis=1)
        bad = np.flatnonzero(~same)
        assert bad.size == 0, "%d rows differ from their twins, %d of them in the second launch: %s" % (bad.size, int((bad >= 32768).sum()), bad[:8].tolist())
        assert np.unique(base[:62, 0, 0, 0]).size > 8
    finally:
        dec.close()


def test_return_types_defaults_and_empty_calls():
    import torch
    src = [cg.source("22k") + (30000,)]
    dec = cg.decoder()
    try:
        out, valid = dec.decode_clips_pitch(src, 20)
        assert tuple(out.shape) == (1, 1, 3, 20) and out.is_cuda and out.dtype == torch.float32 and valid[0] == 20 and valid.dtype == np.int64
        plain, _ = _run(dec, "device", [("22k", 30000)], 20, DEFAULTS, "pitch")       # (the defaults, spelled out)
        assert np.array_equal(cg.host(out).view(np.uint32), plain.view(np.uint32))
        lag = cg.host(out)[0, 0, 2]
        assert ((lag >= 10) & (lag <= 338)).all() and (cg.host(out)[0, 0, 0] > 0).all()
        out, valid = dec.decode_clips_pitch(src, 20, out_mode="curve", channels=2)
        assert tuple(out.shape) == (1, 2, 339, 20) and out.dtype == torch.float32 and (cg.host(out)[0, :, 0] == 1.0).all()
        out, valid = dec.decode_clips_pitch(src, 5, sample_rate=0, frame_length=1024, hop=None, win_length=None, fmin=100.0, fmax=2000.0)
        assert tuple(out.shape) == (1, 1, 3, 5) and valid[0] == 5
        out, valid = dec.decode_clips_pitch([], 10)
        assert tuple(out.shape) == (0, 1, 3, 10) and valid.size == 0
        out, valid = dec.decode_clips_pitch(src, 0)
        assert tuple(out.shape) == (1, 1, 3, 0) and valid[0] == 0
        out, valid = dec.decode_clips_pitch(src, 0, out_mode="curve")
        assert tuple(out.shape) == (1, 1, 339, 0) and valid[0] == 0
    finally:
        dec.close()
