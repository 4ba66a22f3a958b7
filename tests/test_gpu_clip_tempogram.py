"""Onset strength, tempogram and tempo of clips on the device: decode_clips_tempogram's three modes, each
against the binary64 definition evaluated on what the product itself returns one stage earlier -- the envelope on
decode_clips_mel_long's values (and, at a stream's start and end, on the full chain from decode_clips_audio's rows), the
tempogram on mode "onset" of the widened clip, the tempo on mode "tempogram" -- every value within its derived bound; slices of a
longer clip bit for bit; a periodic stream whose answer is known; determinism, batches, refusals, more clips than one grid,
destinations, types and empty calls.

Measured on an MI355X (worst error / bound, printed by the tests): see profiles/clip_tempogram.txt."""
import functools

import numpy as np
import pytest

import clip_gpu as cg
import clip_mel_long_ref as mlref
import clip_mel_ref as mref
import clip_streams
import clip_tempogram_ref as ref
from clip_gpu import GUARD, SENT
from clip_streams import ISO_LSF

pytestmark = pytest.mark.gpu
MODES = ("onset", "tempogram", "tempo")
P0 = dict(sample_rate=22050, n_fft=2048, hop=512, n_mels=128, lag=1, max_size=1, win_length=384, channels=1)      # the defaults, spelled out


@functools.lru_cache(maxsize=None)
def _periodic():
    """one chunk of twenty MPEG-1 frames at 44.1 kHz, mono, no bit reservoir, fifteen times: once the first chunk's overlap has
    settled the decoded row repeats every 23 040 samples = 45 hops of 512.  The CPU oracle's decode of these bytes, through the
    binary64 definition (log-mel, envelope, tempogram, tempo on the tempogram rounded to binary32), is decided at lag 45 by the
    margin rule: margin 0.614 against a bound of 3e-14 (lags 44 and 46 follow, then 90)."""
    from pdmp3_amd import api
    from pdmp3_amd.packer import packer
    chunk = packer.generate(n_frames=20, seed=7, sfreq=0, mode=3, bitrate_index=7, reservoir=False)
    mp3 = b"".join([chunk] * 15)
    return mp3, api.StreamIndex(mp3, ISO_LSF)


cg.STREAMS["periodic/44k"] = _periodic


def _shape(p, f, mode):
    return {"onset": (1, f), "tempogram": (p["win_length"], f), "tempo": (1, 4)}[mode]


def _run(dec, kind, clips, f, p, mode, **kw):
    """clips: (stream name, start) -> (host copy [k, c, f], [k, c, wt, f] or [k, c, 4], valid); the guard floats behind every
    row are looked at"""
    k, c = len(clips), p["channels"]
    nb, inner = _shape(p, f, mode)
    big, view = cg.destination(kind, k, c, (nb, inner))
    dst = view if mode == "tempogram" else view[:, :, 0]
    out, valid = dec.decode_clips_tempogram(cg.src(clips), f, out_mode=mode, out=dst, **dict(p, **kw))
    assert out is dst
    per = nb * inner
    host = cg.host(big).reshape(k, c, per + GUARD)
    assert (host[:, :, per:] == SENT).all(), "written behind a row's floats"
    got = host[:, :, :per].copy()
    return (got.reshape(k, c, nb, inner) if mode == "tempogram" else got), valid


def _mel(dec, clips, f, p, floor=1e-10):
    """decode_clips_mel_long's log10 values of the clips -> [k, c, n_mels, f]"""
    q = {a: p[a] for a in ("sample_rate", "n_fft", "hop", "n_mels", "channels")}
    out, valid = dec.decode_clips_mel_long(cg.src(clips), f, mode="log10", floor=floor, **q)
    return cg.host(out)


def _valid(clips, valid, f, p):
    for i, (name, s) in enumerate(clips):
        assert int(valid[i]) == ref.valid(cg.j_all(p, name), s, p["hop"], f), (name, s, valid[i])


# ---- mode 0 against the definition on decode_clips_mel_long's own output ----
ONSET_CASES = {
    "mono-128-max1-lag1": ("44k-mono", dict(P0)),
    "stereo-40-max3-lag2": ("48k", dict(P0, sample_rate=0, channels=2, n_mels=40, max_size=3, lag=2)),
    "mono-40-max1-lag2": ("22k", dict(P0, n_mels=40, lag=2)),
    "stereo-128-max3-lag1": ("48k", dict(P0, sample_rate=0, channels=2, max_size=3)),
}


@pytest.mark.parametrize("case", sorted(ONSET_CASES))
def test_onset_against_binary64_on_the_log_mel_calls_own_values(case):
    name, p = ONSET_CASES[case]
    f, lag, hop = 261, p["lag"], p["hop"]              # (a workgroup of 256 lanes and five more)
    j_all = cg.j_all(p, name)
    clips = [(name, s) for s in (lag * hop, 12345, j_all - 200 * hop - 3)]
    dec = cg.decoder()
    try:
        l = _mel(dec, [(n, s - lag * hop) for n, s in clips], f + lag, p)
        worst = 0.0
        for kind in ("device", "numpy"):
            got, valid = _run(dec, kind, clips, f, p, "onset")
            _valid(clips, valid, f, p)
            assert valid[0] == f and 0 < valid[2] < f
            for i in range(len(clips)):
                for c in range(p["channels"]):
                    want, bound = ref.onset(l[i, c], lag, p["max_size"])
                    err = np.abs(got[i, c].astype(np.float64) - want)
                    assert (err <= bound).all(), (case, kind, i, c, float((err / bound).max()), int(np.argmax(err / bound)))
                    worst = max(worst, float((err / bound).max()))
            assert (got >= 0.0).all() and (got[:2] > 0.0).mean() > 0.5 and (got[2, :, 215:] == 0.0).all()
        print("%s: worst error / bound %.4f" % (case, worst))
        assert 0.0 < worst <= 1.0
    finally:
        dec.close()


# ---- mode 0 against the full chain from decode_clips_audio's rows, at a stream's start and over its end ----
@pytest.mark.parametrize("case", ["mono-128-max1-lag1", "stereo-40-max3-lag2"])
def test_onset_against_the_full_chain_at_a_streams_start_and_end(case):
    name, p = ONSET_CASES[case]
    f, lag, hop, n, c, floor = 11, p["lag"], p["hop"], p["n_fft"], p["channels"], 1e-6
    j_all = cg.j_all(p, name)
    clips = [(name, 0), (name, hop - 1), (name, j_all - 4 * hop - 7)]
    w = mref.filterbank(cg.rate(p, name), n, p["n_mels"], 0.0, 0.0, "slaney", "slaney")
    dec = cg.decoder()
    try:
        got, valid = _run(dec, "device", clips, f, p, "onset", floor=floor)
        _valid(clips, valid, f, p)
        assert valid[0] == f and valid[2] == 5
        t = (f + lag - 1) * hop + n
        worst = 0.0
        for i, (nm, s) in enumerate(clips):
            first = s - lag * hop                        # the centre of the first log-mel frame: before sample 0 in clips 0 and 1
            s0 = max(0, first - n // 2)
            y = np.full((1, c, t), SENT, dtype=np.float32)
            dec.decode_clips_audio([cg.source(nm) + (s0,)], t, p["sample_rate"], c, out=y)
            l, dl = mlref.mel_all(y[0], s0, first, f + lag, n, hop, w, floor, modes=(2,))[2]
            for ch in range(c):
                want, bound = ref.onset(l[ch], lag, p["max_size"])
                bound = bound + ref.onset_chain_bound(dl[ch], lag, p["max_size"])
                err = np.abs(got[i, ch].astype(np.float64) - want)
                assert (err <= bound).all(), (case, i, ch, float((err / bound).max()), int(np.argmax(err / bound)))
                worst = max(worst, float((err / bound).max()))
            if i < 2:
                assert first < 0 and (got[i] > 0).any()
        assert (got[2, :, 7:] == 0.0).all()              # (frames that read nothing of the stream: the log-mel is at its floor)
        print("%s, the full chain: worst error / bound %.4f" % (case, worst))
        assert 0.0 < worst <= 1.0
    finally:
        dec.close()


# ---- mode 1 against the definition on mode 0's own output of the widened clip ----
@pytest.mark.parametrize("wt,hop", [(16, 512), (272, 64), (384, 64)])
def test_tempogram_against_binary64_on_the_onset_modes_own_values(wt, hop):
    name = "44k-mono"
    p = dict(P0, win_length=wt, hop=hop, n_mels=40, channels=2, lag=2, max_size=3)
    wh = wt // 2
    j_all = cg.j_all(p, name)
    dec = cg.decoder()
    try:
        worst, dead = 0.0, 0
        for f in (7, 9, 17):
            # the stream's start (the window reaches frames in front of sample 0), its middle, over its end, wholly behind it
            clips = [(name, wh * hop), (name, 40000 + f), (name, j_all - 3 * hop), (name, j_all + 2048 + (wh + 3) * hop)]
            env, _ = _run(dec, "device", [(n, s - wh * hop) for n, s in clips], f + wt - 1, p, "onset")
            got, valid = _run(dec, "device", clips, f, p, "tempogram")
            _valid(clips, valid, f, p)
            for i in range(len(clips)):
                for c in range(2):
                    want, bound = ref.tempogram(env[i, c], wt, f)
                    err = np.abs(got[i, c].astype(np.float64) - want)
                    assert (err <= bound).all(), (wt, hop, f, i, c, float((err - bound).max()), np.unravel_index(np.argmax(err - bound), err.shape))
                    live = bound[0] > 0
                    assert (got[i, c][:, ~live] == 0.0).all() and not np.signbit(got[i, c][:, ~live]).any() and (got[i, c][0, live] == 1.0).all()
                    dead += int((~live).sum())
                    if live.any():
                        worst = max(worst, float((err[:, live] / bound[:, live]).max()))
            assert (got[3] == 0.0).all() and (env[3] == 0.0).all() and valid[3] == 0 and (got[0, :, 0] == 1.0).all()
            host, v2 = _run(dec, "numpy", clips, f, p, "tempogram")
            assert np.array_equal(host.view(np.uint32), got.view(np.uint32)) and np.array_equal(valid, v2)
        print("Wt %d, hop %d: worst error / bound %.4f, %d frames of zeros" % (wt, hop, worst, dead))
        assert 0.0 < worst <= 1.0 and dead >= 3 * 2 * 7
    finally:
        dec.close()


# ---- slices ----
def test_a_clip_is_the_slice_of_a_longer_one():
    """the clip (s, F) is columns a .. of the clip (s - a H, F + a), bit for bit: first of decode_clips_mel_long, then of modes 0
    and 1"""
    name, f = "44k-mono", 13
    p = dict(P0, win_length=272, n_mels=40, channels=1, max_size=3)
    hop = p["hop"]
    dec = cg.decoder()
    try:
        for s, a in ((20000, 1), (20000, 9), (200 * hop + 5, 16), (136 * hop, 3)):
            short, long = [(name, s)], [(name, s - a * hop)]
            assert np.array_equal(_mel(dec, short, f, p).view(np.uint32), _mel(dec, long, f + a, p)[..., a:].view(np.uint32)), (s, a)
            for mode in ("onset", "tempogram"):
                x, _ = _run(dec, "device", short, f, p, mode)
                y, _ = _run(dec, "device", long, f + a, p, mode)
                assert np.array_equal(x.view(np.uint32), y[..., a:].view(np.uint32)), (mode, s, a)
                assert np.abs(x).sum() > 0
    finally:
        dec.close()


# ---- mode 2 ----
def test_tempo_of_a_periodic_stream_is_its_period():
    p = dict(P0, sample_rate=0)
    f, start = 200, 250 * 512
    clips = [("periodic/44k", start)]
    assert cg.source("periodic/44k")[1].rate == 44100
    pr, first = ref.prior(44100, 512, 384)
    dec = cg.decoder()
    try:
        tg, valid = _run(dec, "device", clips, f, p, "tempogram")
        got, v2 = _run(dec, "device", clips, f, p, "tempo")
        assert valid[0] == f == v2[0]
        want = ref.tempo(tg[0, 0], pr, 44100, 512)
        decided, r = ref.check_tempo(want, got[0, 0])
        print("periodic stream: tau* %d, %.4f bpm, s %.4f, margin %.4f (the definition's %.4f), bound %.3g, error / bound %.4f"
              % (got[0, 0, 1], got[0, 0, 0], got[0, 0, 2], got[0, 0, 3], want["margin"], want["bound"], r))
        assert decided and r <= 1.0 and want["tau"] == 45 and got[0, 0, 1] == 45.0 and got[0, 0, 0] == np.float32(114.84375)
        assert got[0, 0, 3] > 0.3
        # the tempogram itself says so: the period's row is the largest mean behind the lags next to lag 0
        mean = tg[0, 0].astype(np.float64).mean(axis=1)
        assert int(np.argmax(mean[20:])) + 20 == 45 and mean[45] > 0.85
    finally:
        dec.close()


def test_tempo_is_the_definition_on_the_tempogram_modes_own_values():
    """noise streams: no tempo is claimed; plane by plane the four floats are the definition's on mode 1's output, the lag exact
    where the margin decides it and within the bound of the maximum elsewhere"""
    dec = cg.decoder()
    try:
        for p, name, f in ((dict(P0, channels=2, sample_rate=0), "48k", 57), (dict(P0, win_length=16, n_mels=40, lag=2, max_size=3), "22k", 9),
                           (dict(P0, win_length=1024, hop=64, n_mels=40, start_bpm=300.0, std_bpm=2.0, max_tempo=4000.0), "44k-mono", 17)):
            wt, hop, sr = p["win_length"], p["hop"], cg.rate(p, name)
            clips = [(name, s) for s in ((wt // 2 + 16) * hop, (wt // 2) * hop + 60001, cg.j_all(p, name) - 5 * hop)]
            kw = {a: p[a] for a in ("start_bpm", "std_bpm", "max_tempo") if a in p}
            pr, first = ref.prior(sr, hop, wt, **kw)
            tg, valid = _run(dec, "device", clips, f, p, "tempogram")
            got, v2 = _run(dec, "numpy", clips, f, p, "tempo")
            assert np.array_equal(valid, v2)
            # (the tempogram of these shapes -- Wt 1024 runs the kernel on its static array -- is the definition's too)
            env, _ = _run(dec, "device", [(n, s - (wt // 2) * hop) for n, s in clips], f + wt - 1, p, "onset")
            for i in range(len(clips)):
                for c in range(p["channels"]):
                    t64, b64 = ref.tempogram(env[i, c], wt, f)
                    assert (np.abs(tg[i, c].astype(np.float64) - t64) <= b64).all(), (name, wt, i, c)
            worst, n_dec = 0.0, 0
            for i in range(len(clips)):
                for c in range(p["channels"]):
                    decided, r = ref.check_tempo(ref.tempo(tg[i, c], pr, sr, hop), got[i, c])
                    worst, n_dec = max(worst, r), n_dec + int(decided)
                    assert got[i, c, 1] >= first and got[i, c, 0] == np.float32(60.0 * sr / (hop * float(got[i, c, 1])))
            print("%s, Wt %d: worst error / bound %.4f, %d of %d decided" % (name, wt, worst, n_dec, len(clips) * p["channels"]))
            assert worst <= 1.0
    finally:
        dec.close()


# ---- plumbing ----
def test_twice_the_same_and_alone_as_in_a_batch():
    p = dict(P0, channels=2, win_length=272, n_mels=40)
    f = 9
    batch = [("22k", s) for s in (136 * 512 + 1000, 100000, 136 * 512, 123456, 90000)]
    dec = cg.decoder()
    try:
        for mode in MODES:
            a, va = _run(dec, "device", batch, f, p, mode)
            b, vb = _run(dec, "device", batch, f, p, mode)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(va, vb)
            for i in (0, 2, 4):
                one, v1 = _run(dec, "device", [batch[i]], f, p, mode)
                assert np.array_equal(one[0].view(np.uint32), a[i].view(np.uint32)) and v1[0] == va[i]
            if mode != "tempo":
                assert np.unique(a[:, 0, 3] if mode == "onset" else a[:, 0, 100, 3]).size == 5
    finally:
        dec.close()


def test_a_refused_clip_in_the_middle_of_a_batch_and_bad_arguments():
    from pdmp3_amd import api
    p = dict(P0, win_length=16, n_mels=40)
    f = 9
    bad = clip_streams.replay_stream()
    bix = api.StreamIndex(bad, ISO_LSF)
    assert bix.replay
    mix = cg.ref("mixed/mpeg1-lsf")[0]
    assert not mix.one_format
    s = cg.streams()
    good = [("48k", 9000), ("22k", 30000)]
    dec = cg.decoder()
    try:
        for kind, mode in (("device", "onset"), ("numpy", "tempogram"), ("device", "tempo")):
            want, valid = _run(dec, "device", good, f, p, mode)
            nb, inner = _shape(p, f, mode)
            per = nb * inner
            for mid, exc, code in (((s["mixed/mpeg1-lsf"], mix, 0), api.MixedFormat, -3), ((bad, bix, 10), api.RingReplay, -2)):
                big, view = cg.destination(kind, 3, 1, (nb, inner))
                src = [cg.source("48k") + (9000,), mid, cg.source("22k") + (30000,)]
                with pytest.raises(exc) as e:
                    dec.decode_clips_tempogram(src, f, out_mode=mode, out=view if mode == "tempogram" else view[:, :, 0], **p)
                host = cg.host(big).reshape(3, 1, per + GUARD)
                assert e.value.valid[1] == code and (host[1] == SENT).all() and (host[:, :, per:] == SENT).all()
                got = host[[0, 2], :, :per].reshape(want.shape)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and np.array_equal(e.value.valid[[0, 2]], valid)
        # bad arguments: nothing is written
        src = [cg.source("48k") + (9000,)]
        for mode in MODES:
            nb, inner = _shape(p, f, mode)
            big, view = cg.destination("device", 1, 1, (nb, inner))
            dst = view if mode == "tempogram" else view[:, :, 0]
            for bad_p in (dict(lag=0), dict(lag=17), dict(max_size=2), dict(max_size=11), dict(start_bpm=0.0), dict(std_bpm=float("nan")),
                          dict(max_tempo=float("inf")), dict(max_tempo=1.0), dict(n_fft=1024), dict(hop=0), dict(n_mels=0), dict(floor=0.0),
                          dict(f_max=12000.0), dict(width=65)):
                with pytest.raises(RuntimeError):
                    dec.decode_clips_tempogram(src, f, out_mode=mode, out=dst, **dict(p, **bad_p))
                assert (cg.host(big) == SENT).all(), (mode, bad_p)
            with pytest.raises(RuntimeError):
                dec.decode_clips_tempogram([cg.source("48k") + (-1,)], f, out_mode=mode, out=dst, **p)
            with pytest.raises(RuntimeError):            # (rate 0 and clips of different rates)
                dec.decode_clips_tempogram(src + [cg.source("32k") + (0,)], f, out_mode=mode, **dict(p, sample_rate=0))
            assert (cg.host(big) == SENT).all()
        big, view = cg.destination("device", 1, 1, (1, f))
        for mode in ("bpm", 3, -1):
            with pytest.raises(RuntimeError):
                dec.decode_clips_tempogram(src, f, out_mode=mode, out=view[:, :, 0], **p)
        for wt in (14, 17, 1026):
            with pytest.raises(RuntimeError):
                dec.decode_clips_tempogram(src, f, out_mode="onset", out=view[:, :, 0], **dict(p, win_length=wt))
        assert (cg.host(big) == SENT).all()
    finally:
        dec.close()
        bix.close()


def test_more_clips_than_one_grid():
    """32 768 + 5 one-frame clips in one call of mode "onset": pdmp3_hip_clip_mel_long and pdmp3_hip_clip_tempogram launch their
    kernels twice (a grid's y extent), the second time from descriptor 32 768 on.  Sixty-four distinct clips are held against
    the definition on the log-mel call's values, every row is bit-equal to its twin among them; the last five are other clips
    than rows 0 .. 4, one of them behind the end"""
    name, k, f = "32k", 32768 + 5, 1
    p = dict(P0, sample_rate=0, hop=64, n_mels=8, lag=1, max_size=3)
    mp3, ix = cg.source(name)
    j_all = cg.j_all(p, name)
    starts = [1000 + 3001 * i for i in range(62)] + [j_all + 2048 + 9, j_all - 5]
    assert starts[61] + 2048 < j_all
    twin = (np.arange(k, dtype=np.int64) * 7) % 62
    twin[32768:] = [62, 63, 61, 60, 59]
    assert not np.any(twin[32768:] == twin[:5])
    dec = cg.decoder()
    try:
        first = [(name, s) for s in starts]
        l = _mel(dec, [(n, s - 64) for n, s in first], 2, p)
        base, valid64 = _run(dec, "device", first, f, p, "onset")
        for i in range(64):
            want, bound = ref.onset(l[i, 0], 1, 3)
            assert abs(float(base[i, 0, 0]) - want[0]) <= bound[0], i
        assert list(valid64[61:]) == [1, 0, 1] and base[62, 0, 0] == 0.0 and np.unique(base[:62, 0, 0]).size > 8
        big, view = cg.destination("device", k, 1, (1, f))
        out, valid = dec.decode_clips_tempogram([(mp3, ix, int(starts[t])) for t in twin], f, out_mode="onset", out=view[:, :, 0], **p)
        host = cg.host(big).reshape(k, f + GUARD)
        assert (host[:, f:] == SENT).all(), "written behind a row's floats"
        assert np.array_equal(valid, valid64[twin]) and list(valid[32768:]) == [0, 1, 1, 1, 1]
        bad = np.flatnonzero(host[:, 0].view(np.uint32) != base[twin, 0, 0].view(np.uint32))
        assert bad.size == 0, "%d rows differ from their twins, %d of them in the second launch: %s" % (bad.size, int((bad >= 32768).sum()), bad[:8].tolist())
    finally:
        dec.close()


def test_return_types_defaults_and_empty_calls():
    import torch
    src = [cg.source("22k") + (120000,)]
    dec = cg.decoder()
    try:
        out, valid = dec.decode_clips_tempogram(src, 20)
        assert tuple(out.shape) == (1, 1, 384, 20) and out.is_cuda and out.dtype == torch.float32 and valid[0] == 20 and valid.dtype == np.int64
        plain, _ = _run(dec, "device", [("22k", 120000)], 20, P0, "tempogram")        # (the defaults, spelled out)
        assert np.array_equal(cg.host(out).view(np.uint32), plain.view(np.uint32)) and (plain[0, 0, 0] == 1.0).all()
        out, valid = dec.decode_clips_tempogram(src, 20, out_mode="onset", channels=2)
        assert tuple(out.shape) == (1, 2, 20) and (cg.host(out) >= 0).all()
        out, valid = dec.decode_clips_tempogram(src, 20, out_mode="tempo")
        assert tuple(out.shape) == (1, 1, 4) and 8 < cg.host(out)[0, 0, 1] < 384
        pinned = torch.full((1, 1, 4), float(SENT)).pin_memory()
        out2, _ = dec.decode_clips_tempogram(src, 20, out_mode="tempo", out=pinned)
        assert np.array_equal(pinned.numpy().view(np.uint32), cg.host(out).view(np.uint32))
        for mode, shape in (("onset", (0, 1, 10)), ("tempogram", (0, 1, 384, 10)), ("tempo", (0, 1, 4))):
            out, valid = dec.decode_clips_tempogram([], 10, out_mode=mode)
            assert tuple(out.shape) == shape and valid.size == 0
        for mode, shape in (("onset", (1, 1, 0)), ("tempogram", (1, 1, 384, 0))):
            out, valid = dec.decode_clips_tempogram(src, 0, out_mode=mode)
            assert tuple(out.shape) == shape and valid[0] == 0
        big, view = cg.destination("device", 1, 1, (1, 4))
        out, valid = dec.decode_clips_tempogram(src, 0, out_mode="tempo", out=view[:, :, 0])
        assert valid[0] == 0 and (cg.host(big) == SENT).all()                       # (no frames: nothing but valid is written)
    finally:
        dec.close()
