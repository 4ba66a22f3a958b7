"""Median-filter harmonic-percussive separation of clips on the GPU (include/pdmp3_bulk.h pdmp3_amd_bulk_decode_clips_hpss,
k_clip_hpss).

Two kinds of check.  Against binary64 on the product's own signal, as in test_gpu_clip_spectral.py: decode_clips_audio gives the
binary32 samples the widened clip's frames read, tests/clip_hpss_ref.py evaluates the definition on them in binary64, and every
mask has to lie within the bound derived there -- the elements whose bound is the trivial 1 (finite power) or that the
definition cannot decide (power inf) are counted, printed and capped at one in ten.  And the sharp checks, where nothing of the
transform's error remains: the medians bit for bit against np.sort on decode_clips_stft_long's own magnitudes of the widened
clip, the masks on those medians within one rounding, the masked magnitudes and the masked spectrum bit for bit.
Destinations are filled with a sentinel first.  Each device step runs once; a clip's reference is computed once.

Streams and helpers: tests/clip_gpu.py and tests/clip_gpu_calls.py."""
import math

import numpy as np
import pytest

import clip_audio_ref as aref
import clip_gpu as cg
import clip_gpu_calls as calls
import clip_hpss_ref as href
import clip_streams
from clip_gpu import GUARD, SENT
from clip_gpu_calls import mel_starts as _starts
from clip_streams import ISO_LSF

pytestmark = pytest.mark.gpu
INF = float("inf")
FT = href.TILE_FRAMES

W1764 = (np.random.default_rng(1764).random(1764, dtype=np.float32) * np.float32(1.5) - np.float32(0.25)).astype(np.float32)
PA = dict(sample_rate=0, n_fft=2048, hop=512, channels=2, kernel_size=(31, 31), power=2.0)           # the 48 kHz stream at its own rate
PB = dict(sample_rate=22050, n_fft=2048, hop=441, channels=1, win_length=1764, window=W1764, kernel_size=(17, 5), power=1.0, margin=(2.0, 3.5))
PC = dict(sample_rate=0, n_fft=4096, hop=1024, channels=1, kernel_size=(31, 31), power=INF)
PC24 = dict(PC, sample_rate=24000)              # ... the 48 kHz stream at 24 kHz: the band that holds its energy ("what was tried")
PD = dict(sample_rate=0, n_fft=2048, hop=2048, channels=1, kernel_size=(3, 31), power=2.0)
PE = dict(sample_rate=0, n_fft=2048, hop=1, channels=1, kernel_size=(31, 3), power=2.0)


def _margins(p):
    m = p.get("margin", 1.0)
    return m if isinstance(m, tuple) else (m, m)


def _run(dec, kind, clips, f, p, mode="mask"):
    """clips: (stream name, start) -> (host copy [k, c, 2, K, f] (complex: [.., 2]), valid)"""
    nb = p["n_fft"] // 2 + 1
    return cg.run(dec, "decode_clips_hpss", kind, clips, f, p["channels"], (2, nb, f, 2) if mode == "complex" else (2, nb, f), mode=mode, **p)


def _signal(dec, clips, f, p):
    """the binary32 samples the widened clips' frames read, from the product's own audio call: per clip (s0, y [C, T])"""
    rh = p["kernel_size"][0] // 2
    return cg.signal(dec, clips, f, p, front=rh, back=rh)


def _wants(clips, sig, f, p):
    """per clip clip_hpss_ref.hpss's result: the definition on the product's own signal"""
    (lh, lp), (mh, mp) = p["kernel_size"], _margins(p)
    return [href.hpss(y, s0, s, f, p["n_fft"], p["hop"], lh, lp, p["power"], mh, mp, p.get("win_length"), p.get("window"))
            for (n, s), (s0, y) in zip(clips, sig)]


def _check(clips, wants, got, valid, f, p):
    """every mask against the definition -> (worst error / bound, loose elements, elements)"""
    worst, loose, total = 0.0, 0, 0
    for i, (n, s) in enumerate(clips):
        ix = cg.ref(n)[0]
        j_all = aref.out_length(ix.samples, ix.rate, cg.rate(p, n))
        assert int(valid[i]) == href.sref.valid(j_all, s, p["hop"], f), (n, s, valid[i])
        w, l, t = href.check_masks(got[i], wants[i], p["power"])
        print("  %s at %d: worst error / bound %.4f, %d of %d elements %s" % (n, s, w, l, t, "undecided" if math.isinf(p["power"]) else "with the trivial bound"))
        worst, loose, total = max(worst, w), loose + l, total + t
    return worst, loose, total


CASES = {
    "a-48k-stereo-2048-hop-512-31-31-power-2": (PA, "48k", 96),
    "b-22k-2048-hop-441-own-window-1764-17-5-power-1-margins": (PB, "22k", 96),
    "c-48k-at-24k-4096-hop-1024-31-31-power-inf": (PC24, "48k", 96),
    "d-44k-mono-2048-hop-2048-3-31": (PD, "44k-mono", 96),
    "e-32k-2048-hop-1-31-3": (PE, "32k", 96),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_against_binary64_on_the_products_own_signal(case):
    from pdmp3_amd import api
    p, name, f = CASES[case]
    assert FT < f < 2 * FT and api.hpss_plan(*p["kernel_size"])[2:4] == (64, FT) and (p["n_fft"] // 2 + 1) % 64 == 1
    clips = [(name, s) for s in _starts(name, p, f)]
    dec = cg.decoder()
    try:
        sig = _signal(dec, clips, f, p)
        wants = _wants(clips, sig, f, p)
        for kind in ("device", "numpy"):
            got, valid = _run(dec, kind, clips, f, p)
            worst, loose, total = _check(clips, wants, got, valid, f, p)
            print("%s, %s: worst error / bound %.4f over %d clips of %d frames; %d of %d elements (%.2f %%) %s"
                  % (case, kind, worst, len(clips), f, loose, total, 100.0 * loose / total,
                     "undecided" if math.isinf(p["power"]) else "with the trivial bound"))
            assert loose <= href.CAP * total and worst <= 1.0
            assert math.isinf(p["power"]) or worst > 0.0
    finally:
        dec.close()


@pytest.mark.parametrize("p", [PA, PC], ids=["2048-hop-512-stereo", "4096-hop-1024"])
def test_the_sharp_check_on_the_spectrum_calls_own_output(p):
    """mode 3 against np.sort medians of decode_clips_stft_long(mode="magnitude") for the widened clip, bit for bit; mode 0 against
    item 4 on those medians within one rounding (exactly at inf); modes 1 and 2 against mode 0 times that call's magnitude and
    complex output, bit for bit.  The starts are rh hop and later: the spectrum call takes no clip that begins before the stream"""
    name, f = "48k", 96
    (lh, lp), rh, hop = p["kernel_size"], p["kernel_size"][0] // 2, p["hop"]
    ix = cg.ref(name)[0]
    clips = [(name, s) for s in (rh * hop, rh * hop + 57, ix.samples // 3 + 11, ix.samples - 40 * hop - 3, ix.samples + rh * hop + 3)]
    wide = cg.src([(n, s - rh * hop) for n, s in clips])
    long = dict(sample_rate=0, n_fft=p["n_fft"], hop=hop, channels=p["channels"])
    dec = cg.decoder()
    try:
        mag = cg.host(dec.decode_clips_stft_long(wide, f + 2 * rh, mode="magnitude", **long)[0])              # [k, c, K, f + 2 rh]
        cplx = cg.host(dec.decode_clips_stft_long(wide, f + 2 * rh, mode="complex", **long)[0])
        cplx = np.ascontiguousarray(cplx).view(np.float32).reshape(cplx.shape + (2,))
        med, valid = _run(dec, "device", clips, f, p, "median")
        hm, pm = href.medians(mag, lh, lp)
        assert hm.dtype == np.float32 and np.array_equal(med[:, :, 0].view(np.uint32), hm.view(np.uint32)), "the harmonic median"
        assert np.array_equal(med[:, :, 1].view(np.uint32), pm.view(np.uint32)), "the percussive median"
        assert list(valid[:3]) == [f, f, f] and 0 < valid[3] < f and valid[4] == 0 and np.unique(hm).size > 1000
        centre = mag[:, :, None, :, rh:rh + f]
        for power, margin in ((2.0, 1.0), (INF, (2.0, 3.5)), (1.0, (2.0, 3.5))):
            q = dict(p, power=power, margin=margin)
            m0, _ = _run(dec, "device", clips, f, q, "mask")
            want, bound = href.from_medians(med[:, :, 0], med[:, :, 1], *_margins(q), power)
            err = np.abs(m0.astype(np.float64) - want)
            assert (err <= bound).all(), (power, float((err - bound).max()), np.unravel_index(np.argmax(err - bound), err.shape))
            print("N %d power %s margins %s: worst |mask - item 4 on the medians| / bound %.4f" % (p["n_fft"], power, _margins(q),
                                                                                               float((err / np.maximum(bound, 1e-300)).max())))
            if math.isinf(power):
                assert np.array_equal(m0, want.astype(np.float32))
            if power == 2.0:
                m1, _ = _run(dec, "device", clips, f, q, "magnitude")
                assert np.array_equal(m1.view(np.uint32), (centre * m0).view(np.uint32)), "mode 1 is not mode 0 times the magnitude"
                m2, _ = _run(dec, "device", clips, f, q, "complex")
                want2 = cplx[:, :, None, :, rh:rh + f] * m0[..., None]
                assert np.array_equal(m2.view(np.uint32), want2.view(np.uint32)), "mode 2 is not mode 0 times the complex spectrum"
                assert (m0[4] == np.float32(0.5)).all() and (m1[4].view(np.uint32) == 0).all()      # behind the end: silence
    finally:
        dec.close()


@pytest.mark.parametrize("p", [PA, PC], ids=["2048-hop-512-stereo", "4096-hop-1024"])
def test_frames_are_frames(p):
    """frame f of a clip at `start` is frame 0 of the clip at start + f H, bit for bit, on both sides of both tile edges"""
    name, start = "48k", 4321
    assert start % p["hop"] != 0
    fs = [0, 1, FT - 1, FT, FT + 1, 2 * FT - 1, 2 * FT, 2 * FT + 2]
    f_long = 2 * FT + 4
    q = dict(p, power=2.0)
    dec = cg.decoder()
    try:
        long, _ = _run(dec, "device", [(name, start)], f_long, q)
        short, _ = _run(dec, "device", [(name, start + f * p["hop"]) for f in fs], 2, q)
        for i, f in enumerate(fs):
            assert np.array_equal(long[0, ..., f].view(np.uint32), short[i, ..., 0].view(np.uint32)), f
            assert np.array_equal(long[0, ..., f + 1].view(np.uint32), short[i, ..., 1].view(np.uint32)), f
        assert np.unique(long).size > 1000
    finally:
        dec.close()


def test_slices_of_a_batch_are_the_batchs_slices():
    p, f = dict(PB, sample_rate=16000), 11
    clips = [(n, s) for n in ("48k", "22k", "16k-mono") for s in (0, 5000, 23457)]
    dec = cg.decoder()
    try:
        whole, valid = _run(dec, "device", clips, f, p)
        for a, b in ((0, 1), (2, 5), (4, 9), (8, 9)):
            part, v = _run(dec, "device", clips[a:b], f, p)
            assert np.array_equal(part.view(np.uint32), whole[a:b].view(np.uint32)) and np.array_equal(v, valid[a:b]), (a, b)
        assert np.unique(whole).size > 1000
    finally:
        dec.close()


def test_a_refused_clip_in_the_middle_of_a_batch_and_bad_arguments():
    from pdmp3_amd import api
    p, f = dict(PA, sample_rate=16000, channels=1, kernel_size=(9, 7)), 9
    bad = clip_streams.replay_stream()
    bix = api.StreamIndex(bad, ISO_LSF)
    assert bix.replay
    mix = cg.ref("mixed/mpeg1-lsf")[0]
    assert not mix.one_format
    s = cg.streams()
    good = [("48k", 100), ("22k", 3000)]
    nb = p["n_fft"] // 2 + 1
    per = 2 * nb * f
    dec = cg.decoder()
    try:
        sig = _signal(dec, good, f, p)
        wants = _wants(good, sig, f, p)
        for kind in ("device", "numpy"):
            for mid, exc, code in (((s["mixed/mpeg1-lsf"], mix, 0), api.MixedFormat, -3), ((bad, bix, 10), api.RingReplay, -2)):
                big, view = cg.destination(kind, 3, 1, (2, nb, f))
                src = [(s["48k"], cg.ref("48k")[0], 100), mid, (s["22k"], cg.ref("22k")[0], 3000)]
                with pytest.raises(exc) as e:
                    dec.decode_clips_hpss(src, f, out=view, **p)
                host = cg.host(big).reshape(3, 1, per + GUARD)
                assert e.value.valid[1] == code and (host[1] == SENT).all()
                assert (host[:, :, per:] == SENT).all()
                got = host[[0, 2], :, :per].reshape(2, 1, 2, nb, f)
                worst, loose, total = _check(good, wants, got, e.value.valid[[0, 2]], f, p)
                assert loose <= href.CAP * total
        # bad arguments: nothing is written
        big, view = cg.destination("device", 1, 1, (2, nb, f))
        src = [(s["48k"], cg.ref("48k")[0], 0)]
        nan_window = np.ones(2048, dtype=np.float32)
        nan_window[123] = np.nan
        nan = float("nan")
        for bad_p in (dict(n_fft=1024), dict(n_fft=8192), dict(n_fft=400), dict(hop=0), dict(hop=2049), dict(win_length=2049), dict(window=nan_window),
                      dict(kernel_size=30), dict(kernel_size=33), dict(kernel_size=(31, 1)), dict(kernel_size=(2, 31)), dict(kernel_size=(31, 35)),
                      dict(margin=0.5), dict(margin=(1.0, nan)), dict(margin=INF), dict(power=0.5), dict(power=3.0), dict(power=nan), dict(power=-INF),
                      dict(width=65)):
            q = dict(p, **bad_p)
            if q["n_fft"] != 2048:
                with pytest.raises((RuntimeError, AssertionError)):            # (another n_fft is another shape: `out` does not fit either)
                    dec.decode_clips_hpss(src, f, out=view, **q)
                with pytest.raises(RuntimeError):
                    dec.decode_clips_hpss(src, f, **q)
            else:
                with pytest.raises(RuntimeError):
                    dec.decode_clips_hpss(src, f, out=view, **q)
            assert (cg.host(big) == SENT).all(), bad_p
        for bad_mode in (4, -1, "power"):
            with pytest.raises(RuntimeError):
                dec.decode_clips_hpss(src, f, out=view, mode=bad_mode, **p)
        with pytest.raises(RuntimeError):
            dec.decode_clips_hpss(src, -1, **p)
        with pytest.raises(RuntimeError):
            dec.decode_clips_hpss([(s["48k"], cg.ref("48k")[0], -1)], f, out=view, **p)
        with pytest.raises(RuntimeError):            # (rate 0 and clips of different rates)
            dec.decode_clips_hpss(src + [(s["32k"], cg.ref("32k")[0], 0)], f, **dict(p, sample_rate=0))
        # a row of the output beyond 2^31 - 1 floats, straight at the library: refused, nothing written
        import ctypes as C
        a8 = api._as_u8(s["48k"])
        arr = (api._AudioClip * 1)(api._AudioClip(a8.ctypes.data, len(s["48k"]), cg.ref("48k")[0].h, 0, view.data_ptr(), 0))
        got = (C.c_longlong * 1)()
        for mode, frames in ((0, 2 ** 31 // 2050 + 1), (2, 2 ** 31 // 4100 + 1), (3, 2 ** 40)):
            spec, keep = api._hpss_spec(frames, 16000, channels=1, mode=mode)
            assert dec.lib.pdmp3_amd_bulk_decode_clips_hpss(dec.h, arr, 1, C.byref(spec), got) == -1, (mode, frames)
        assert (cg.host(big) == SENT).all()
    finally:
        dec.close()
        bix.close()


def test_clips_wholly_behind_the_end_return_types_and_empty_calls():
    import torch
    p, f = PA, 5
    name = "48k"
    ix = cg.ref(name)[0]
    j_all = aref.out_length(ix.samples, ix.rate, ix.rate)
    clips = [(name, j_all + 5 * p["n_fft"] + 15 * p["hop"]), (name, j_all + 1000000)]
    nb = p["n_fft"] // 2 + 1
    dec = cg.decoder()
    try:
        got, valid = _run(dec, "device", clips, f, p)
        assert (valid == 0).all() and (got == np.float32(0.5)).all()                 # margins 1, a finite power: exactly 0.5
        got, valid = _run(dec, "device", clips, f, dict(p, margin=(1.0, 2.0)))
        assert (valid == 0).all() and (got.view(np.uint32) == 0).all()               # other margins: exactly +0
        got, valid = _run(dec, "device", clips, f, dict(p, power=INF))
        assert (valid == 0).all() and (got.view(np.uint32) == 0).all()
        for mode in ("magnitude", "complex", "median"):
            got, valid = _run(dec, "numpy", clips, f, p, mode)
            assert (valid == 0).all() and (got.view(np.uint32) == 0).all(), mode
        out, valid = dec.decode_clips_hpss(cg.src(clips), f, sample_rate=0)
        assert tuple(out.shape) == (2, 2, 2, nb, f) and out.is_cuda and out.dtype == torch.float32 and (valid == 0).all()
        out, valid = dec.decode_clips_hpss(cg.src(clips), f, sample_rate=0, mode="complex")
        assert tuple(out.shape) == (2, 2, 2, nb, f) and out.is_cuda and out.dtype == torch.complex64 and (valid == 0).all()
        out, valid = dec.decode_clips_hpss([], 10)
        assert tuple(out.shape) == (0, 1, 2, nb, 10) and valid.size == 0
        out, valid = dec.decode_clips_hpss(cg.src(clips), 0, sample_rate=0, n_fft=4096, channels=1)
        assert tuple(out.shape) == (2, 1, 2, 2049, 0) and (valid == 0).all()
    finally:
        dec.close()


def test_more_clips_than_one_grid():
    """32 768 + 5 clips of one frame at (2048, 2048), kernels (3, 3), mode 3, in one call: pdmp3_hip_clip_hpss launches the kernel
    twice (a grid's y extent), the second time from descriptor 32 768 on.  Sixty-four distinct clips are held by the sharp check --
    np.sort on the spectrum call's magnitudes of the widened clip --, every row is bit-equal to its twin among them; the last
    five are other clips than rows 0 .. 4, one of them behind the end"""
    name, k = "32k", 32768 + 5
    p = dict(sample_rate=0, n_fft=2048, hop=2048, channels=1, kernel_size=(3, 3), power=2.0)
    nb = 1025
    ix = cg.ref(name)[0]
    j_all = aref.out_length(ix.samples, ix.rate, ix.rate)
    starts = [3000 + 3001 * i for i in range(62)] + [j_all + 7, j_all - 1]
    assert starts[61] + 2 * 2048 < j_all and starts[0] >= 2048
    twin = (np.arange(k, dtype=np.int64) * 7) % 62
    twin[32768:] = [62, 63, 61, 60, 59]
    assert not np.any(twin[32768:] == twin[:5])
    mp3 = cg.streams()[name]
    dec = cg.decoder()
    try:
        first = [(name, s) for s in starts]
        base, valid64 = _run(dec, "device", first, 1, p, "median")
        mag = cg.host(dec.decode_clips_stft_long(cg.src([(n, s - 2048) for n, s in first]), 3, mode="magnitude", sample_rate=0, n_fft=2048, hop=2048,
                                                   channels=1)[0])
        hm, pm = href.medians(mag, 3, 3)
        assert np.array_equal(base[:, :, 0].view(np.uint32), hm.view(np.uint32)) and np.array_equal(base[:, :, 1].view(np.uint32), pm.view(np.uint32))
        assert list(valid64[61:]) == [1, 0, 1]
        big, view = cg.destination("device", k, 1, (2, nb, 1))
        out, valid = dec.decode_clips_hpss([(mp3, ix, int(starts[t])) for t in twin], 1, mode="median", out=view, **p)
        host = cg.host(big)
        assert (host[:, :, 2 * nb:] == SENT).all(), "written behind a row's floats"
        assert np.array_equal(valid, valid64[twin]) and list(valid[32768:]) == [0, 1, 1, 1, 1]
        bad = np.flatnonzero((host[:, 0, :2 * nb].view(np.uint32) != base[twin, 0].reshape(k, 2 * nb).view(np.uint32)).any(axis=1))
        assert bad.size == 0, "%d rows differ from their twins, %d of them in the second launch: %s" % (bad.size, int((bad >= 32768).sum()), bad[:8].tolist())
        assert np.unique(base[:62, 0, 0, 100, 0]).size > 32
    finally:
        dec.close()


def test_one_decoder_through_this_call_the_other_calls_and_this_call_again():
    """the new call, decode_clips_stft_long, decode_clips_mel_long, decode_clips_audio, the new call with other parameters and
    with the other n_fft -- and all of it again: every call is bit-equal to its first answer; the transform's tables are shared
    with the spectrum and the log-mel call, the stage with the tempogram call"""
    small = [("32k", 500), ("8k", 1234)]
    pa = dict(PA, sample_rate=16000, channels=1)
    pb = dict(pa, kernel_size=(5, 17), power=1.0, margin=(1.5, 1.0), win_length=1764, window=W1764)
    pc = dict(PC, sample_rate=16000)
    dec = cg.decoder()
    try:
        def once():
            return [_run(dec, "device", small, 9, pa),
                    calls.stft_long_run(dec, "device", small, 9, dict(calls.STFT_LONG_PA, sample_rate=16000, channels=1), "complex"),
                    calls.mel_long_run(dec, "device", small, 9, dict(calls.MEL_LONG_PA, sample_rate=16000, channels=1), "log10"),
                    calls.audio_run(dec, "device", [("48k", 700), ("22k", 9000)], 6000, 16000, 1),
                    _run(dec, "device", small, 9, pb, "complex"),
                    _run(dec, "numpy", small, 5, pc, "magnitude")]
        a, b = once(), once()
        for i, ((x, vx), (y, vy)) in enumerate(zip(a, b)):
            assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)) and np.array_equal(vx, vy), i
            assert np.abs(x.astype(np.float64)).sum() > 0, i
        sig = _signal(dec, small, 9, pa)
        worst, loose, total = _check(small, _wants(small, sig, 9, pa), a[0][0], a[0][1], 9, pa)
        print("after the other calls: worst error / bound %.4f, %d of %d elements with the trivial bound" % (worst, loose, total))
    finally:
        dec.close()
