"""Log-mel features of clips on the GPU (include/pdmp3_bulk.h pdmp3_amd_bulk_decode_clips_mel, k_clip_mel; DESIGN.md
section 10).

The reference is made from the product's own signal: for every clip decode_clips_audio gives the binary32 samples its frames
read (the span from max(0, start - N / 2) on), tests/clip_mel_ref.py evaluates the definition on them in binary64, and the mel
call's output has to agree within the binary32 bound derived there -- every value, none left out; the bound is 0 on silence
in mode 0.  Destinations are filled with a sentinel first: nothing outside a row's n_mels * F floats may change.  Each device
step runs once.

Streams and helpers: tests/clip_gpu.py and tests/clip_gpu_calls.py."""
import ctypes as C
import math

import numpy as np
import pytest

import clip_audio_ref as aref
import clip_gpu as cg
import clip_gpu_calls as calls
import clip_mel_ref as ref
import clip_streams
from clip_forms_cases import MEL_CASES as CASES, MEL_P16 as P16, MEL_P24 as P24, MEL_P48 as P48
from clip_gpu import GUARD, SENT, signal as _signal
from clip_gpu_calls import MEL_MODES as MODES, mel_check as _check, mel_filterbank as _filterbank, mel_run as _run, mel_starts as _starts
from clip_streams import ISO_LSF

pytestmark = pytest.mark.gpu
U = ref.U


@pytest.mark.parametrize("case", sorted(CASES))
def test_against_binary64_on_the_products_own_signal(case):
    from pdmp3_amd import api
    p, names, f = CASES[case]
    if case == "16k-mono-batch":
        assert set(cg.ref(n)[0].rate for n in names) == {44100, 48000, 32000, 22050, 16000, 8000}
    clips = [(n, s) for n in names for s in _starts(n, p, f)]
    tile = api.mel_tile(p["n_fft"], p["hop"], p["n_mels"])[0]
    dec = cg.decoder()
    try:
        sig = _signal(dec, clips, f, p)
        for mode in MODES:
            for kind in ("device", "numpy") if mode == "log10" else ("device",):
                got, valid = _run(dec, kind, clips, f, p, mode)
                worst = _check(clips, sig, got, valid, f, p, mode)
                print("%s (tile %d), mode %s, %s: worst error / bound %.4f over %d clips of %d frames" % (case, tile, mode, kind, worst, len(clips), f))
                assert 0.0 < worst <= 1.0
    finally:
        dec.close()


@pytest.mark.parametrize("p", [P16, P24], ids=["16k", "24k-stereo"])
def test_slices_are_slices(p):
    """frame f of a clip at `start` is frame 0 of a clip at start + f H, bit for bit, on both sides of the kernel's tile edges"""
    from pdmp3_amd import api
    tile = api.mel_tile(p["n_fft"], p["hop"], p["n_mels"])[0]
    name, start = "48k", 4321
    assert start % p["hop"] != 0
    fs = [0, 1, tile - 1, tile, tile + 1, 2 * tile - 1, 2 * tile, 2 * tile + 1, 2 * tile + 5]
    f_long = 2 * tile + 7
    dec = cg.decoder()
    try:
        for mode in MODES[:3]:
            long, _ = _run(dec, "device", [(name, start)], f_long, p, mode)
            short, _ = _run(dec, "device", [(name, start + f * p["hop"]) for f in fs], 3, p, mode)
            for i, f in enumerate(fs):
                assert np.array_equal(long[0, :, :, f].view(np.uint32), short[i, :, :, 0].view(np.uint32)), (mode, f)
                assert np.array_equal(long[0, :, :, f + 1].view(np.uint32), short[i, :, :, 1].view(np.uint32)), (mode, f)
            assert np.abs(long).sum() > 0
    finally:
        dec.close()


def test_edges_of_the_tile_and_of_the_stream():
    """F and valid at the tile size and one either side of it, and at 1; clips wholly behind the end"""
    from pdmp3_amd import api
    p = P16
    tile = api.mel_tile(p["n_fft"], p["hop"], p["n_mels"])[0]
    name = "32k"
    ix = cg.ref(name)[0]
    j_all = aref.out_length(ix.samples, ix.rate, 16000)
    dec = cg.decoder()
    try:
        for f in (1, tile - 1, tile, tile + 1):
            clips = [(name, 777), (name, 0)]
            sig = _signal(dec, clips, f, p)
            got, valid = _run(dec, "device", clips, f, p, "log10")
            assert list(valid) == [f, f]
            print("F = %d: worst error / bound %.4f" % (f, _check(clips, sig, got, valid, f, p, "log10")))
        f = tile + 2
        clips = [(name, j_all - (v - 1) * p["hop"] - 1) for v in (1, tile - 1, tile, tile + 1)]
        sig = _signal(dec, clips, f, p)
        for mode in ("power", "log10"):
            got, valid = _run(dec, "device", clips, f, p, mode)
            assert list(valid) == [1, tile - 1, tile, tile + 1]
            print("valid at the tile's edges, mode %s: worst error / bound %.4f" % (mode, _check(clips, sig, got, valid, f, p, mode)))
        # wholly behind the end: the transform of zeros
        stats = dec.clip_stats()
        clips = [(name, j_all + p["n_fft"] // 2), (name, j_all + 10 ** 6), (name, 2 ** 40)]
        for mode, floor in (("power", 1e-10), ("log", 1e-10), ("log10", 1e-10), ("log10", 3e-5), ("whisper", 1e-10)):
            got, valid = _run(dec, "device", clips, f, p, mode, floor)
            assert list(valid) == [0, 0, 0]
            fl = float(np.float32(floor))
            want = {"power": 0.0, "log": math.log(fl), "log10": math.log10(fl), "whisper": (math.log10(fl) + 4.0) / 4.0}[mode]
            # the definition on silence: its bound is 0 in mode 0 and the logarithm's own c u (mode 3: its two roundings more) else
            w64, bound = ref.mel(np.zeros((1, 8)), 0, 10 ** 6, f, p["n_fft"], p["hop"], _filterbank(p, name), MODES.index(mode), floor)
            lg = abs(math.log(fl) if mode == "log" else math.log10(fl))
            cap = {"power": 0.0, "log": ref.LOG_C * U * lg, "log10": ref.LOG_C * U * lg,
                   "whisper": (ref.LOG_C * U * lg + U * (lg + 8.0) + U * abs(4.0 - lg)) / 4.0 * (1.0 + 4.0 * U)}[mode]
            assert np.allclose(w64, want, rtol=1e-15, atol=0) and np.allclose(bound, cap, rtol=1e-12, atol=0)
            if mode == "power":
                assert (got == 0.0).all() and (bound == 0.0).all()
            else:
                assert (np.abs(got.astype(np.float64) - w64[None]) <= bound[None]).all(), (mode, floor)
        assert dec.clip_stats() == stats
    finally:
        dec.close()


def _host_clips(p, f):
    return [(n, s) for n in ("48k", "22k", "16k-mono") for s in _starts(n, p, f)[1:4]]


def test_host_destinations():
    """a dense numpy array (its rows leave the stage in one copy), one with a guard behind it, and pinned host memory"""
    import pdmp3_amd
    from pdmp3_amd import api
    p, f = P16, 37
    clips = _host_clips(p, f)
    k, nm = len(clips), p["n_mels"]
    dec = cg.decoder()
    try:
        sig = _signal(dec, clips, f, p)
        src = cg.src(clips)
        flat = np.full(k * nm * f + GUARD, SENT, dtype=np.float32)
        dense = flat[:k * nm * f].reshape(k, 1, nm, f)
        out, valid = dec.decode_clips_mel(src, f, out=dense, **p)
        assert out is dense and (flat[k * nm * f:] == SENT).all()
        print("dense numpy rows: worst error / bound %.4f" % _check(clips, sig, dense, valid, f, p, "log10"))
        want = dense.copy()
        pin = api.PinnedPCM(2 * (k * nm * f + GUARD))
        hip = pdmp3_amd.load_library()
        hip.pdmp3_hip_host_is_pinned.argtypes = [C.c_void_p, C.c_size_t]
        pf = pin.array.view(np.float32)
        assert hip.pdmp3_hip_host_is_pinned(pf.ctypes.data, pf.nbytes) == 1
        pf[:] = SENT
        pd = pf[:k * nm * f].reshape(k, 1, nm, f)
        out, valid2 = dec.decode_clips_mel(src, f, out=pd, **p)
        assert (pf[k * nm * f:] == SENT).all() and np.array_equal(valid, valid2)
        assert np.array_equal(pd.view(np.uint32), want.view(np.uint32))
        # stereo rows with a guard between the channels: one copy a channel
        p2 = dict(p, channels=2)
        sig2 = _signal(dec, clips, f, p2)
        got, valid = _run(dec, "numpy", clips, f, p2, "log10")
        print("strided stereo numpy rows: worst error / bound %.4f" % _check(clips, sig2, got, valid, f, p2, "log10"))
    finally:
        dec.close()


def test_a_refused_clip_in_the_middle_of_a_batch():
    from pdmp3_amd import api
    p, f = P16, 35
    bad = clip_streams.replay_stream()
    bix = api.StreamIndex(bad, ISO_LSF)
    assert bix.replay
    mix = cg.ref("mixed/mpeg1-lsf")[0]
    assert not mix.one_format
    s = cg.streams()
    good = [("48k", 100), ("22k", 3000)]
    dec = cg.decoder()
    try:
        sig = _signal(dec, good, f, p)
        for kind in ("device", "numpy"):
            for mid, exc, code in (((s["mixed/mpeg1-lsf"], mix, 0), api.MixedFormat, -3), ((bad, bix, 10), api.RingReplay, -2)):
                big, view = cg.destination(kind, 3, 1, (p["n_mels"], f))
                src = [(s["48k"], cg.ref("48k")[0], 100), mid, (s["22k"], cg.ref("22k")[0], 3000)]
                with pytest.raises(exc) as e:
                    dec.decode_clips_mel(src, f, out=view, **p)
                host = cg.host(big)
                assert e.value.valid[1] == code and (host[1] == SENT).all()
                assert (host[:, :, p["n_mels"] * f:] == SENT).all()
                got = host[[0, 2], :, :p["n_mels"] * f].reshape(2, 1, p["n_mels"], f)
                _check(good, sig, got, e.value.valid[[0, 2]], f, p, "log10")
        # bad arguments: nothing is written
        big, view = cg.destination("device", 1, 1, (p["n_mels"], f))
        src = [(s["48k"], cg.ref("48k")[0], 0)]
        for bad_p in (dict(n_fft=401), dict(n_fft=2048), dict(hop=0), dict(hop=401), dict(f_max=8000.5), dict(floor=0.0), dict(width=65)):
            with pytest.raises(RuntimeError):
                dec.decode_clips_mel(src, f, out=view, **dict(p, **bad_p))
        with pytest.raises(RuntimeError):
            dec.decode_clips_mel([(s["48k"], cg.ref("48k")[0], -1)], f, out=view, **p)
        with pytest.raises(RuntimeError):            # (rate 0 and clips of different rates)
            dec.decode_clips_mel(src + [(s["32k"], cg.ref("32k")[0], 0)], f, **dict(p, sample_rate=0))
        assert (cg.host(big) == SENT).all()
    finally:
        dec.close()
        bix.close()


def test_one_decoder_through_small_large_small_and_the_other_calls_after_it():
    p = P16
    small = [("32k", 500), ("8k", 1234)]
    large = [(n, s) for n in ("mixed/mono-stereo", "48k", "32k", "22k", "16k-mono", "8k") for s in (0, 999, 20001)]
    fresh = cg.decoder()
    try:
        audio_before, av = calls.audio_run(fresh, "device", [("48k", 700), ("22k", 9000)], 6000, 16000, 1)
        ix = cg.ref("48k")[0]
        plain_before = fresh.decode_range(cg.streams()["48k"], ix, 33, 50).copy()
    finally:
        fresh.close()
    dec = cg.decoder()
    try:
        a, va = _run(dec, "device", small, 9, p, "log10")
        sig = _signal(dec, large, 300, p)
        b, vb = _run(dec, "device", large, 300, p, "log10")
        print("the large call: worst error / bound %.4f" % _check(large, sig, b, vb, 300, p, "log10"))
        c, vc = _run(dec, "device", small, 9, p, "log10")
        assert np.array_equal(a.view(np.uint32), c.view(np.uint32)) and np.array_equal(va, vc)
        # other shapes of the tables on the same decoder, then the first again
        _run(dec, "device", small, 9, P24, "power")
        _run(dec, "device", [("48k", 10)], 17, P48, "whisper")
        c, vc = _run(dec, "numpy", small, 9, p, "log10")
        assert np.array_equal(a.view(np.uint32), c.view(np.uint32))
        audio_after, av2 = calls.audio_run(dec, "device", [("48k", 700), ("22k", 9000)], 6000, 16000, 1)
        assert np.array_equal(audio_before.view(np.uint32), audio_after.view(np.uint32)) and np.array_equal(av, av2)
        plain_after = dec.decode_range(cg.streams()["48k"], cg.ref("48k")[0], 33, 50)
        assert np.array_equal(plain_before, plain_after)
    finally:
        dec.close()


def test_4099_clips_of_3_frames_in_one_call():
    p, f, k = P16, 3, 4099
    name = "mixed/mono-stereo"
    ix = cg.ref(name)[0]
    j_all = aref.out_length(ix.samples, ix.rate, 16000)
    rng = np.random.default_rng(4099)
    starts = [0, 1, 199, 200, 201, j_all - 1, j_all, j_all + 999] + [int(x) for x in rng.integers(0, j_all + 400, k - 8)]
    clips = [(name, s) for s in starts]
    w = _filterbank(p, name)
    dec = cg.decoder()
    try:
        # the whole stream at 16 kHz, once: every clip's samples are slices of it (the audio call's rows are)
        whole = np.zeros((1, 1, j_all + 2048), dtype=np.float32)
        dec.decode_clips_audio([(cg.streams()[name], ix, 0)], j_all + 2048, 16000, 1, out=whole)
        got, valid = _run(dec, "device", clips, f, p, "log10")
        worst = 0.0
        for i, s in enumerate(starts):
            assert int(valid[i]) == ref.valid(j_all, s, p["hop"], f)
            want, bound = ref.mel(whole[0], 0, s, f, p["n_fft"], p["hop"], w, 2, 1e-10)
            err = np.abs(got[i].astype(np.float64) - want)
            assert (err <= bound).all(), (i, s, float((err - bound).max()))
            worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max(initial=0.0)))
        print("%d clips of %d frames in one call: worst error / bound %.4f" % (k, f, worst))
        assert 0.0 < worst <= 1.0
    finally:
        dec.close()


def test_made_output_and_empty_calls():
    dec = cg.decoder()
    try:
        out, valid = dec.decode_clips_mel([(cg.streams()["32k"], cg.ref("32k")[0], 1000)], 50)
        assert tuple(out.shape) == (1, 1, 80, 50) and out.is_cuda and valid[0] == 50
        sig = _signal(dec, [("32k", 1000)], 50, P16)
        _check([("32k", 1000)], sig, cg.host(out), valid, 50, P16, "log10")
        out, valid = dec.decode_clips_mel([], 10)
        assert tuple(out.shape) == (0, 1, 80, 10) and valid.size == 0
        out, valid = dec.decode_clips_mel([(cg.streams()["32k"], cg.ref("32k")[0], 1000)], 0)
        assert tuple(out.shape) == (1, 1, 80, 0) and valid[0] == 0
    finally:
        dec.close()
