"""Kaldi-style filterbank features of clips on the GPU (include/pdmp3_bulk.h pdmp3_amd_bulk_decode_clips_fbank, k_clip_fbank;
DESIGN.md section 11).

The reference is made from the product's own signal: for every clip decode_clips_audio gives the binary32 samples its frames
read (the span from `start` on), tests/clip_fbank_ref.py evaluates the definition on them step by step in binary64, and the
fbank call's output has to agree within the binary32 bound derived there -- every value, none left out -- and to differ from
it wherever a row holds signal (a thing compared with itself cannot pass).  Destinations are filled with a sentinel first:
nothing outside a row's F * D floats may change.  Each device step runs once.

Streams and helpers: tests/clip_gpu.py and tests/clip_gpu_calls.py."""
import ctypes as C
import math

import numpy as np
import pytest

import clip_fbank_ref as ref
import clip_forms_cases as cases
import clip_gpu as cg
import clip_gpu_calls as calls
import clip_streams
from clip_forms_cases import FBANK_CASES as CASES, FBANK_P8 as P8, FBANK_P16 as P16, FBANK_POWN as POWN, FBANK_VARIANTS as VARIANTS, SIX
from clip_gpu import GUARD, SENT
from clip_gpu_calls import fbank_check as _check, fbank_d as _d, fbank_filterbank as _filterbank, fbank_n as _n, fbank_run as _run, fbank_signal as _signal, fbank_starts as _starts
from clip_streams import ISO_LSF

pytestmark = pytest.mark.gpu
U = ref.U
LN_EPS = math.log(ref.EPS)


@pytest.mark.parametrize("case", sorted(CASES))
def test_against_binary64_on_the_products_own_signal(case):
    from pdmp3_amd import api
    p, names, f = CASES[case]
    if case == "16k-mono-batch":
        assert set(cg.ref(n)[0].rate for n in names) == {44100, 48000, 32000, 22050, 16000, 8000}
    clips = [(n, s) for n in names for s in _starts(n, p, f)]
    tile, _, lds = api.fbank_tile(p["win_length"], _n(p), p["hop"], p["num_mel_bins"])
    if case == "own-rate-1024-stereo":
        assert tile == 16 and lds > 64 * 1024      # the static-array kernel
    else:
        assert tile == 32 and lds <= 64 * 1024
    dec = cg.decoder()
    try:
        sig = _signal(dec, clips, f, p)
        for log in (True, False):
            for kind in ("device", "numpy") if log else ("device",):
                q = dict(p, use_log_fbank=log)
                got, valid = _run(dec, kind, clips, f, q)
                worst = _check(clips, sig, got, valid, f, q)
                print("%s (tile %d, LDS %d), log %d, %s: worst error / bound %.4f over %d clips of %d frames" % (case, tile, lds, log, kind, worst, len(clips), f))
                assert 0.0 < worst <= 1.0
    finally:
        dec.close()


def test_every_window_and_option():
    f = 40
    clips = [(n, s) for n in ("48k", "22k") for s in _starts(n, P16, f)[1:6]]
    dec = cg.decoder()
    try:
        sig = _signal(dec, clips, f, P16)
        for name in VARIANTS:
            p = dict(P16, **VARIANTS[name])
            got, valid = _run(dec, "device", clips, f, p)
            worst = _check(clips, sig, got, valid, f, p)
            print("%s: worst error / bound %.4f" % (name, worst))
            assert 0.0 < worst <= 1.0
    finally:
        dec.close()


@pytest.mark.parametrize("p", [P16, dict(P8, energy_floor=0.0), POWN], ids=["16k", "8k-energy", "own-rate-tile-16"])
def test_slices_are_slices(p):
    """frame f of a clip at `start` is frame 0 of a clip at start + f H, bit for bit, on both sides of both edges of a tile"""
    from pdmp3_amd import api
    tile = api.fbank_tile(p["win_length"], _n(p), p["hop"], p["num_mel_bins"])[0]
    name, start = "48k", 4321
    assert start % p["hop"] != 0
    fs = [0, 1, tile - 1, tile, tile + 1, 2 * tile - 1, 2 * tile, 2 * tile + 1, 2 * tile + 5]
    f_long = 2 * tile + 7
    dec = cg.decoder()
    try:
        for log in (True, False):
            q = dict(p, use_log_fbank=log)
            long, _ = _run(dec, "device", [(name, start)], f_long, q)
            short, _ = _run(dec, "device", [(name, start + f * p["hop"]) for f in fs], 3, q)
            for i, f in enumerate(fs):
                assert np.array_equal(long[0, :, f].view(np.uint32), short[i, :, 0].view(np.uint32)), (log, f)
                assert np.array_equal(long[0, :, f + 1].view(np.uint32), short[i, :, 1].view(np.uint32)), (log, f)
            assert np.abs(long).sum() > 0
    finally:
        dec.close()


def test_edges_of_the_tile_and_of_the_stream():
    """F and valid at 1, 15, 16, 17, 31, 32, 33; subtract_mean twice; clips wholly behind the end"""
    p = P16
    name = "32k"
    j_all = cg.j_all(p, name)
    counts = (1, 15, 16, 17, 31, 32, 33)
    dec = cg.decoder()
    try:
        for sub in (False, True):
            q = dict(p, subtract_mean=sub, use_energy=sub)
            for f in counts:
                clips = [(name, 777), (name, 0)]
                sig = _signal(dec, clips, f, q)
                got, valid = _run(dec, "device", clips, f, q)
                assert list(valid) == [f, f]
                print("F = %d, subtract_mean %d: worst error / bound %.4f" % (f, sub, _check(clips, sig, got, valid, f, q)))
            f = 35
            clips = [(name, j_all - p["win_length"] - (v - 1) * p["hop"] - 1) for v in counts]
            sig = _signal(dec, clips, f, q)
            for log in (True, False):
                r = dict(q, use_log_fbank=log)
                got, valid = _run(dec, "device", clips, f, r)
                assert list(valid) == list(counts)
                print("valid at the tile's edges, log %d, subtract_mean %d: worst error / bound %.4f" % (log, sub, _check(clips, sig, got, valid, f, r)))
                if sub:
                    again, valid2 = _run(dec, "device", clips, f, r)
                    assert np.array_equal(got.view(np.uint32), again.view(np.uint32)) and np.array_equal(valid, valid2)
        # wholly behind the end: no frame is valid, the transform of zeros, and no frame of the stream is decoded
        stats = dec.clip_stats()
        f = 35
        clips = [(name, j_all), (name, j_all + 10 ** 6), (name, 2 ** 40)]
        for sub in (False, True):
            got, valid = _run(dec, "device", clips, f, dict(p, use_log_fbank=False, use_energy=True, subtract_mean=sub))
            assert list(valid) == [0, 0, 0] and (got == 0.0).all()
            got, valid = _run(dec, "device", clips, f, dict(p, use_energy=True, energy_floor=0.0, subtract_mean=sub))
            assert list(valid) == [0, 0, 0]
            # ln eps by the device's logf: within its own c u |ln eps|
            assert (np.abs(got.astype(np.float64) - LN_EPS) <= ref.LOG_C * U * abs(LN_EPS)).all()
            assert (got == got.flat[0]).all()
        assert dec.clip_stats() == stats
        # a clip whose last samples are inside the stream but that holds no whole frame: valid 0, and its frame is not silence
        got, valid = _run(dec, "device", [(name, j_all - p["win_length"] + 1)], 2, dict(p, subtract_mean=True))
        assert list(valid) == [0] and (got[0, 0, 0] > LN_EPS + 1.0).any()
    finally:
        dec.close()


def _host_clips(p, f):
    return [(n, s) for n in ("48k", "22k", "16k-mono") for s in _starts(n, p, f)[1:4]]


def test_host_destinations():
    """a dense numpy array with a guard behind it (its rows leave the stage in one copy), pinned host memory, and stereo rows
    with a guard between the channels"""
    import pdmp3_amd
    from pdmp3_amd import api
    p, f = P16, 37
    clips = _host_clips(p, f)
    k, d = len(clips), _d(p)
    dec = cg.decoder()
    try:
        sig = _signal(dec, clips, f, p)
        src = cg.src(clips)
        flat = np.full(k * f * d + GUARD, SENT, dtype=np.float32)
        dense = flat[:k * f * d].reshape(k, 1, f, d)
        out, valid = dec.decode_clips_fbank(src, f, out=dense, **p)
        assert out is dense and (flat[k * f * d:] == SENT).all()
        print("dense numpy rows: worst error / bound %.4f" % _check(clips, sig, dense, valid, f, p))
        want = dense.copy()
        pin = api.PinnedPCM(2 * (k * f * d + GUARD))
        hip = pdmp3_amd.load_library()
        hip.pdmp3_hip_host_is_pinned.argtypes = [C.c_void_p, C.c_size_t]
        pf = pin.array.view(np.float32)
        assert hip.pdmp3_hip_host_is_pinned(pf.ctypes.data, pf.nbytes) == 1
        pf[:] = SENT
        pd = pf[:k * f * d].reshape(k, 1, f, d)
        out, valid2 = dec.decode_clips_fbank(src, f, out=pd, **p)
        assert (pf[k * f * d:] == SENT).all() and np.array_equal(valid, valid2)
        assert np.array_equal(pd.view(np.uint32), want.view(np.uint32))
        # stereo rows with a guard between the channels: one copy a channel; with the mean subtracted
        p2 = dict(p, channels=2, subtract_mean=True, use_energy=True)
        sig2 = _signal(dec, clips, f, p2)
        got, valid = _run(dec, "numpy", clips, f, p2)
        print("strided stereo numpy rows: worst error / bound %.4f" % _check(clips, sig2, got, valid, f, p2))
        got_dev, valid_dev = _run(dec, "device", clips, f, p2)
        assert np.array_equal(got.view(np.uint32), got_dev.view(np.uint32)) and np.array_equal(valid, valid_dev)
    finally:
        dec.close()


def test_a_refused_clip_in_the_middle_of_a_batch():
    from pdmp3_amd import api
    p, f = P16, 35
    d = _d(p)
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
                big, view = cg.destination(kind, 3, 1, (f, d))
                src = [(s["48k"], cg.ref("48k")[0], 100), mid, (s["22k"], cg.ref("22k")[0], 3000)]
                with pytest.raises(exc) as e:
                    dec.decode_clips_fbank(src, f, out=view, **p)
                host = cg.host(big)
                assert e.value.valid[1] == code and (host[1] == SENT).all()
                assert (host[:, :, f * d:] == SENT).all()
                got = host[[0, 2], :, :f * d].reshape(2, 1, f, d)
                _check(good, sig, got, e.value.valid[[0, 2]], f, p)
        # bad arguments: nothing is written
        big, view = cg.destination("device", 1, 1, (f, d))
        src = [(s["48k"], cg.ref("48k")[0], 0)]
        for bad_p in (dict(win_length=1), dict(win_length=1025), dict(win_length=401, round_to_power_of_two=False), dict(hop=0), dict(hop=401),
                      dict(high_freq=8000.5), dict(low_freq=-1.0), dict(preemphasis_coefficient=1.5), dict(window_type="kaiser"), dict(scale=0.0),
                      dict(energy_floor=-1.0), dict(width=65), dict(dither=1.0), dict(use_power=False), dict(raw_energy=False),
                      dict(snip_edges=False), dict(vtln_warp=1.1)):
            with pytest.raises(RuntimeError):
                dec.decode_clips_fbank(src, f, out=view, **dict(p, **bad_p))
        with pytest.raises(RuntimeError):
            dec.decode_clips_fbank([(s["48k"], cg.ref("48k")[0], -1)], f, out=view, **p)
        with pytest.raises(RuntimeError):            # (rate 0 and clips of different rates)
            dec.decode_clips_fbank(src + [(s["32k"], cg.ref("32k")[0], 0)], f, **dict(p, sample_rate=0))
        assert (cg.host(big) == SENT).all()
    finally:
        dec.close()
        bix.close()


def test_one_decoder_through_small_large_small_and_the_other_calls_after_it():
    p = dict(P16, subtract_mean=True, use_energy=True)
    small = [("32k", 500), ("8k", 1234)]
    large = [(n, s) for n in SIX for s in (0, 999, 20001)]
    fresh = cg.decoder()
    try:
        audio_before, av = calls.audio_run(fresh, "device", [("48k", 700), ("22k", 9000)], 6000, 16000, 1)
        mel_before, mv = calls.mel_run(fresh, "device", [("48k", 700), ("22k", 9000)], 40, cases.MEL_P16, "log10")
        ix = cg.ref("48k")[0]
        plain_before = fresh.decode_range(cg.streams()["48k"], ix, 33, 50).copy()
    finally:
        fresh.close()
    dec = cg.decoder()
    try:
        a, va = _run(dec, "device", small, 9, p)
        sig = _signal(dec, large, 300, p)
        b, vb = _run(dec, "device", large, 300, p)
        print("the large call: worst error / bound %.4f" % _check(large, sig, b, vb, 300, p))
        c, vc = _run(dec, "device", small, 9, p)
        assert np.array_equal(a.view(np.uint32), c.view(np.uint32)) and np.array_equal(va, vc)
        # other shapes of the tables on the same decoder, then the first again
        _run(dec, "device", small, 9, P8)
        _run(dec, "device", [("48k", 10)], 17, POWN)
        _run(dec, "device", small, 9, dict(P16, window_type="hamming", scale=32768.0))
        c, vc = _run(dec, "numpy", small, 9, p)
        assert np.array_equal(a.view(np.uint32), c.view(np.uint32))
        mel_after, mv2 = calls.mel_run(dec, "device", [("48k", 700), ("22k", 9000)], 40, cases.MEL_P16, "log10")
        assert np.array_equal(mel_before.view(np.uint32), mel_after.view(np.uint32)) and np.array_equal(mv, mv2)
        audio_after, av2 = calls.audio_run(dec, "device", [("48k", 700), ("22k", 9000)], 6000, 16000, 1)
        assert np.array_equal(audio_before.view(np.uint32), audio_after.view(np.uint32)) and np.array_equal(av, av2)
        plain_after = dec.decode_range(cg.streams()["48k"], cg.ref("48k")[0], 33, 50)
        assert np.array_equal(plain_before, plain_after)
    finally:
        dec.close()


def test_4099_clips_of_3_frames_in_one_call():
    p, f, k = dict(P16, use_energy=True), 3, 4099
    name = "mixed/mono-stereo"
    j_all = cg.j_all(p, name)
    ix = cg.ref(name)[0]
    rng = np.random.default_rng(4099)
    nw, hop = p["win_length"], p["hop"]
    starts = [0, 1, 199, 200, 201, j_all - nw - 2 * hop, j_all - nw - 2 * hop + 1, j_all - nw, j_all - nw + 1, j_all - 1, j_all, j_all + 999]
    starts += [int(x) for x in rng.integers(0, j_all + 400, k - len(starts))]
    clips = [(name, s) for s in starts]
    w = _filterbank(p, name)
    dec = cg.decoder()
    try:
        # the whole stream at 16 kHz, once: every clip's samples are slices of it (the audio call's rows are)
        whole = np.zeros((1, 1, j_all + 2048), dtype=np.float32)
        dec.decode_clips_audio([(cg.streams()[name], ix, 0)], j_all + 2048, 16000, 1, out=whole)
        got, valid = _run(dec, "device", clips, f, p)
        worst = 0.0
        for i, s in enumerate(starts):
            nv = ref.valid(j_all, s, nw, hop, f)
            assert int(valid[i]) == nv
            want, bound = ref.fbank(whole[0], 0, s, f, nw, hop, w, nv, use_energy=True, energy_floor=1.0)
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
        # torchaudio's defaults: 25 ms frames every 10 ms, 23 bins
        out, valid = dec.decode_clips_fbank([(cg.streams()["32k"], cg.ref("32k")[0], 1000)], 50)
        assert tuple(out.shape) == (1, 1, 50, 23) and out.is_cuda and valid[0] == 50
        q = dict(P16, num_mel_bins=23)
        sig = _signal(dec, [("32k", 1000)], 50, q)
        _check([("32k", 1000)], sig, cg.host(out), valid, 50, q)
        out2, _ = dec.decode_clips_fbank([(cg.streams()["32k"], cg.ref("32k")[0], 1000)], 50, frame_length=25.0, frame_shift=10.0, **dict(q, win_length=None, hop=None))
        assert np.array_equal(cg.host(out).view(np.uint32), cg.host(out2).view(np.uint32))
        out, valid = dec.decode_clips_fbank([], 10)
        assert tuple(out.shape) == (0, 1, 10, 23) and valid.size == 0
        out, valid = dec.decode_clips_fbank([(cg.streams()["32k"], cg.ref("32k")[0], 1000)], 0)
        assert tuple(out.shape) == (1, 1, 0, 23) and valid[0] == 0
    finally:
        dec.close()
