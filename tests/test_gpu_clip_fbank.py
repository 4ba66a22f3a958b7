"""Kaldi-style filterbank features of clips on the GPU (include/pdmp3_bulk.h pdmp3_amd_bulk_decode_clips_fbank, k_clip_fbank;
DESIGN.md section 11).

The reference is made from the product's own signal: for every clip decode_clips_audio gives the binary32 samples its frames
read (the span from `start` on), tests/clip_fbank_ref.py evaluates the definition on them step by step in binary64, and the
fbank call's output has to agree within the binary32 bound derived there -- every value, none left out -- and to differ from
it wherever a row holds signal (a thing compared with itself cannot pass).  Destinations are filled with a sentinel first:
nothing outside a row's F * D floats may change.  Each device step runs once.

Streams and helpers: those of test_gpu_clip_audio.py."""
import ctypes as C
import math

import numpy as np
import pytest

import clip_audio_ref as aref
import clip_fbank_ref as ref
import clip_streams
import test_gpu_clip_audio as tga
from clip_streams import ISO_LSF

pytestmark = pytest.mark.gpu
SENT = np.float32(-1234.5)
GUARD = 24
U = ref.U
LN_EPS = math.log(ref.EPS)

P16 = dict(sample_rate=16000, win_length=400, hop=160, num_mel_bins=80, channels=1)
P8 = dict(sample_rate=8000, win_length=200, hop=80, num_mel_bins=23, channels=1, use_energy=True, htk_compat=True, scale=32768.0)
POWN = dict(sample_rate=0, win_length=1024, hop=480, num_mel_bins=80, channels=2)          # the own rate (the 48 kHz stream), stereo
PEQ = dict(sample_rate=16000, win_length=400, hop=160, num_mel_bins=40, channels=1, round_to_power_of_two=False)
SIX = ["mixed/mono-stereo", "48k", "32k", "22k", "16k-mono", "8k"]


def _rate(p, name):
    return p["sample_rate"] or tga._ref(name)[0].rate


def _n(p):
    return ref.dft_length(p["win_length"], p.get("round_to_power_of_two", True))


def _d(p):
    return p["num_mel_bins"] + int(p.get("use_energy", False))


def _filterbank(p, name):
    return ref.filterbank(_rate(p, name), _n(p), p["num_mel_bins"], p.get("low_freq", 20.0), p.get("high_freq", 0.0))


def _definition(y, start, f, p, w, nv):
    return ref.fbank(y, start, start, f, p["win_length"], p["hop"], w, nv, p.get("round_to_power_of_two", True), p.get("remove_dc_offset", True),
                     p.get("preemphasis_coefficient", 0.97), p.get("window_type", "povey"), p.get("blackman_coeff", 0.42),
                     int(p.get("use_log_fbank", True)), p.get("use_energy", False), p.get("htk_compat", False), p.get("energy_floor", 1.0),
                     p.get("subtract_mean", False), p.get("scale", 1.0))


def _destination(kind, k, c, f, d, guard=GUARD):
    """a sentinel-filled [k, c, f * d + guard] buffer and its [k, c, f, d] view (rows and channels strided)"""
    per = f * d
    if kind == "device":
        import torch
        big = torch.full((k, c, per + guard), float(SENT), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        return big, big.as_strided((k, c, f, d), (c * (per + guard), per + guard, d, 1))
    big = np.full((k, c, per + guard), SENT, dtype=np.float32)
    return big, np.lib.stride_tricks.as_strided(big, (k, c, f, d), (4 * c * (per + guard), 4 * (per + guard), 4 * d, 4))


def _run(dec, kind, clips, f, p):
    """clips: (stream name, start) -> (host copy [k, c, f, d], valid)"""
    k, c, d = len(clips), p["channels"], _d(p)
    big, view = _destination(kind, k, c, f, d)
    out, valid = dec.decode_clips_fbank([(tga._streams()[n], tga._ref(n)[0], s) for n, s in clips], f, out=view, **p)
    assert out is view
    host = tga._host(big)
    assert (host[:, :, f * d:] == SENT).all(), "written behind a row's floats"
    return host[:, :, :f * d].reshape(k, c, f, d), valid


def _signal(dec, clips, f, p):
    """the binary32 samples the clips' frames read, from the product's own audio call: per clip y [C, T] from `start` on"""
    t = (f - 1) * p["hop"] + p["win_length"]
    y = np.full((len(clips), p["channels"], t), SENT, dtype=np.float32)
    dec.decode_clips_audio([(tga._streams()[n], tga._ref(n)[0], s) for n, s in clips], t, _rate(p, clips[0][0]), p["channels"], out=y)
    return list(y)


def _check(clips, sig, got, valid, f, p):
    """every row against the definition on `sig`; -> worst error / bound over the rows that hold signal"""
    worst = 0.0
    for i, (n, s) in enumerate(clips):
        ix = tga._ref(n)[0]
        j_all = aref.out_length(ix.samples, ix.rate, _rate(p, n))
        nv = ref.valid(j_all, s, p["win_length"], p["hop"], f)
        assert int(valid[i]) == nv, (n, s, valid[i], nv)
        want, bound = _definition(sig[i], s, f, p, _filterbank(p, n), nv)
        err = np.abs(got[i].astype(np.float64) - want)
        assert (err <= bound).all(), "%s at %d: error beyond the bound by %g at %s" % (
            n, s, float((err - bound).max()), np.unravel_index(np.argmax(err - bound), err.shape))
        nz = bound > 0
        if not p.get("use_log_fbank", True) and not p.get("subtract_mean", False):
            assert (got[i][~nz] == 0.0).all()
        if p.get("subtract_mean", False) and nv == 1 and f == 1:
            # the only frame minus the mean of that one frame: x - x / 1, exactly 0.0 in the definition and in binary32 alike,
            # so no error can show here; the row is held to that instead
            assert (want == 0.0).all() and (got[i] == 0.0).all(), (n, s)
        elif np.abs(sig[i]).sum() > 0:
            r = float((err[nz] / bound[nz]).max())
            assert 0.0 < r <= 1.0, (n, s, r)
            worst = max(worst, r)
    return worst


def _j(name, p):
    ix = tga._ref(name)[0]
    return aref.out_length(ix.samples, ix.rate, _rate(p, name))


def _starts(name, p, f):
    j_all = _j(name, p)
    return [0, 57, j_all // 3 + 11, max(j_all - (f // 2) * p["hop"] - 3, 0), j_all - p["win_length"] // 2, j_all + 3, j_all + 5 * p["win_length"]]


CASES = {
    "16k-mono-batch": (P16, SIX, 70),
    "8k-energy-htk-int16": (P8, ["48k", "22k", "8k"], 45),
    "own-rate-1024-stereo": (POWN, ["48k"], 21),
    "n-equals-nw": (PEQ, ["32k", "16k-mono"], 40),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_against_binary64_on_the_products_own_signal(case):
    from pdmp3_amd import api
    p, names, f = CASES[case]
    if case == "16k-mono-batch":
        assert set(tga._ref(n)[0].rate for n in names) == {44100, 48000, 32000, 22050, 16000, 8000}
    clips = [(n, s) for n in names for s in _starts(n, p, f)]
    tile, _, lds = api.fbank_tile(p["win_length"], _n(p), p["hop"], p["num_mel_bins"])
    if case == "own-rate-1024-stereo":
        assert tile == 16 and lds > 64 * 1024      # the static-array kernel
    else:
        assert tile == 32 and lds <= 64 * 1024
    dec = tga._decoder()
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


VARIANTS = {
    "hanning": dict(window_type="hanning"),
    "hamming": dict(window_type="hamming"),
    "rectangular": dict(window_type="rectangular"),
    "blackman": dict(window_type="blackman"),
    "blackman-0.4": dict(window_type="blackman", blackman_coeff=0.4),
    "rho-0": dict(preemphasis_coefficient=0.0),
    "rho-1": dict(preemphasis_coefficient=1.0),
    "no-dc-removal": dict(remove_dc_offset=False, use_energy=True),
    "energy-first-floor": dict(use_energy=True, energy_floor=0.5),
    "energy-power": dict(use_energy=True, use_log_fbank=False),
    "subtract-mean": dict(subtract_mean=True),
    "subtract-mean-energy-power": dict(subtract_mean=True, use_energy=True, use_log_fbank=False, htk_compat=True),
    "band": dict(low_freq=300.0, high_freq=-400.0, num_mel_bins=23),
}


def test_every_window_and_option():
    f = 40
    clips = [(n, s) for n in ("48k", "22k") for s in _starts(n, P16, f)[1:6]]
    dec = tga._decoder()
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
    dec = tga._decoder()
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
    j_all = _j(name, p)
    counts = (1, 15, 16, 17, 31, 32, 33)
    dec = tga._decoder()
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
    dec = tga._decoder()
    try:
        sig = _signal(dec, clips, f, p)
        src = [(tga._streams()[n], tga._ref(n)[0], s) for n, s in clips]
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
    mix = tga._ref("mixed/mpeg1-lsf")[0]
    assert not mix.one_format
    s = tga._streams()
    good = [("48k", 100), ("22k", 3000)]
    dec = tga._decoder()
    try:
        sig = _signal(dec, good, f, p)
        for kind in ("device", "numpy"):
            for mid, exc, code in (((s["mixed/mpeg1-lsf"], mix, 0), api.MixedFormat, -3), ((bad, bix, 10), api.RingReplay, -2)):
                big, view = _destination(kind, 3, 1, f, d)
                src = [(s["48k"], tga._ref("48k")[0], 100), mid, (s["22k"], tga._ref("22k")[0], 3000)]
                with pytest.raises(exc) as e:
                    dec.decode_clips_fbank(src, f, out=view, **p)
                host = tga._host(big)
                assert e.value.valid[1] == code and (host[1] == SENT).all()
                assert (host[:, :, f * d:] == SENT).all()
                got = host[[0, 2], :, :f * d].reshape(2, 1, f, d)
                _check(good, sig, got, e.value.valid[[0, 2]], f, p)
        # bad arguments: nothing is written
        big, view = _destination("device", 1, 1, f, d)
        src = [(s["48k"], tga._ref("48k")[0], 0)]
        for bad_p in (dict(win_length=1), dict(win_length=1025), dict(win_length=401, round_to_power_of_two=False), dict(hop=0), dict(hop=401),
                      dict(high_freq=8000.5), dict(low_freq=-1.0), dict(preemphasis_coefficient=1.5), dict(window_type="kaiser"), dict(scale=0.0),
                      dict(energy_floor=-1.0), dict(width=65), dict(dither=1.0), dict(use_power=False), dict(raw_energy=False),
                      dict(snip_edges=False), dict(vtln_warp=1.1)):
            with pytest.raises(RuntimeError):
                dec.decode_clips_fbank(src, f, out=view, **dict(p, **bad_p))
        with pytest.raises(RuntimeError):
            dec.decode_clips_fbank([(s["48k"], tga._ref("48k")[0], -1)], f, out=view, **p)
        with pytest.raises(RuntimeError):            # (rate 0 and clips of different rates)
            dec.decode_clips_fbank(src + [(s["32k"], tga._ref("32k")[0], 0)], f, **dict(p, sample_rate=0))
        assert (tga._host(big) == SENT).all()
    finally:
        dec.close()
        bix.close()


def test_one_decoder_through_small_large_small_and_the_other_calls_after_it():
    import test_gpu_clip_mel as tgm
    p = dict(P16, subtract_mean=True, use_energy=True)
    small = [("32k", 500), ("8k", 1234)]
    large = [(n, s) for n in SIX for s in (0, 999, 20001)]
    fresh = tga._decoder()
    try:
        audio_before, av = tga._run(fresh, "device", [("48k", 700), ("22k", 9000)], 6000, 16000, 1)
        mel_before, mv = tgm._run(fresh, "device", [("48k", 700), ("22k", 9000)], 40, tgm.P16, "log10")
        ix = tga._ref("48k")[0]
        plain_before = fresh.decode_range(tga._streams()["48k"], ix, 33, 50).copy()
    finally:
        fresh.close()
    dec = tga._decoder()
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
        mel_after, mv2 = tgm._run(dec, "device", [("48k", 700), ("22k", 9000)], 40, tgm.P16, "log10")
        assert np.array_equal(mel_before.view(np.uint32), mel_after.view(np.uint32)) and np.array_equal(mv, mv2)
        audio_after, av2 = tga._run(dec, "device", [("48k", 700), ("22k", 9000)], 6000, 16000, 1)
        assert np.array_equal(audio_before.view(np.uint32), audio_after.view(np.uint32)) and np.array_equal(av, av2)
        plain_after = dec.decode_range(tga._streams()["48k"], tga._ref("48k")[0], 33, 50)
        assert np.array_equal(plain_before, plain_after)
    finally:
        dec.close()


def test_4099_clips_of_3_frames_in_one_call():
    p, f, k = dict(P16, use_energy=True), 3, 4099
    name = "mixed/mono-stereo"
    j_all = _j(name, p)
    ix = tga._ref(name)[0]
    rng = np.random.default_rng(4099)
    nw, hop = p["win_length"], p["hop"]
    starts = [0, 1, 199, 200, 201, j_all - nw - 2 * hop, j_all - nw - 2 * hop + 1, j_all - nw, j_all - nw + 1, j_all - 1, j_all, j_all + 999]
    starts += [int(x) for x in rng.integers(0, j_all + 400, k - len(starts))]
    clips = [(name, s) for s in starts]
    w = _filterbank(p, name)
    dec = tga._decoder()
    try:
        # the whole stream at 16 kHz, once: every clip's samples are slices of it (the audio call's rows are)
        whole = np.zeros((1, 1, j_all + 2048), dtype=np.float32)
        dec.decode_clips_audio([(tga._streams()[name], ix, 0)], j_all + 2048, 16000, 1, out=whole)
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
    dec = tga._decoder()
    try:
        # torchaudio's defaults: 25 ms frames every 10 ms, 23 bins
        out, valid = dec.decode_clips_fbank([(tga._streams()["32k"], tga._ref("32k")[0], 1000)], 50)
        assert tuple(out.shape) == (1, 1, 50, 23) and out.is_cuda and valid[0] == 50
        q = dict(P16, num_mel_bins=23)
        sig = _signal(dec, [("32k", 1000)], 50, q)
        _check([("32k", 1000)], sig, tga._host(out), valid, 50, q)
        out2, _ = dec.decode_clips_fbank([(tga._streams()["32k"], tga._ref("32k")[0], 1000)], 50, frame_length=25.0, frame_shift=10.0, **dict(q, win_length=None, hop=None))
        assert np.array_equal(tga._host(out).view(np.uint32), tga._host(out2).view(np.uint32))
        out, valid = dec.decode_clips_fbank([], 10)
        assert tuple(out.shape) == (0, 1, 10, 23) and valid.size == 0
        out, valid = dec.decode_clips_fbank([(tga._streams()["32k"], tga._ref("32k")[0], 1000)], 0)
        assert tuple(out.shape) == (1, 1, 0, 23) and valid[0] == 0
    finally:
        dec.close()
