"""Log-mel features of clips at n_fft 2048 and 4096 on the GPU (include/pdmp3_bulk.h pdmp3_amd_bulk_decode_clips_mel_long,
k_clip_mel_long).

The reference is made from the product's own signal, as in test_gpu_clip_mel.py: decode_clips_audio gives the binary32 samples
a clip's frames read, tests/clip_stft_ref.py and tests/clip_mel_ref.py evaluate the definition on them in binary64, and the
call's output has to agree within the bound derived in tests/clip_mel_long_ref.py -- every value of every mode, none left out;
the bound is 0 and the output exactly 0 on silence in mode 0.  Destinations are filled with a sentinel first.  Each device step
runs once; a clip's reference is computed once and shared by the modes.

Streams and helpers: tests/clip_gpu.py and tests/clip_gpu_calls.py."""
import math

import numpy as np
import pytest

import clip_audio_ref as aref
import clip_forms_cases as cases
import clip_gpu as cg
import clip_gpu_calls as calls
import clip_mel_long_ref as mlref
import clip_mel_ref as mref
import clip_streams
from clip_gpu import GUARD, SENT, signal as _signal
from clip_gpu_calls import MEL_LONG_PA as PA, mel_filterbank as _filterbank, mel_long_run as _run, mel_starts as _starts
from clip_streams import ISO_LSF

pytestmark = pytest.mark.gpu
MODES, U = mlref.MODES, mref.U

W1764 = (np.random.default_rng(1764).random(1764, dtype=np.float32) * np.float32(1.5) - np.float32(0.25)).astype(np.float32)
PB = dict(sample_rate=22050, n_fft=2048, hop=441, n_mels=128, scale="htk", norm=None, channels=1, win_length=1764, window=W1764)
PC = dict(sample_rate=0, n_fft=2048, hop=2048, n_mels=17, scale="slaney", norm="slaney", channels=1)
PD = dict(sample_rate=0, n_fft=4096, hop=1024, n_mels=128, scale="slaney", norm="slaney", channels=1)
PE = dict(sample_rate=0, n_fft=4096, hop=4096, n_mels=1, scale="slaney", norm="slaney", channels=2)
PF = dict(sample_rate=0, n_fft=2048, hop=1, n_mels=256, scale="slaney", norm="slaney", channels=1)


def _wants(clips, sig, f, p, floor=1e-10):
    """per clip {mode: (out, bound)}: the definition on the product's own signal, once for all modes"""
    return [mlref.mel_all(y, s0, s, f, p["n_fft"], p["hop"], _filterbank(p, n), floor, p.get("win_length"), p.get("window"))
            for (n, s), (s0, y) in zip(clips, sig)]


def _check(clips, sig, wants, got, valid, f, p, mode):
    """every row against the definition; -> worst error / bound over the rows that hold signal (a clip whose frames all lie
    in silence contributes none)"""
    worst = 0.0
    m = MODES.index(mode)
    for i, (n, s) in enumerate(clips):
        ix = cg.ref(n)[0]
        j_all = aref.out_length(ix.samples, ix.rate, cg.rate(p, n))
        assert int(valid[i]) == mref.valid(j_all, s, p["hop"], f), (n, s, valid[i])
        want, bound = wants[i][m]
        assert want.shape == got[i].shape
        err = np.abs(got[i].astype(np.float64) - want)
        assert (err <= bound).all(), "%s at %d, mode %s: error beyond the bound by %g at %s" % (
            n, s, mode, float((err - bound).max()), np.unravel_index(np.argmax(err - bound), err.shape))
        nz = wants[i][0][1] > 0                      # (mode 0's bound: where the frame holds signal and the band has a weight)
        if m == 0:
            assert (got[i][~nz] == 0.0).all() and (got[i] >= 0.0).all()
        if np.abs(sig[i][1]).sum() > 0 and nz.any():
            r = float((err[nz] / bound[nz]).max())
            assert 0.0 < r <= 1.0, (n, s, mode, r)
            worst = max(worst, r)
    return worst


CASES = {
    "a-48k-stereo-2048-hop-512-128-slaney": (PA, "48k", 21, "N2048-tile16"),        # one full tile and a partial one
    "b-22k-2048-hop-441-128-htk-own-window-1764": (PB, "22k", 19, "N2048-tile16"),
    "c-44k-mono-2048-hop-2048-17": (PC, "44k-mono", 11, "N2048-tile8"),
    "d-48k-4096-hop-1024-128": (PD, "48k", 11, "N4096-tile8"),
    "e-48k-stereo-4096-hop-4096-1": (PE, "48k", 5, "N4096-tile4"),
    "f-32k-2048-hop-1-256": (PF, "32k", 19, "N2048-tile16"),
}
RATES = {"48k": 48000, "22k": 22050, "44k-mono": 44100, "32k": 32000}


def test_the_cases_cover_every_launch_path():
    assert set(path for _, _, _, path in CASES.values()) == set(mlref.PATHS)
    for case, (p, name, f, path) in CASES.items():
        tile = mlref.plan(p["n_fft"], p["hop"], p["n_mels"])
        assert tile[3] == path and tile[0] < f < 2 * tile[0], case          # one full tile plus a partial one
        if case[0] in "abd":                                                 # every band of the music front ends has a weight
            w = mref.filterbank(p["sample_rate"] or RATES[name], p["n_fft"], p["n_mels"], 0.0, 0.0, p["scale"], p["norm"])
            assert (w > 0).any(axis=1).all(), case


@pytest.mark.parametrize("case", sorted(CASES))
def test_against_binary64_on_the_products_own_signal(case):
    from pdmp3_amd import api
    p, name, f, path = CASES[case]
    assert cg.rate(p, name) == RATES[name]
    clips = [(name, s) for s in _starts(name, p, f)]
    tile = api.mel_long_plan(p["n_fft"], p["hop"], p["n_mels"])[0]
    assert mlref.plan(p["n_fft"], p["hop"], p["n_mels"])[3] == path and path.endswith("tile%d" % tile)
    dec = cg.decoder()
    try:
        sig = _signal(dec, clips, f, p)
        wants = _wants(clips, sig, f, p)
        for mode in MODES:
            for kind in ("device", "numpy") if mode in ("power", "log10") else ("device",):
                got, valid = _run(dec, kind, clips, f, p, mode)
                worst = _check(clips, sig, wants, got, valid, f, p, mode)
                print("%s (tile %d, %s), mode %s, %s: worst error / bound %.4f over %d clips of %d frames"
                      % (case, tile, path, mode, kind, worst, len(clips), f))
                assert 0.0 < worst <= 1.0
    finally:
        dec.close()


@pytest.mark.parametrize("p", [PA, PD], ids=["2048-hop-512", "4096-hop-1024"])
def test_frames_are_frames(p):
    """frame f of a clip at `start` is frame 0 of the clip at start + f H, bit for bit, on both sides of both tile edges"""
    from pdmp3_amd import api
    name, start = "48k", 4321
    assert start % p["hop"] != 0
    tile = api.mel_long_plan(p["n_fft"], p["hop"], p["n_mels"])[0]
    fs = [0, 1, tile - 1, tile, tile + 1, 2 * tile - 1, 2 * tile, 2 * tile + 2]
    f_long = 2 * tile + 4
    dec = cg.decoder()
    try:
        for mode in MODES:
            long, _ = _run(dec, "device", [(name, start)], f_long, p, mode)
            short, _ = _run(dec, "device", [(name, start + f * p["hop"]) for f in fs], 2, p, mode)
            for i, f in enumerate(fs):
                assert np.array_equal(long[0, :, :, f].view(np.uint32), short[i, :, :, 0].view(np.uint32)), (mode, f)
                assert np.array_equal(long[0, :, :, f + 1].view(np.uint32), short[i, :, :, 1].view(np.uint32)), (mode, f)
            assert np.abs(long).sum() > 0
    finally:
        dec.close()


@pytest.mark.parametrize("p,f", [(PA, 19), (PD, 10)], ids=["2048-hop-512", "4096-hop-1024"])
def test_mode_0_is_the_filterbank_of_the_spectrum_calls_powers(p, f):
    """W times decode_clips_stft_long(mode="power") of the same clips, evaluated in binary64, against this call's mode 0: the
    powers are the same chains in both kernels, so what remains is the filterbank's own rounding, (K_m + 2) u W P -- the
    second part of dM alone"""
    name = "48k"
    clips = [(name, s) for s in (0, 57, 30011)]
    src = cg.src(clips)
    dec = cg.decoder()
    try:
        got, valid = _run(dec, "device", clips, f, p, "power")
        power, v2 = dec.decode_clips_stft_long(src, f, sample_rate=0, n_fft=p["n_fft"], hop=p["hop"], channels=p["channels"], mode="power")
        assert np.array_equal(valid, v2)
        pw = cg.host(power).astype(np.float64)                             # [k, c, K, f]
        want, bound = mlref.gemm_bound(_filterbank(p, name), pw)
        err = np.abs(got.astype(np.float64) - want)
        assert want.shape == got.shape and (err <= bound).all(), float((err - bound).max())
        r = float((err[bound > 0] / bound[bound > 0]).max())
        print("N %d: worst |mode 0 - W P| / ((K_m + 2) u W P) = %.4f" % (p["n_fft"], r))
        assert 0.0 < r <= 1.0
    finally:
        dec.close()


def test_slices_of_a_batch_are_the_batchs_slices():
    p, f = dict(PB, sample_rate=16000), 19
    clips = [(n, s) for n in ("48k", "22k", "16k-mono") for s in (0, 5000, 23457)]
    dec = cg.decoder()
    try:
        for mode in ("power", "log10"):
            whole, valid = _run(dec, "device", clips, f, p, mode)
            for a, b in ((0, 1), (2, 5), (4, 9), (8, 9)):
                part, v = _run(dec, "device", clips[a:b], f, p, mode)
                assert np.array_equal(part.view(np.uint32), whole[a:b].view(np.uint32)) and np.array_equal(v, valid[a:b]), (mode, a, b)
            assert np.abs(whole).sum() > 0
    finally:
        dec.close()


def test_a_refused_clip_in_the_middle_of_a_batch_and_bad_arguments():
    from pdmp3_amd import api
    p, f = dict(PA, sample_rate=16000, channels=1), 9
    nm = p["n_mels"]
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
        wants = _wants(good, sig, f, p)
        for kind, mode in (("device", "power"), ("numpy", "log10")):
            per = nm * f
            for mid, exc, code in (((s["mixed/mpeg1-lsf"], mix, 0), api.MixedFormat, -3), ((bad, bix, 10), api.RingReplay, -2)):
                big, view = cg.destination(kind, 3, 1, (nm, f))
                src = [(s["48k"], cg.ref("48k")[0], 100), mid, (s["22k"], cg.ref("22k")[0], 3000)]
                with pytest.raises(exc) as e:
                    dec.decode_clips_mel_long(src, f, mode=mode, out=view, **p)
                host = cg.host(big).reshape(3, 1, per + GUARD)
                assert e.value.valid[1] == code and (host[1] == SENT).all()
                assert (host[:, :, per:] == SENT).all()
                got = host[[0, 2], :, :per].reshape(2, 1, nm, f)
                _check(good, sig, wants, got, e.value.valid[[0, 2]], f, p, mode)
        # bad arguments: nothing is written
        big, view = cg.destination("device", 1, 1, (nm, f))
        src = [(s["48k"], cg.ref("48k")[0], 0)]
        nan_window = np.ones(2048, dtype=np.float32)
        nan_window[123] = np.nan
        for bad_p in (dict(n_fft=1024), dict(n_fft=8192), dict(n_fft=400), dict(hop=0), dict(hop=2049), dict(win_length=2049), dict(window=nan_window),
                      dict(floor=0.0), dict(width=65), dict(mode="whisper"), dict(mode=4), dict(f_max=8001.0), dict(f_min=3000.0, f_max=3000.0)):
            q = dict(dict(p, mode="log10"), **bad_p)
            with pytest.raises(RuntimeError):
                dec.decode_clips_mel_long(src, f, out=view, **q)
            assert (cg.host(big) == SENT).all()
        with pytest.raises(RuntimeError):
            dec.decode_clips_mel_long([(s["48k"], cg.ref("48k")[0], -1)], f, out=view, **p)
        with pytest.raises(RuntimeError):            # (rate 0 and clips of different rates)
            dec.decode_clips_mel_long(src + [(s["32k"], cg.ref("32k")[0], 0)], f, **dict(p, sample_rate=0))
        assert (cg.host(big) == SENT).all()
        # the call of section 10 keeps refusing this length
        with pytest.raises(RuntimeError):
            dec.decode_clips_mel(src, f, mode="log10", out=view, **p)
        assert (cg.host(big) == SENT).all()
    finally:
        dec.close()
        bix.close()


def test_clips_wholly_behind_the_end_return_types_and_empty_calls():
    import torch
    p, f, floor = PA, 5, 1e-7
    name = "48k"
    ix = cg.ref(name)[0]
    j_all = aref.out_length(ix.samples, ix.rate, ix.rate)
    clips = [(name, j_all + 5 * p["n_fft"]), (name, j_all + 1000000)]
    src = cg.src(clips)
    dec = cg.decoder()
    try:
        got, valid = _run(dec, "device", clips, f, p, "power", floor)
        assert (valid == 0).all() and (got.view(np.uint32) == 0).all()        # exactly +0.0
        for mode, base in (("log", math.e), ("log10", 10.0)):
            got, valid = _run(dec, "device", clips, f, p, mode, floor)
            want = math.log(float(np.float32(floor))) / math.log(base)
            assert (valid == 0).all() and (np.abs(got.astype(np.float64) - want) <= mref.LOG_C * U * max(1.0, abs(want))).all()
        out, valid = dec.decode_clips_mel_long(src, f, sample_rate=0, channels=2)
        assert tuple(out.shape) == (2, 2, 128, f) and out.is_cuda and out.dtype == torch.float32 and (valid == 0).all()
        out, valid = dec.decode_clips_mel_long([], 10)
        assert tuple(out.shape) == (0, 1, 128, 10) and valid.size == 0
        out, valid = dec.decode_clips_mel_long(src, 0, sample_rate=0, n_fft=4096, n_mels=17)
        assert tuple(out.shape) == (2, 1, 17, 0) and (valid == 0).all()
    finally:
        dec.close()


def test_more_clips_than_one_grid():
    """32 768 + 5 clips of one frame at (2048, 2048, 1) in one call: pdmp3_hip_clip_mel_long launches the kernel twice (a
    grid's y extent), the second time from descriptor 32 768 on.  Sixty-four distinct clips are held against the definition,
    every row is bit-equal to its twin among them; the last five are other clips than rows 0 .. 4, one of them behind the end"""
    name, k = "32k", 32768 + 5
    p = dict(sample_rate=0, n_fft=2048, hop=2048, n_mels=1, scale="slaney", norm="slaney", channels=1)
    ix = cg.ref(name)[0]
    j_all = aref.out_length(ix.samples, ix.rate, ix.rate)
    starts = [1000 + 3001 * i for i in range(62)] + [j_all + 7, j_all - 1]
    assert starts[61] + 2048 < j_all
    twin = (np.arange(k, dtype=np.int64) * 7) % 62
    twin[32768:] = [62, 63, 61, 60, 59]
    assert not np.any(twin[32768:] == twin[:5])
    mp3 = cg.streams()[name]
    dec = cg.decoder()
    try:
        first = [(name, s) for s in starts]
        sig = _signal(dec, first, 1, p)
        wants = _wants(first, sig, 1, p)
        base, valid64 = _run(dec, "device", first, 1, p, "log10")
        assert 0.0 < _check(first, sig, wants, base, valid64, 1, p, "log10") <= 1.0
        assert list(valid64[61:]) == [1, 0, 1]
        big, view = cg.destination("device", k, 1, (1, 1))
        out, valid = dec.decode_clips_mel_long([(mp3, ix, int(starts[t])) for t in twin], 1, mode="log10", out=view, **p)
        host = cg.host(big)
        assert (host[:, :, 1:] == SENT).all(), "written behind a row's floats"
        assert np.array_equal(valid, valid64[twin]) and list(valid[32768:]) == [0, 1, 1, 1, 1]
        bad = np.flatnonzero(host[:, 0, 0].view(np.uint32) != base[twin, 0, 0, 0].view(np.uint32))
        assert bad.size == 0, "%d rows differ from their twins, %d of them in the second launch: %s" % (bad.size, int((bad >= 32768).sum()), bad[:8].tolist())
        assert np.unique(base[:62, 0, 0, 0]).size > 32
    finally:
        dec.close()


def test_one_decoder_through_this_call_the_other_calls_and_this_call_again():
    """the new call, decode_clips_stft_long, decode_clips_mel, decode_clips_audio, decode_range, the new call with another
    filterbank and with the other n_fft -- and all of it again: every call is bit-equal to its first answer, the filterbank
    operands live side by side and the transform's tables are shared with the spectrum call"""
    small = [("32k", 500), ("8k", 1234)]
    pa = dict(PA, sample_rate=16000, channels=1)
    pb = dict(pa, n_mels=40, scale="htk", norm=None, f_min=50.0, f_max=7000.0)
    pd = dict(PD, sample_rate=16000, n_mels=17)
    dec = cg.decoder()
    try:
        def once():
            r = [_run(dec, "device", small, 9, pa, "log10"),
                 calls.stft_long_run(dec, "device", small, 9, dict(calls.STFT_LONG_PA, sample_rate=16000, channels=1), "complex"),
                 calls.mel_run(dec, "device", small, 9, cases.MEL_P16, "log10"),
                 calls.audio_run(dec, "device", [("48k", 700), ("22k", 9000)], 6000, 16000, 1),
                 (dec.decode_range(cg.streams()["48k"], cg.ref("48k")[0], 33, 50).copy(), np.zeros(0)),
                 _run(dec, "device", small, 9, pb, "log10"),
                 _run(dec, "numpy", small, 5, pd, "power")]
            return r
        a, b = once(), once()
        for i, ((x, vx), (y, vy)) in enumerate(zip(a, b)):
            assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)) and np.array_equal(vx, vy), i
            assert np.abs(x.astype(np.float64)).sum() > 0, i
        assert a[0][0].shape != a[5][0].shape
        sig = _signal(dec, small, 9, pb)
        print("the second filterbank: worst error / bound %.4f" % _check(small, sig, _wants(small, sig, 9, pb), a[5][0], a[5][1], 9, pb, "log10"))
    finally:
        dec.close()
