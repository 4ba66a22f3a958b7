"""The short-time Fourier transform of clips at n_fft 2048 and 4096 on the GPU (include/pdmp3_bulk.h
pdmp3_amd_bulk_decode_clips_stft_long, k_clip_stft_long).

The reference is made from the product's own signal, as in test_gpu_clip_stft.py: decode_clips_audio gives the binary32 samples
a clip's frames read, tests/clip_stft_ref.py evaluates the definition on them in binary64, and the call's output has to agree
within the two-stage bound derived in tests/clip_stft_long_ref.py -- every value of every mode, none left out; the bound is 0
and the output exactly 0 on silence in modes 0 - 2.  Destinations are filled with a sentinel first.  Each device step runs
once; a clip's reference is computed once and shared by the modes.

Streams and helpers: tests/clip_gpu.py and tests/clip_gpu_calls.py."""
import numpy as np
import pytest

import clip_forms_cases as cases
import clip_gpu as cg
import clip_gpu_calls as calls
import clip_stft_long_ref as lref
import clip_stft_ref as ref
import clip_streams
from clip_gpu import GUARD, SENT, signal as _signal
from clip_gpu_calls import STFT_LONG_PA as PA, STFT_MODES as MODES, mel_starts as _starts, stft_long_check as _check, stft_long_run as _run, stft_long_wants as _wants, stft_per as _per
from clip_streams import ISO_LSF

pytestmark = pytest.mark.gpu

W1764 = (np.random.default_rng(1764).random(1764, dtype=np.float32) * np.float32(1.5) - np.float32(0.25)).astype(np.float32)
PB = dict(sample_rate=22050, n_fft=2048, hop=441, channels=1, win_length=1764, window=W1764, normalized=True)
PC = dict(sample_rate=0, n_fft=2048, hop=2048, channels=1)                 # the reduced tile
PD = dict(sample_rate=0, n_fft=4096, hop=1024, channels=1)
PE = dict(sample_rate=0, n_fft=4096, hop=4096, channels=1)
PF = dict(sample_rate=0, n_fft=2048, hop=1, channels=1)
W1920 = (np.random.default_rng(1920).random(1920, dtype=np.float32) * np.float32(1.5) - np.float32(0.25)).astype(np.float32)
PG = dict(sample_rate=0, n_fft=4096, hop=1024, channels=2, win_length=1920, window=W1920, normalized=True)
PH = dict(sample_rate=0, n_fft=4096, hop=4096, channels=2)
CASES = {
    "a-48k-stereo-2048-hop-512": (PA, "48k", 21, "N2048-tile16"),       # one full tile and a partial one
    "b-22k-2048-hop-441-own-window": (PB, "22k", 19, "N2048-tile16"),
    "c-44k-mono-2048-hop-2048": (PC, "44k-mono", 11, "N2048-tile8"),
    "d-48k-4096-hop-1024": (PD, "48k", 18, "N4096-tile8"),
    "e-48k-4096-hop-4096": (PE, "48k", 5, "N4096-tile4"),
    "f-32k-2048-hop-1": (PF, "32k", 40, "N2048-tile16"),
    "g-48k-stereo-4096-hop-1024-own-window-1920": (PG, "48k", 11, "N4096-tile8"),      # 4096: stereo, win_length, a caller's window, normalized
    "h-48k-stereo-4096-hop-4096": (PH, "48k", 7, "N4096-tile4"),
}


def test_the_cases_cover_every_launch_path():
    assert set(path for _, _, _, path in CASES.values()) == set(lref.PATHS)


@pytest.mark.parametrize("case", sorted(CASES))
def test_against_binary64_on_the_products_own_signal(case):
    from pdmp3_amd import api
    p, name, f, path = CASES[case]
    clips = [(name, s) for s in _starts(name, p, f)]
    dec = cg.decoder()
    try:
        sig = _signal(dec, clips, f, p)
        wants = _wants(clips, sig, f, p)
        for mode in MODES:
            tile = api.stft_long_plan(p["n_fft"], p["hop"], mode)[0]
            assert lref.plan(p["n_fft"], p["hop"], MODES.index(mode))[3] == path
            for kind in ("device", "numpy") if mode in ("complex", "log10") else ("device",):
                got, valid = _run(dec, kind, clips, f, p, mode)
                worst = _check(clips, sig, wants, got, valid, f, p, mode)
                print("%s (tile %d, %s), mode %s, %s: worst error / bound %.4f over %d clips of %d frames"
                      % (case, tile, path, mode, kind, worst, len(clips), f))
                assert 0.0 < worst <= 1.0
    finally:
        dec.close()


@pytest.mark.parametrize("p", [PA, PD], ids=["2048-hop-512", "4096-hop-1024"])
def test_frames_are_frames_and_mode_0_rederives_the_others_bit_for_bit(p):
    """frame f of a clip at `start` is frame 0 of the clip at start + f H, bit for bit, on both sides of the kernel's tile
    edges; Re^2 + Im^2 through the product's own arithmetic on mode 0's output is mode 2's, its correctly rounded square root
    mode 1's, bit for bit: a transposed frame, a swapped bin or a mixed pair would show"""
    from pdmp3_amd import api
    name, start = "48k", 4321
    assert start % p["hop"] != 0
    tile = api.stft_long_plan(p["n_fft"], p["hop"], "complex")[0]
    fs = [0, 1, tile - 1, tile, tile + 1, 2 * tile - 1, 2 * tile, 2 * tile + 2]
    f_long = 2 * tile + 4
    dec = cg.decoder()
    try:
        outs = {}
        for mode in MODES[:3]:
            long, _ = _run(dec, "device", [(name, start)], f_long, p, mode)
            short, _ = _run(dec, "device", [(name, start + f * p["hop"]) for f in fs], 2, p, mode)
            for i, f in enumerate(fs):
                assert np.array_equal(long[0, :, :, f].view(np.uint32), short[i, :, :, 0].view(np.uint32)), (mode, f)
                assert np.array_equal(long[0, :, :, f + 1].view(np.uint32), short[i, :, :, 1].view(np.uint32)), (mode, f)
            assert np.abs(long).sum() > 0
            outs[mode] = long
        z = outs["complex"]
        want = ref.power_as_the_product(z[..., 0], z[..., 1])
        assert np.array_equal(want.view(np.uint32), outs["power"].view(np.uint32))
        assert np.array_equal(np.sqrt(want).view(np.uint32), outs["magnitude"].view(np.uint32))
        assert np.abs(z[..., 1]).sum() > 0 and not np.array_equal(z[..., 0], z[..., 1])
    finally:
        dec.close()


def test_slices_of_a_batch_are_the_batchs_slices():
    p, f = dict(PB, sample_rate=16000), 19
    clips = [(n, s) for n in ("48k", "22k", "16k-mono") for s in (0, 5000, 23457)]
    dec = cg.decoder()
    try:
        for mode in ("complex", "log10"):
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
    nb = p["n_fft"] // 2 + 1
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
        for kind, mode in (("device", "complex"), ("numpy", "log10")):
            per = _per(p, mode) * f
            for mid, exc, code in (((s["mixed/mpeg1-lsf"], mix, 0), api.MixedFormat, -3), ((bad, bix, 10), api.RingReplay, -2)):
                big, view = cg.destination(kind, 3, 1, calls.stft_inner(nb, f, mode))
                src = [(s["48k"], cg.ref("48k")[0], 100), mid, (s["22k"], cg.ref("22k")[0], 3000)]
                with pytest.raises(exc) as e:
                    dec.decode_clips_stft_long(src, f, mode=mode, out=view, **p)
                host = cg.host(big).reshape(3, 1, per + GUARD)
                assert e.value.valid[1] == code and (host[1] == SENT).all()
                assert (host[:, :, per:] == SENT).all()
                got = host[[0, 2], :, :per].reshape((2, 1, nb, f, 2) if mode == "complex" else (2, 1, nb, f))
                _check(good, sig, wants, got, e.value.valid[[0, 2]], f, p, mode)
        # bad arguments: nothing is written
        big, view = cg.destination("device", 1, 1, calls.stft_inner(nb, f, "log10"))
        src = [(s["48k"], cg.ref("48k")[0], 0)]
        nan_window = np.ones(2048, dtype=np.float32)
        nan_window[123] = np.nan
        for bad_p in (dict(n_fft=1024), dict(n_fft=8192), dict(n_fft=400), dict(hop=0), dict(hop=2049), dict(win_length=2049), dict(window=nan_window),
                      dict(floor=0.0), dict(width=65)):
            q = dict(p, **bad_p)
            bb, bv = (big, view) if q["n_fft"] == 2048 else cg.destination("device", 1, 1, calls.stft_inner(q["n_fft"] // 2 + 1, f, "log10"))
            with pytest.raises(RuntimeError):
                dec.decode_clips_stft_long(src, f, mode="log10", out=bv, **q)
            assert (cg.host(bb) == SENT).all()
        with pytest.raises(RuntimeError):
            dec.decode_clips_stft_long([(s["48k"], cg.ref("48k")[0], -1)], f, mode="log10", out=view, **p)
        with pytest.raises(RuntimeError):            # (rate 0 and clips of different rates)
            dec.decode_clips_stft_long(src + [(s["32k"], cg.ref("32k")[0], 0)], f, **dict(p, sample_rate=0))
        assert (cg.host(big) == SENT).all()
        # the call of section 13 keeps refusing this length
        with pytest.raises(RuntimeError):
            dec.decode_clips_stft(src, f, mode="log10", out=view, **p)
        assert (cg.host(big) == SENT).all()
    finally:
        dec.close()
        bix.close()


def test_an_odd_float_destination_return_types_and_empty_calls():
    import torch
    p, f = PD, 10
    clips = [("48k", 1000)]
    src = [(cg.streams()["48k"], cg.ref("48k")[0], 1000)]
    dec = cg.decoder()
    try:
        plain, _ = _run(dec, "device", clips, f, p, "complex")
        # a row at an odd float: the pairs' 8-byte stores are 4-byte aligned there, the values the same
        odd, _ = _run(dec, "device", clips, f, p, "complex", offset=1)
        assert np.array_equal(odd.view(np.uint32), plain.view(np.uint32)) and np.abs(plain).sum() > 0
        out, valid = dec.decode_clips_stft_long(src, f, **p)
        assert tuple(out.shape) == (1, 1, 2049, f) and out.is_cuda and out.dtype == torch.complex64 and valid[0] == f
        assert np.array_equal(cg.host(torch.view_as_real(out)).view(np.uint32), plain.view(np.uint32))
        out, valid = dec.decode_clips_stft_long(src, f, mode="magnitude", channels=2)
        assert tuple(out.shape) == (1, 2, 1025, f) and out.dtype == torch.float32
        out, valid = dec.decode_clips_stft_long([], 10)
        assert tuple(out.shape) == (0, 1, 1025, 10) and out.dtype == torch.complex64 and valid.size == 0
        out, valid = dec.decode_clips_stft_long(src, 0, mode="power", n_fft=4096)
        assert tuple(out.shape) == (1, 1, 2049, 0) and out.dtype == torch.float32 and valid[0] == 0
    finally:
        dec.close()


def test_one_decoder_through_the_long_call_the_other_calls_and_the_long_call_again():
    """the long call, then decode_clips_stft, decode_clips_mel, decode_clips_audio and decode_range, then the long call with
    another window and the first again: every call is bit-equal to its first answer (on a fresh decoder), both n_fft's tables
    live side by side and the window is taken anew on every call"""
    rng = np.random.default_rng(14)
    wa = rng.random(2048, dtype=np.float32)
    wb = rng.random(2048, dtype=np.float32)
    pa, pb = dict(PA, channels=1, window=wa), dict(PA, channels=1, window=wb)
    small = [("32k", 500), ("8k", 1234)]
    p16 = dict(pa, sample_rate=16000)
    p16b = dict(pb, sample_rate=16000)
    fresh = cg.decoder()
    try:
        stft_before, sv = calls.stft_run(fresh, "device", small, 9, cases.STFT_P16, "complex")
        mel_before, mv = calls.mel_run(fresh, "device", small, 9, cases.MEL_P16, "log10")
        audio_before, av = calls.audio_run(fresh, "device", [("48k", 700), ("22k", 9000)], 6000, 16000, 1)
        plain_before = fresh.decode_range(cg.streams()["48k"], cg.ref("48k")[0], 33, 50).copy()
    finally:
        fresh.close()
    dec = cg.decoder()
    try:
        a, va = _run(dec, "device", small, 9, p16, "complex")
        stft_after, sv2 = calls.stft_run(dec, "device", small, 9, cases.STFT_P16, "complex")
        assert np.array_equal(stft_before.view(np.uint32), stft_after.view(np.uint32)) and np.array_equal(sv, sv2)
        mel_after, mv2 = calls.mel_run(dec, "device", small, 9, cases.MEL_P16, "log10")
        assert np.array_equal(mel_before.view(np.uint32), mel_after.view(np.uint32)) and np.array_equal(mv, mv2)
        audio_after, av2 = calls.audio_run(dec, "device", [("48k", 700), ("22k", 9000)], 6000, 16000, 1)
        assert np.array_equal(audio_before.view(np.uint32), audio_after.view(np.uint32)) and np.array_equal(av, av2)
        plain_after = dec.decode_range(cg.streams()["48k"], cg.ref("48k")[0], 33, 50)
        assert np.array_equal(plain_before, plain_after)
        b, vb = _run(dec, "device", small, 9, p16b, "complex")
        assert not np.array_equal(a, b) and np.array_equal(va, vb)
        d4, _ = _run(dec, "device", small, 5, dict(PD, sample_rate=16000), "power")          # (the other n_fft's tables)
        a2, _ = _run(dec, "numpy", small, 9, p16, "complex")
        assert np.array_equal(a.view(np.uint32), a2.view(np.uint32))
        b2, _ = _run(dec, "device", small, 9, p16b, "complex")
        assert np.array_equal(b.view(np.uint32), b2.view(np.uint32))
        d4b, _ = _run(dec, "device", small, 5, dict(PD, sample_rate=16000), "power")
        assert np.array_equal(d4.view(np.uint32), d4b.view(np.uint32)) and np.abs(d4).sum() > 0
        # the window's values hold against the definition (the second window is not the first one's table)
        sig = _signal(dec, small, 9, p16b)
        print("the second window: worst error / bound %.4f" % _check(small, sig, _wants(small, sig, 9, p16b), b, vb, 9, p16b, "complex"))
    finally:
        dec.close()
