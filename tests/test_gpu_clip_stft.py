"""The short-time Fourier transform of clips on the GPU (include/pdmp3_bulk.h pdmp3_amd_bulk_decode_clips_stft, k_clip_stft;
DESIGN.md section 13).

The reference is made from the product's own signal: for every clip decode_clips_audio gives the binary32 samples its frames
read (the span from max(0, start - N / 2) on), tests/clip_stft_ref.py evaluates the definition on them in binary64, and the
call's output has to agree within the binary32 bound derived there -- every value of every mode, none left out; the bound is 0
and the output exactly 0 on silence in modes 0 - 2.  Destinations are filled with a sentinel first: nothing outside a row's
floats may change.  Each device step runs once.

Streams and helpers: tests/clip_gpu.py and tests/clip_gpu_calls.py."""
import ctypes as C
import math

import numpy as np
import pytest

import clip_audio_ref as aref
import clip_forms_cases as cases
import clip_gpu as cg
import clip_gpu_calls as calls
import clip_stft_ref as ref
import clip_streams
from clip_forms_cases import STFT_CASES as CASES, STFT_P16 as P16, STFT_P24 as P24, STFT_P48 as P48, STFT_P48H as P48H
from clip_gpu import GUARD, SENT, signal as _signal
from clip_gpu_calls import STFT_MODES as MODES, mel_starts as _starts, stft_check as _check, stft_per as _per, stft_run as _run
from clip_streams import ISO_LSF

pytestmark = pytest.mark.gpu
U = ref.U
PATHS = {"16k-mono-batch": "tile32", "24k-stereo-own-window": "tile32", "own-rate-1024": "tile16-static", "own-rate-1024-hop-512": "tile16",
         "n16-hop1": "tile32"}


@pytest.mark.parametrize("case", sorted(CASES))
def test_against_binary64_on_the_products_own_signal(case):
    from pdmp3_amd import api
    p, names, f = CASES[case]
    if case == "16k-mono-batch":
        assert set(cg.ref(n)[0].rate for n in names) == {44100, 48000, 32000, 22050, 16000, 8000}
    clips = [(n, s) for n in names for s in _starts(n, p, f)]
    dec = cg.decoder()
    try:
        sig = _signal(dec, clips, f, p)
        for mode in MODES:
            tile = api.stft_tile(p["n_fft"], p["hop"], mode)[0]
            assert ref.tile_plan(p["n_fft"], p["hop"], MODES.index(mode))[3] == PATHS[case]
            for kind in ("device", "numpy") if mode in ("complex", "log10") else ("device",):
                got, valid = _run(dec, kind, clips, f, p, mode)
                worst = _check(clips, sig, got, valid, f, p, mode)
                print("%s (tile %d, %s), mode %s, %s: worst error / bound %.4f over %d clips of %d frames"
                      % (case, tile, PATHS[case], mode, kind, worst, len(clips), f))
                assert 0.0 < worst <= 1.0
    finally:
        dec.close()


@pytest.mark.parametrize("p", [P16, P24, P48H], ids=["16k", "24k-stereo-own-window", "1024-hop-512"])
def test_mode_0_rederives_the_others_bit_for_bit(p):
    """Re^2 + Im^2 through the product's own arithmetic on mode 0's output is mode 2's, its correctly rounded square root
    mode 1's, bit for bit: a transposed frame, a swapped bin or a mixed pair would show"""
    f = 37
    clips = [("48k", 4321), ("22k", 0)] if p["sample_rate"] else [("48k", 4321)]
    dec = cg.decoder()
    try:
        z, _ = _run(dec, "device", clips, f, p, "complex")
        power, _ = _run(dec, "device", clips, f, p, "power")
        mag, _ = _run(dec, "device", clips, f, p, "magnitude")
        want = ref.power_as_the_product(z[..., 0], z[..., 1])
        assert np.array_equal(want.view(np.uint32), power.view(np.uint32))
        assert np.array_equal(np.sqrt(want).view(np.uint32), mag.view(np.uint32))
        assert np.abs(z[..., 1]).sum() > 0 and not np.array_equal(z[..., 0], z[..., 1])
    finally:
        dec.close()


@pytest.mark.parametrize("p", [P16, P24], ids=["16k", "24k-stereo-own-window"])
def test_slices_are_slices(p):
    """frame f of a clip at `start` is frame 0 of a clip at start + f H, bit for bit, on both sides of the kernel's tile edges"""
    from pdmp3_amd import api
    name, start = "48k", 4321
    assert start % p["hop"] != 0
    dec = cg.decoder()
    try:
        for mode in MODES[:3]:
            tile = api.stft_tile(p["n_fft"], p["hop"], mode)[0]
            fs = [0, 1, tile - 1, tile, tile + 1, 2 * tile - 1, 2 * tile, 2 * tile + 1, 2 * tile + 5]
            f_long = 2 * tile + 7
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
    tile = api.stft_tile(p["n_fft"], p["hop"], "complex")[0]
    assert tile == api.stft_tile(p["n_fft"], p["hop"], "log10")[0]
    name = "32k"
    ix = cg.ref(name)[0]
    j_all = aref.out_length(ix.samples, ix.rate, 16000)
    nb = p["n_fft"] // 2 + 1
    dec = cg.decoder()
    try:
        for f in (1, tile - 1, tile, tile + 1):
            clips = [(name, 777), (name, 0)]
            sig = _signal(dec, clips, f, p)
            for mode in ("complex", "log10"):
                got, valid = _run(dec, "device", clips, f, p, mode)
                assert list(valid) == [f, f]
                print("F = %d, mode %s: worst error / bound %.4f" % (f, mode, _check(clips, sig, got, valid, f, p, mode)))
        f = tile + 2
        clips = [(name, j_all - (v - 1) * p["hop"] - 1) for v in (1, tile - 1, tile, tile + 1)]
        sig = _signal(dec, clips, f, p)
        for mode in ("complex", "magnitude", "log10"):
            got, valid = _run(dec, "device", clips, f, p, mode)
            assert list(valid) == [1, tile - 1, tile, tile + 1]
            print("valid at the tile's edges, mode %s: worst error / bound %.4f" % (mode, _check(clips, sig, got, valid, f, p, mode)))
        # wholly behind the end: the transform of zeros
        stats = dec.clip_stats()
        clips = [(name, j_all + p["n_fft"] // 2), (name, j_all + 10 ** 6), (name, 2 ** 40)]
        for mode, floor in (("complex", 1e-10), ("magnitude", 1e-10), ("power", 0.0), ("log", 1e-10), ("log10", 1e-10), ("log10", 3e-5)):
            got, valid = _run(dec, "device", clips, f, p, mode, floor)
            assert list(valid) == [0, 0, 0]
            if mode in ("complex", "magnitude", "power"):
                assert (got == 0.0).all()
                continue
            fl = float(np.float32(floor))
            want = math.log(fl) if mode == "log" else math.log10(fl)
            w64, bound = ref.stft(np.zeros((1, 8)), 0, 10 ** 6, f, p["n_fft"], p["hop"], MODES.index(mode), floor)
            assert w64.shape == (1, nb, f) and np.allclose(w64, want, rtol=1e-15, atol=0)
            assert np.allclose(bound, ref.LOG_C * U * abs(want), rtol=1e-12, atol=0)       # (the logarithm's own c u |out| alone)
            assert (np.abs(got.astype(np.float64) - w64[None]) <= bound[None]).all(), (mode, floor)
        assert dec.clip_stats() == stats
    finally:
        dec.close()


def test_host_destinations():
    """a dense numpy array (its rows leave the stage in one copy), strided stereo rows and pinned host memory: bit-equal"""
    import pdmp3_amd
    from pdmp3_amd import api
    p, f = P16, 37
    clips = [(n, s) for n in ("48k", "22k", "16k-mono") for s in _starts(n, p, f)[1:4]]
    k, nb = len(clips), p["n_fft"] // 2 + 1
    dec = cg.decoder()
    try:
        sig = _signal(dec, clips, f, p)
        src = cg.src(clips)
        for mode in ("complex", "log10"):
            per = _per(p, mode) * f
            shape = (k, 1, nb, f, 2) if mode == "complex" else (k, 1, nb, f)
            flat = np.full(k * per + GUARD, SENT, dtype=np.float32)
            dense = flat[:k * per].reshape(shape)
            out, valid = dec.decode_clips_stft(src, f, mode=mode, out=dense, **p)
            assert out is dense and (flat[k * per:] == SENT).all()
            print("dense numpy rows, mode %s: worst error / bound %.4f" % (mode, _check(clips, sig, dense, valid, f, p, mode)))
            strided, valid1 = _run(dec, "numpy", clips, f, p, mode)
            assert np.array_equal(strided.view(np.uint32), dense.view(np.uint32)) and np.array_equal(valid, valid1)
            pin = api.PinnedPCM(2 * (k * per + GUARD))
            hip = pdmp3_amd.load_library()
            hip.pdmp3_hip_host_is_pinned.argtypes = [C.c_void_p, C.c_size_t]
            pf = pin.array.view(np.float32)
            assert hip.pdmp3_hip_host_is_pinned(pf.ctypes.data, pf.nbytes) == 1
            pf[:] = SENT
            pd = pf[:k * per].reshape(shape)
            out, valid2 = dec.decode_clips_stft(src, f, mode=mode, out=pd, **p)
            assert (pf[k * per:] == SENT).all() and np.array_equal(valid, valid2)
            assert np.array_equal(pd.view(np.uint32), dense.view(np.uint32))
            if mode == "complex":                                               # a complex64 numpy array is the same memory
                z = np.full((k, 1, nb, f), SENT, dtype=np.complex64)
                dec.decode_clips_stft(src, f, mode=mode, out=z, **p)
                assert np.array_equal(z.view(np.float32).reshape(shape).view(np.uint32), dense.view(np.uint32))
        # stereo rows with a guard between the channels: one copy a channel; dense stereo rows: one copy
        p2 = dict(p, channels=2)
        sig2 = _signal(dec, clips, f, p2)
        got, valid = _run(dec, "numpy", clips, f, p2, "complex")
        print("strided stereo numpy rows: worst error / bound %.4f" % _check(clips, sig2, got, valid, f, p2, "complex"))
        dense2 = np.full((k, 2, nb, f, 2), SENT, dtype=np.float32)
        dec.decode_clips_stft(src, f, out=dense2, **p2)
        assert np.array_equal(dense2.view(np.uint32), got.view(np.uint32))
    finally:
        dec.close()


def test_a_refused_clip_in_the_middle_of_a_batch_and_bad_arguments():
    from pdmp3_amd import api
    p, f = P16, 35
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
        for kind, mode in (("device", "complex"), ("numpy", "log10")):
            per = _per(p, mode) * f
            for mid, exc, code in (((s["mixed/mpeg1-lsf"], mix, 0), api.MixedFormat, -3), ((bad, bix, 10), api.RingReplay, -2)):
                big, view = cg.destination(kind, 3, 1, calls.stft_inner(nb, f, mode))
                src = [(s["48k"], cg.ref("48k")[0], 100), mid, (s["22k"], cg.ref("22k")[0], 3000)]
                with pytest.raises(exc) as e:
                    dec.decode_clips_stft(src, f, mode=mode, out=view, **p)
                host = cg.host(big).reshape(3, 1, per + GUARD)
                assert e.value.valid[1] == code and (host[1] == SENT).all()
                assert (host[:, :, per:] == SENT).all()
                got = host[[0, 2], :, :per].reshape((2, 1, nb, f, 2) if mode == "complex" else (2, 1, nb, f))
                _check(good, sig, got, e.value.valid[[0, 2]], f, p, mode)
        # bad arguments: nothing is written
        big, view = cg.destination("device", 1, 1, calls.stft_inner(nb, f, "log10"))
        src = [(s["48k"], cg.ref("48k")[0], 0)]
        nan_window = np.ones(400, dtype=np.float32)
        nan_window[123] = np.nan
        for bad_p in (dict(n_fft=401), dict(n_fft=2048), dict(hop=0), dict(hop=401), dict(win_length=401), dict(window=nan_window),
                      dict(floor=0.0), dict(width=65)):
            q = dict(p, **bad_p)
            bb, bv = (big, view) if q["n_fft"] == 400 else cg.destination("device", 1, 1, calls.stft_inner(q["n_fft"] // 2 + 1, f, "log10"))
            with pytest.raises(RuntimeError):
                dec.decode_clips_stft(src, f, mode="log10", out=bv, **q)
            assert (cg.host(bb) == SENT).all()
        with pytest.raises(RuntimeError):
            dec.decode_clips_stft([(s["48k"], cg.ref("48k")[0], -1)], f, mode="log10", out=view, **p)
        with pytest.raises(RuntimeError):            # (rate 0 and clips of different rates)
            dec.decode_clips_stft(src + [(s["32k"], cg.ref("32k")[0], 0)], f, **dict(p, sample_rate=0))
        assert (cg.host(big) == SENT).all()
    finally:
        dec.close()
        bix.close()


def test_one_decoder_through_small_large_small_and_the_other_calls_around_it():
    """two windows of one length take turns (the table's key is the window's contents, not its length or address), more
    windows than the decoder keeps tables pass through it, and the audio call, the mel call and decode_range are what they were"""
    from pdmp3_amd import api
    rng = np.random.default_rng(9)
    wa = rng.random(400, dtype=np.float32)
    wb = rng.random(400, dtype=np.float32)
    pa, pb = dict(P16, window=wa), dict(P16, window=wb)
    small = [("32k", 500), ("8k", 1234)]
    large = [(n, s) for n in ("mixed/mono-stereo", "48k", "32k", "22k", "16k-mono", "8k") for s in (0, 999, 20001)]
    fresh = cg.decoder()
    try:
        audio_before, av = calls.audio_run(fresh, "device", [("48k", 700), ("22k", 9000)], 6000, 16000, 1)
        mel_before, mv = calls.mel_run(fresh, "device", small, 9, cases.MEL_P16, "log10")
        ix = cg.ref("48k")[0]
        plain_before = fresh.decode_range(cg.streams()["48k"], ix, 33, 50).copy()
        a_fresh, _ = _run(fresh, "device", small, 9, pa, "complex")
    finally:
        fresh.close()
    dec = cg.decoder()
    try:
        a, va = _run(dec, "device", small, 9, pa, "complex")
        b, vb = _run(dec, "device", small, 9, pb, "complex")
        assert np.array_equal(a.view(np.uint32), a_fresh.view(np.uint32)) and not np.array_equal(a, b)
        sig = _signal(dec, large, 300, pb)
        big, vbig = _run(dec, "device", large, 300, pb, "complex")
        print("the large call: worst error / bound %.4f" % _check(large, sig, big, vbig, 300, pb, "complex"))
        # the same values in another array, and the array of the first window overwritten with the second's values
        a2, _ = _run(dec, "device", small, 9, dict(P16, window=wa.copy()), "complex")
        assert np.array_equal(a.view(np.uint32), a2.view(np.uint32))
        scratch = wa.copy()
        _run(dec, "device", small, 9, dict(P16, window=scratch), "complex")
        scratch[:] = wb
        b2, _ = _run(dec, "device", small, 9, dict(P16, window=scratch), "complex")
        assert np.array_equal(b.view(np.uint32), b2.view(np.uint32))
        # more tables than the decoder keeps, other shapes, then the first again
        for i in range(6):
            _run(dec, "device", small, 3, dict(P16, window=rng.random(400, dtype=np.float32)), "power")
        _run(dec, "device", small, 9, P24, "power")
        _run(dec, "device", [("48k", 10)], 17, P48, "log10")
        c, vc = _run(dec, "numpy", small, 9, pa, "complex")
        assert np.array_equal(a.view(np.uint32), c.view(np.uint32)) and np.array_equal(va, vc)
        audio_after, av2 = calls.audio_run(dec, "device", [("48k", 700), ("22k", 9000)], 6000, 16000, 1)
        assert np.array_equal(audio_before.view(np.uint32), audio_after.view(np.uint32)) and np.array_equal(av, av2)
        mel_after, mv2 = calls.mel_run(dec, "device", small, 9, cases.MEL_P16, "log10")
        assert np.array_equal(mel_before.view(np.uint32), mel_after.view(np.uint32)) and np.array_equal(mv, mv2)
        plain_after = dec.decode_range(cg.streams()["48k"], cg.ref("48k")[0], 33, 50)
        assert np.array_equal(plain_before, plain_after)
    finally:
        dec.close()


def test_return_types_and_empty_calls():
    import torch
    src = [(cg.streams()["32k"], cg.ref("32k")[0], 1000)]
    dec = cg.decoder()
    try:
        out, valid = dec.decode_clips_stft(src, 50)
        assert tuple(out.shape) == (1, 1, 201, 50) and out.is_cuda and out.dtype == torch.complex64 and valid[0] == 50
        sig = _signal(dec, [("32k", 1000)], 50, P16)
        as_real = cg.host(torch.view_as_real(out))
        _check([("32k", 1000)], sig, as_real, valid, 50, P16, "complex")
        plain, _ = _run(dec, "device", [("32k", 1000)], 50, P16, "complex")
        assert np.array_equal(as_real.view(np.uint32), plain.view(np.uint32))
        # a row at an odd float: the pairs' 8-byte stores are 4-byte aligned there, the values the same
        odd, _ = _run(dec, "device", [("32k", 1000)], 50, P16, "complex", offset=1)
        assert np.array_equal(odd.view(np.uint32), plain.view(np.uint32))
        # a complex64 destination of the caller's
        z = torch.full((1, 1, 201, 50), complex(float(SENT), float(SENT)), dtype=torch.complex64, device="cuda")
        got, _ = dec.decode_clips_stft(src, 50, out=z)
        assert got is z and np.array_equal(cg.host(torch.view_as_real(z)).view(np.uint32), plain.view(np.uint32))
        out, valid = dec.decode_clips_stft(src, 50, mode="magnitude", channels=2)
        assert tuple(out.shape) == (1, 2, 201, 50) and out.dtype == torch.float32
        out, valid = dec.decode_clips_stft([], 10)
        assert tuple(out.shape) == (0, 1, 201, 10) and out.dtype == torch.complex64 and valid.size == 0
        out, valid = dec.decode_clips_stft(src, 0)
        assert tuple(out.shape) == (1, 1, 201, 0) and valid[0] == 0
        out, valid = dec.decode_clips_stft(src, 0, mode="power", n_fft=512)
        assert tuple(out.shape) == (1, 1, 257, 0) and out.dtype == torch.float32 and valid[0] == 0
    finally:
        dec.close()
