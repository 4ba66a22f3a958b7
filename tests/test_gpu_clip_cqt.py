"""The constant-Q transform of clips on the GPU (include/pdmp3_bulk.h pdmp3_amd_bulk_decode_clips_cqt, k_clip_cqt; DESIGN.md
section 16).

The reference is made from the product's own signal: for every clip decode_clips_audio gives the binary32 samples its frames
read (the span from max(0, start - h_0) on), tests/clip_cqt_ref.py evaluates the definition on them in binary64, and the call's
output has to agree within the binary32 bound derived there -- every value of every mode, none left out; the bound is 0 and the
output exactly 0 on silence in modes 0 - 2.  Destinations are filled with a sentinel first: nothing outside a row's floats may
change.  Each device step runs once.

Streams and helpers: tests/clip_gpu.py and tests/clip_gpu_calls.py."""
import math

import numpy as np
import pytest

import clip_audio_ref as aref
import clip_cqt_ref as ref
import clip_forms_cases as cases
import clip_gpu as cg
import clip_gpu_calls as calls
import clip_streams
from clip_gpu import GUARD, SENT
from clip_gpu_calls import centred_starts as _starts, cqt_geo as _geo, cqt_run as _run, cqt_shape as _shape, cqt_signal as _signal
from clip_streams import ISO_LSF

pytestmark = pytest.mark.gpu
U = ref.U
MODES = ["complex", "magnitude", "power", "log", "log10"]
C1 = ref.FMIN_C1
SEEN = {"im": False, "swap": False}

# (a) split and unsplit tiles, a last tile of 4 bins, a tile edge inside the clip (20 frames); (b) every tile split, N_0 = 29 783,
# the static array near its limit; (c) no split, one full tile and one bin, dynamic LDS; (d) the shortest filter 3 taps, hop 1;
# (e) tiles of 8 and of 4 frames: the hops come from the plan's restatement below
PA = dict(sample_rate=22050, hop=512, channels=2, fmin=C1, n_bins=84, bins_per_octave=12)
PB = dict(sample_rate=0, hop=256, channels=1, fmin=55.0, n_bins=96, bins_per_octave=24)
PC = dict(sample_rate=16000, hop=160, channels=1, fmin=1000.0, n_bins=17, bins_per_octave=12, norm=2, scale=2)
PD = dict(sample_rate=0, hop=1, channels=1, fmin=500.0, n_bins=3, bins_per_octave=1, filter_scale=0.875)
PE = dict(sample_rate=0, channels=1, fmin=C1, n_bins=24, bins_per_octave=12, norm=1, scale=0)


def _hop_for(tile, sr=44100):
    """the smallest multiple of 64 at which the plan of (e) at 44.1 kHz takes `tile` frames"""
    return next(h for h in range(64, 8193, 64) if ref.plan(sr, h, **_shape(PE))[0] == tile)


PE8, PE4 = dict(PE, hop=_hop_for(8)), dict(PE, hop=_hop_for(4))


def _check(clips, sig, got, valid, f, p, mode, floor=1e-10):
    """every row against the definition on `sig`; -> worst error / bound over the rows that hold signal"""
    worst = 0.0
    m = MODES.index(mode)
    for i, (n, s) in enumerate(clips):
        ix = cg.ref(n)[0]
        rate = cg.rate(p, n)
        j_all = aref.out_length(ix.samples, ix.rate, rate)
        assert int(valid[i]) == ref.valid(j_all, s, p["hop"], f), (n, s, valid[i])
        s0, y = sig[i]
        want, bound = ref.cqt(y, s0, s, f, rate, p["hop"], m, floor, **_geo(p))
        assert want.shape == got[i].shape
        err = np.abs(got[i].astype(np.float64) - want)
        assert (err <= bound).all(), "%s at %d, mode %s: error beyond the bound by %g at %s" % (
            n, s, mode, float((err - bound).max()), np.unravel_index(np.argmax(err - bound), err.shape))
        nz = bound > 0
        if m <= 2:
            assert (got[i][~nz] == 0.0).all()
        if np.abs(y).sum() > 0 and nz.any():
            r = float((err[nz] / bound[nz]).max())
            assert 0.0 < r <= 1.0, (n, s, mode, r)
            worst = max(worst, r)
            if m == 0:
                # where Im (and Re - Im) is well above the bound, its sign (and a swap with Re) shows in the comparison above;
                # the long filters' bound is a larger part of a value than the STFT's, so the callers ask for it once a case
                SEEN["im"] |= bool((np.abs(want[..., 1]) > 4.0 * bound[..., 1])[nz[..., 1]].any())
                SEEN["swap"] |= bool((np.abs(want[..., 0] - want[..., 1]) > 4.0 * bound[..., 0])[nz[..., 0]].any())
    return worst


CASES = {
    "a-22k-c1-84-stereo": (PA, ["22k", "48k", "mixed/mono-stereo"], 20, "tile16-static", 4, 6),
    "b-48k-own-rate-96-bins": (PB, ["48k"], 18, "tile16-static", 6, 6),
    "c-16k-17-bins": (PC, ["32k", "16k-mono"], 35, "tile16-dyn", 0, 2),
    "d-8k-three-taps-hop-1": (PD, ["8k"], 40, "tile16-dyn", 0, 1),
    "e-44k-tile-8": (PE8, ["44k-mono"], 11, "tile8-static", 2, 2),
    "e-44k-tile-4": (PE4, ["44k-mono"], 7, "tile4-static", 2, 2),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_against_binary64_on_the_products_own_signal(case):
    from pdmp3_amd import api
    p, names, f, path, n_split, n_tiles = CASES[case]
    rate = cg.rate(p, names[0])
    assert all(cg.rate(p, n) == rate for n in names)
    if case[0] == "a":
        assert cg.ref("22k")[0].rate == 22050 and cg.ref("48k")[0].rate == 48000
    if case[0] == "b":
        assert rate == 48000 and 2 * api.cqt_lengths(rate, **_shape(p))[1][0] + 1 == 29783 and api.cqt_plan(rate, hop=p["hop"], **_shape(p))[2] == 153632
    if case[0] == "d":
        assert rate == 8000 and 2 * api.cqt_lengths(rate, **_shape(p))[1][-1] + 1 == 3
    # the launch path and the tile, from the plan function and from its restatement
    plan = api.cqt_plan(rate, hop=p["hop"], **_shape(p))
    want = ref.plan(rate, p["hop"], **_shape(p))
    assert plan == want[:6] and want[6] == path and plan[5] == n_split and (p["n_bins"] + 15) // 16 == n_tiles
    tile = plan[0]
    assert f > tile                                                          # (a tile edge inside the clip)
    clips = [(n, s) for n in names for s in _starts(n, p, f)]
    SEEN.update(im=False, swap=False)
    dec = cg.decoder()
    try:
        sig = _signal(dec, clips, f, p)
        for mode in MODES:
            for kind in ("device", "numpy") if mode in ("complex", "log10") else ("device",):
                got, valid = _run(dec, kind, clips, f, p, mode)
                worst = _check(clips, sig, got, valid, f, p, mode)
                print("%s (tile %d, %s, %d of %d tiles split), mode %s, %s: worst error / bound %.4f over %d clips of %d frames"
                      % (case, tile, path, n_split, n_tiles, mode, kind, worst, len(clips), f))
                assert 0.0 < worst <= 1.0
        assert SEEN["im"] and SEEN["swap"]
    finally:
        dec.close()


def test_mode_0_rederives_the_others_bit_for_bit():
    """Re^2 + Im^2 through the product's own arithmetic on mode 0's output is mode 2's, its correctly rounded square root mode
    1's, bit for bit: a transposed frame, a swapped bin or a mixed pair would show"""
    import clip_stft_ref as sref
    f, clips = 19, [("48k", 4321), ("22k", 0)]
    dec = cg.decoder()
    try:
        z, _ = _run(dec, "device", clips, f, PA, "complex")
        power, _ = _run(dec, "device", clips, f, PA, "power")
        mag, _ = _run(dec, "device", clips, f, PA, "magnitude")
        want = sref.power_as_the_product(z[..., 0], z[..., 1])
        assert np.array_equal(want.view(np.uint32), power.view(np.uint32))
        assert np.array_equal(np.sqrt(want).view(np.uint32), mag.view(np.uint32))
        assert np.abs(z[..., 1]).sum() > 0 and not np.array_equal(z[..., 0], z[..., 1])
    finally:
        dec.close()


def test_frames_are_frames_and_slices_of_a_batch_are_slices():
    """(a): frame f of a clip at `start` is frame 0 of a clip at start + f H, bit for bit, on both sides of the kernel's tile
    edge; a clip's row does not depend on the batch around it"""
    from pdmp3_amd import api
    p = PA
    name, start = "48k", 4321
    assert start % p["hop"] != 0
    tile = api.cqt_plan(22050, hop=p["hop"], **_shape(p))[0]
    dec = cg.decoder()
    try:
        fs = [0, 1, tile - 1, tile, tile + 1, tile + 4]
        f_long = tile + 6
        for mode in ("complex", "log10"):
            long, _ = _run(dec, "device", [(name, start)], f_long, p, mode)
            batch = [(name, start + f * p["hop"]) for f in fs]
            short, _ = _run(dec, "device", batch, 2, p, mode)
            for i, f in enumerate(fs):
                assert np.array_equal(long[0, :, :, f].view(np.uint32), short[i, :, :, 0].view(np.uint32)), (mode, f)
                assert np.array_equal(long[0, :, :, f + 1].view(np.uint32), short[i, :, :, 1].view(np.uint32)), (mode, f)
            assert np.abs(long).sum() > 0
            # slices of the batch: the middle rows alone, and in another order among other clips
            part, _ = _run(dec, "device", batch[2:5], 2, p, mode)
            assert np.array_equal(part.view(np.uint32), short[2:5].view(np.uint32))
            mixed, _ = _run(dec, "device", [("22k", 999), batch[4], batch[1]], 2, p, mode)
            assert np.array_equal(mixed[1].view(np.uint32), short[4].view(np.uint32)) and np.array_equal(mixed[2].view(np.uint32), short[1].view(np.uint32))
    finally:
        dec.close()


def test_clips_wholly_behind_the_end():
    p, f, name = PC, 18, "32k"
    ix = cg.ref(name)[0]
    j_all = aref.out_length(ix.samples, ix.rate, 16000)
    h0 = int(ref.lengths(16000, **_shape(p))[2][0])
    dec = cg.decoder()
    try:
        stats = dec.clip_stats()
        clips = [(name, j_all + h0), (name, j_all + 10 ** 6), (name, 2 ** 40)]
        for mode, floor in (("complex", 1e-10), ("magnitude", 1e-10), ("power", 0.0), ("log", 1e-10), ("log10", 1e-10), ("log10", 3e-5)):
            got, valid = _run(dec, "device", clips, f, p, mode, floor)
            assert list(valid) == [0, 0, 0]
            if mode in ("complex", "magnitude", "power"):
                assert (got == 0.0).all()
                continue
            fl = float(np.float32(floor))
            want = math.log(fl) if mode == "log" else math.log10(fl)
            assert (np.abs(got.astype(np.float64) - want) <= ref.LOG_C * U * abs(want)).all(), (mode, floor)
        assert dec.clip_stats() == stats
    finally:
        dec.close()


def test_a_refused_clip_in_the_middle_of_a_batch_and_bad_arguments():
    from pdmp3_amd import api
    p, f = PC, 19
    nb = p["n_bins"]
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
            per = nb * f * (2 if mode == "complex" else 1)
            for mid, exc, code in (((s["mixed/mpeg1-lsf"], mix, 0), api.MixedFormat, -3), ((bad, bix, 10), api.RingReplay, -2)):
                big, view = cg.destination(kind, 3, 1, calls.stft_inner(nb, f, mode))
                src = [(s["48k"], cg.ref("48k")[0], 100), mid, (s["22k"], cg.ref("22k")[0], 3000)]
                with pytest.raises(exc) as e:
                    dec.decode_clips_cqt(src, f, mode=mode, out=view, **p)
                host = cg.host(big).reshape(3, 1, per + GUARD)
                assert e.value.valid[1] == code and (host[1] == SENT).all()
                assert (host[:, :, per:] == SENT).all()
                got = host[[0, 2], :, :per].reshape((2, 1, nb, f, 2) if mode == "complex" else (2, 1, nb, f))
                _check(good, sig, got, e.value.valid[[0, 2]], f, p, mode)
        # bad arguments: nothing is written
        big, view = cg.destination("device", 1, 1, calls.stft_inner(nb, f, "log10"))
        src = [(s["48k"], cg.ref("48k")[0], 0)]
        for bad_p in (dict(hop=0), dict(hop=8193), dict(fmin=0.0), dict(fmin=7600.0), dict(fmin=5.0), dict(bins_per_octave=0), dict(bins_per_octave=97),
                      dict(filter_scale=0.0), dict(filter_scale=float("nan")), dict(norm=3), dict(scale=-1), dict(floor=0.0), dict(width=65)):
            with pytest.raises(RuntimeError):
                dec.decode_clips_cqt(src, f, mode="log10", out=view, **dict(p, **bad_p))
            assert (cg.host(big) == SENT).all(), bad_p
        with pytest.raises(RuntimeError):
            dec.decode_clips_cqt(src, f, mode=7, out=view, **p)
        with pytest.raises(RuntimeError):
            dec.decode_clips_cqt([(s["48k"], cg.ref("48k")[0], -1)], f, mode="log10", out=view, **p)
        with pytest.raises(RuntimeError):            # (rate 0 and clips of different rates)
            dec.decode_clips_cqt(src + [(s["32k"], cg.ref("32k")[0], 0)], f, mode="log10", **dict(p, sample_rate=0))
        assert (cg.host(big) == SENT).all()
    finally:
        dec.close()
        bix.close()


def test_more_clips_than_one_grid():
    """32 768 + 5 clips of case (d) in one call: pdmp3_hip_clip_cqt launches the kernel twice (a grid's y extent), the second
    time from descriptor 32 768 on.  Sixty-four distinct clips are held against the definition, every row is bit-equal to its
    twin among them; the last five are other clips than rows 0 .. 4, one of them behind the end"""
    name, k, f, p = "8k", 32768 + 5, 40, PD
    ix = cg.ref(name)[0]
    j_all = aref.out_length(ix.samples, ix.rate, ix.rate)
    starts = [1000 + 3001 * i for i in range(62)] + [j_all + 9, j_all - 5]
    assert starts[61] + f + 16 < j_all
    twin = (np.arange(k, dtype=np.int64) * 7) % 62
    twin[32768:] = [62, 63, 61, 60, 59]
    assert not np.any(twin[32768:] == twin[:5])
    mp3 = cg.streams()[name]
    dec = cg.decoder()
    try:
        first = [(name, s) for s in starts]
        sig = _signal(dec, first, f, p)
        base, valid64 = _run(dec, "device", first, f, p, "magnitude")
        assert 0.0 < _check(first, sig, base, valid64, f, p, "magnitude") <= 1.0
        assert list(valid64[61:]) == [f, 0, 5]
        big, view = cg.destination("device", k, 1, (p["n_bins"], f))
        out, valid = dec.decode_clips_cqt([(mp3, ix, int(starts[t])) for t in twin], f, mode="magnitude", out=view, **p)
        per = p["n_bins"] * f
        host = cg.host(big).reshape(k, per + GUARD)
        assert (host[:, per:] == SENT).all(), "written behind a row's floats"
        assert np.array_equal(valid, valid64[twin]) and list(valid[32768:]) == [0, 5, f, f, f]
        same = (host[:, :per].view(np.uint32) == base[twin].reshape(k, per).view(np.uint32)).all(axis=1)
        bad = np.flatnonzero(~same)
        assert bad.size == 0, "%d rows differ from their twins, %d of them in the second launch: %s" % (bad.size, int((bad >= 32768).sum()), bad[:8].tolist())
        assert np.unique(base[:62, 0, 0, 0]).size > 32
    finally:
        dec.close()


def test_one_decoder_through_this_call_the_other_calls_and_this_call_again():
    """this call, decode_clips_stft, decode_clips_mel_long, decode_clips_audio, this call with another spec and with more specs
    than the decoder keeps tables -- and all of it again: every call is bit-equal to its first answer"""
    small = [("48k", 500), ("22k", 1234)]
    dec = cg.decoder()
    try:
        def round_():
            out = []
            out.append(_run(dec, "device", small, 9, PC, "complex"))
            out.append(calls.stft_run(dec, "device", small, 9, cases.STFT_P16, "complex"))
            pl = dict(sample_rate=22050, n_fft=2048, hop=512, n_mels=64, scale="slaney", norm="slaney", channels=1)
            out.append(dec.decode_clips_mel_long([(cg.streams()[n], cg.ref(n)[0], s) for n, s in small], 9, mode="log10", **pl))
            out.append(calls.audio_run(dec, "device", [("48k", 700), ("22k", 9000)], 6000, 16000, 1))
            out.append(_run(dec, "device", small, 9, dict(PC, norm=1, scale=1), "complex"))
            for i in range(5):                                                   # (more tables than the decoder keeps)
                out.append(_run(dec, "device", small, 3, dict(PC, fmin=1000.0 + 10.0 * i), "power"))
            out.append(_run(dec, "numpy", small, 9, PC, "complex"))
            return [(cg.host(a), v) for a, v in out]
        one, two = round_(), round_()
        assert len(one) == len(two)
        for (a, va), (b, vb) in zip(one, two):
            a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
            assert a.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
            assert np.array_equal(va, vb)
        assert np.array_equal(one[0][0].view(np.uint32), one[-1][0].view(np.uint32))        # (device and numpy destinations)
        assert not np.array_equal(one[0][0], one[4][0])                                     # (another spec is another answer)
        sig = _signal(dec, small, 9, PC)
        print("after all the calls: worst error / bound %.4f" % _check(small, sig, two[0][0], two[0][1], 9, PC, "complex"))
    finally:
        dec.close()


def test_return_types_and_empty_calls():
    import torch
    src = [(cg.streams()["22k"], cg.ref("22k")[0], 1000)]
    dec = cg.decoder()
    try:
        out, valid = dec.decode_clips_cqt(src, 17)                              # the defaults: 22 050 Hz, C1, 84 bins, magnitude
        assert tuple(out.shape) == (1, 1, 84, 17) and out.is_cuda and out.dtype == torch.float32 and valid[0] == 17
        p = dict(PA, channels=1)
        sig = _signal(dec, [("22k", 1000)], 17, p)
        _check([("22k", 1000)], sig, cg.host(out), valid, 17, p, "magnitude")
        z, _ = dec.decode_clips_cqt(src, 17, mode="complex")
        assert tuple(z.shape) == (1, 1, 84, 17) and z.dtype == torch.complex64
        plain, _ = _run(dec, "device", [("22k", 1000)], 17, p, "complex")
        assert np.array_equal(cg.host(torch.view_as_real(z)).view(np.uint32), plain.view(np.uint32))
        # a row at an odd float: the pairs' 8-byte stores are 4-byte aligned there, the values the same
        odd, _ = _run(dec, "device", [("22k", 1000)], 17, p, "complex", offset=1)
        assert np.array_equal(odd.view(np.uint32), plain.view(np.uint32))
        out, valid = dec.decode_clips_cqt([], 10)
        assert tuple(out.shape) == (0, 1, 84, 10) and valid.size == 0
        out, valid = dec.decode_clips_cqt(src, 0, mode="complex", n_bins=24)
        assert tuple(out.shape) == (1, 1, 24, 0) and out.dtype == torch.complex64 and valid[0] == 0
    finally:
        dec.close()
