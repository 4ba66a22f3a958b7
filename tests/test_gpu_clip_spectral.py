"""Spectral descriptors of clips at n_fft 2048 and 4096 on the GPU (include/pdmp3_bulk.h pdmp3_amd_bulk_decode_clips_spectral,
k_clip_spectral).

The reference is made from the product's own signal, as in test_gpu_clip_mel_long.py: decode_clips_audio gives the binary32
samples a clip's frames read, tests/clip_spectral_ref.py evaluates the six rows on them in binary64, and the call's output has to
agree within the bounds derived there -- every value of rows 0 .. 3 and 5, none left out; row 1 exactly; row 4, a decision, by
the undecided rule with its cap of one frame in ten, the share printed.  The streams are the packer's, whose audio is noise: at
roll_percent 0.85 the definition itself cannot decide most of their frames within the derived bound (clip_spectral_ref.py says
why), so the cases against binary64 run at roll_percent 0.01 (N 2048) and 0.005 (N 4096, and hop 1), where it can -- checked on the
CPU before relying on it; roll_percent 0.85 is held exactly, bin for bin, against the stated order on the spectrum call's own
magnitudes (test_rows_2_to_5_are_the_reductions_of_the_spectrum_calls_output).  Destinations are filled with a sentinel first.
Each device step runs once; a clip's reference is computed once.

Streams and helpers: tests/clip_gpu.py and tests/clip_gpu_calls.py."""
import numpy as np
import pytest

import clip_audio_ref as aref
import clip_gpu as cg
import clip_gpu_calls as calls
import clip_spectral_ref as spref
import clip_streams
from clip_gpu import GUARD, SENT, signal as _signal
from clip_gpu_calls import mel_starts as _starts
from clip_streams import ISO_LSF

pytestmark = pytest.mark.gpu
U = spref.U
ROWS = len(spref.ROWS)

W1764 = (np.random.default_rng(1764).random(1764, dtype=np.float32) * np.float32(1.5) - np.float32(0.25)).astype(np.float32)
PA = dict(sample_rate=0, n_fft=2048, hop=512, channels=2, roll_percent=0.01)           # the 48 kHz stream at its own rate
PB = dict(sample_rate=22050, n_fft=2048, hop=441, channels=1, win_length=1764, window=W1764, roll_percent=0.01)
PC = dict(sample_rate=0, n_fft=2048, hop=2048, channels=1, roll_percent=0.01)
PD = dict(sample_rate=0, n_fft=4096, hop=1024, channels=1, roll_percent=0.005)
PE = dict(sample_rate=0, n_fft=4096, hop=4096, channels=2, roll_percent=0.005)
PF = dict(sample_rate=0, n_fft=2048, hop=1, channels=1, roll_percent=0.005)         # (eleven frames one sample apart decide alike: the lower share)


def _run(dec, kind, clips, f, p):
    """clips: (stream name, start) -> (host copy [k, c, 6, f], valid)"""
    return cg.run(dec, "decode_clips_spectral", kind, clips, f, p["channels"], (ROWS, f), **p)


def _wants(clips, sig, f, p):
    """per clip clip_spectral_ref.spectral's result: the definition on the product's own signal"""
    return [spref.spectral(y, s0, s, f, p["n_fft"], p["hop"], cg.rate(p, n), p.get("roll_percent", 0.85), p.get("amin", 1e-10),
                           p.get("zcr_threshold", 1e-10), p.get("win_length"), p.get("window")) for (n, s), (s0, y) in zip(clips, sig)]


def _check(clips, wants, got, valid, f, p):
    """every row against the definition -> (worst error / bound per row, undecided frames, frames)"""
    worst = np.zeros(ROWS)
    und = frames = 0
    for i, (n, s) in enumerate(clips):
        ix = cg.ref(n)[0]
        j_all = aref.out_length(ix.samples, ix.rate, cg.rate(p, n))
        assert int(valid[i]) == spref.sref.valid(j_all, s, p["hop"], f), (n, s, valid[i])
        res = wants[i]
        want, bound, signal = res["want"], res["bound"], res["signal"]
        assert want.shape == got[i].shape
        err = np.abs(got[i].astype(np.float64) - want)
        for r in (0, 1, 2, 3, 5):
            assert (err[:, r] <= bound[:, r]).all(), "%s at %d, row %s: error beyond the bound by %g at %s" % (
                n, s, spref.ROWS[r], float((err[:, r] - bound[:, r]).max()), np.unravel_index(np.argmax(err[:, r] - bound[:, r]), err[:, r].shape))
            nz = bound[:, r] > 0
            if nz.any():
                worst[r] = max(worst[r], float((err[:, r][nz] / bound[:, r][nz]).max()))
        assert np.array_equal(got[i][:, 1], want[:, 1].astype(np.float32)), (n, s, "zcr")
        u, fr = spref.check_rolloff(got[i][:, 4], res, cg.rate(p, n), p["n_fft"])
        und, frames = und + u, frames + fr
        assert (got[i][:, :5].transpose(0, 2, 1)[~signal].view(np.uint32) == 0).all(), (n, s, "a silent frame")
        assert (got[i][:, 5] > 0).all() and (got[i][:, 5] <= 1.0 + 1e-5).all()
    return worst, und, frames


CASES = {
    "a-48k-stereo-2048-hop-512": (PA, "48k", 11, "N2048-tile8"),                 # one full tile and a partial one
    "b-22k-2048-hop-441-own-window-1764": (PB, "22k", 11, "N2048-tile8"),
    "c-44k-mono-2048-hop-2048": (PC, "44k-mono", 11, "N2048-tile8"),
    "d-48k-4096-hop-1024": (PD, "48k", 5, "N4096-tile4"),
    "e-48k-stereo-4096-hop-4096": (PE, "48k", 5, "N4096-tile4"),
    "f-32k-2048-hop-1": (PF, "32k", 11, "N2048-tile8"),
}
RATES = {"48k": 48000, "22k": 22050, "44k-mono": 44100, "32k": 32000}


def test_the_cases_cover_both_launch_paths():
    assert set(path for _, _, _, path in CASES.values()) == set(spref.PATHS)
    for case, (p, name, f, path) in CASES.items():
        tile = spref.plan(p["n_fft"], p["hop"])
        assert tile[3] == path and tile[0] < f < 2 * tile[0], case           # one full tile plus a partial one


@pytest.mark.parametrize("case", sorted(CASES))
def test_against_binary64_on_the_products_own_signal(case):
    from pdmp3_amd import api
    p, name, f, path = CASES[case]
    assert cg.rate(p, name) == RATES[name]
    clips = [(name, s) for s in _starts(name, p, f)]
    tile = api.spectral_plan(p["n_fft"], p["hop"])[0]
    assert spref.plan(p["n_fft"], p["hop"])[3] == path and path.endswith("tile%d" % tile)
    dec = cg.decoder()
    try:
        sig = _signal(dec, clips, f, p)
        wants = _wants(clips, sig, f, p)
        for kind in ("device", "numpy"):
            got, valid = _run(dec, kind, clips, f, p)
            worst, und, frames = _check(clips, wants, got, valid, f, p)
            print("%s (tile %d, %s), %s: worst error / bound %s over %d clips of %d frames; roll-off undecided in %d of %d frames (%.1f %%)"
                  % (case, tile, path, kind, " ".join("%s %.4f" % (spref.ROWS[r], worst[r]) for r in (0, 2, 3, 5)), len(clips), f, und, frames,
                     100.0 * und / frames))
            assert und <= spref.UNDECIDED_CAP * frames
            assert 0.0 < worst[0] <= 1.0 and (worst <= 1.0).all()
    finally:
        dec.close()


@pytest.mark.parametrize("p,f", [(PA, 11), (PD, 6)], ids=["2048-hop-512", "4096-hop-1024"])
def test_rows_2_to_5_are_the_reductions_of_the_spectrum_calls_output(p, f):
    """the same formulas evaluated in binary64 on decode_clips_stft_long's magnitudes (rows 2 .. 4) and powers (row 5: the plane
    holds the power, and the magnitude is its correctly rounded square root) against this call at the default roll_percent 0.85:
    the spectrum is the same chains in both kernels, the Nyquist bin included, so what remains is the reductions' bound alone --
    and row 4, whose stated order clip_spectral_ref.rolloff_stated repeats, agrees bin for bin"""
    name = "48k"
    q = dict(p, roll_percent=0.85)
    clips = [(name, s) for s in (0, 57, 30011)]
    src = cg.src(clips)
    dec = cg.decoder()
    try:
        got, valid = _run(dec, "device", clips, f, q)
        long = dict(sample_rate=0, n_fft=p["n_fft"], hop=p["hop"], channels=p["channels"])
        mag, v1 = dec.decode_clips_stft_long(src, f, mode="magnitude", **long)
        power, v2 = dec.decode_clips_stft_long(src, f, mode="power", **long)
        assert np.array_equal(valid, v1) and np.array_equal(valid, v2)
        s32 = np.moveaxis(cg.host(mag), 2, 3)                              # [k, c, f, K]
        p32 = np.moveaxis(cg.host(power), 2, 3)
        assert s32.shape[-1] == p["n_fft"] // 2 + 1 and (s32[..., -1] > 0).any()
        want, bound = spref.from_spectrum(s32, p32, RATES[name], p["n_fft"], 0.85, 1e-10)
        mine = np.moveaxis(got[:, :, 2:6, :], 2, 3).astype(np.float64)       # [k, c, f, 4]
        err = np.abs(mine - want)
        assert (err <= bound).all(), (float((err - bound).max()), np.unravel_index(np.argmax(err - bound), err.shape))
        assert np.array_equal(mine[..., 2].astype(np.float32), want[..., 2].astype(np.float32)), "roll-off: another bin than the stated order's"
        for r, row in ((0, "centroid"), (1, "bandwidth"), (3, "flatness")):
            nz = bound[..., r] > 0
            ratio = float((err[..., r][nz] / bound[..., r][nz]).max())
            print("N %d: worst |%s - the reduction of the spectrum call's output| / bound = %.4f" % (p["n_fft"], row, ratio))
            assert ratio <= 1.0
        assert np.unique(want[..., 2]).size > 3
    finally:
        dec.close()


@pytest.mark.parametrize("p", [PA, PD], ids=["2048-hop-512", "4096-hop-1024"])
def test_frames_are_frames(p):
    """frame f of a clip at `start` is frame 0 of the clip at start + f H, bit for bit, on both sides of both tile edges"""
    from pdmp3_amd import api
    name, start = "48k", 4321
    assert start % p["hop"] != 0
    tile = api.spectral_plan(p["n_fft"], p["hop"])[0]
    fs = [0, 1, tile - 1, tile, tile + 1, 2 * tile - 1, 2 * tile, 2 * tile + 2]
    f_long = 2 * tile + 4
    dec = cg.decoder()
    try:
        long, _ = _run(dec, "device", [(name, start)], f_long, p)
        short, _ = _run(dec, "device", [(name, start + f * p["hop"]) for f in fs], 2, p)
        for i, f in enumerate(fs):
            assert np.array_equal(long[0, :, :, f].view(np.uint32), short[i, :, :, 0].view(np.uint32)), f
            assert np.array_equal(long[0, :, :, f + 1].view(np.uint32), short[i, :, :, 1].view(np.uint32)), f
        assert np.abs(long).sum() > 0
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
        assert np.abs(whole).sum() > 0
    finally:
        dec.close()


def test_a_refused_clip_in_the_middle_of_a_batch_and_bad_arguments():
    from pdmp3_amd import api
    p, f = dict(PA, sample_rate=16000, channels=1), 9
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
        per = ROWS * f
        for kind in ("device", "numpy"):
            for mid, exc, code in (((s["mixed/mpeg1-lsf"], mix, 0), api.MixedFormat, -3), ((bad, bix, 10), api.RingReplay, -2)):
                big, view = cg.destination(kind, 3, 1, (ROWS, f))
                src = [(s["48k"], cg.ref("48k")[0], 100), mid, (s["22k"], cg.ref("22k")[0], 3000)]
                with pytest.raises(exc) as e:
                    dec.decode_clips_spectral(src, f, out=view, **p)
                host = cg.host(big).reshape(3, 1, per + GUARD)
                assert e.value.valid[1] == code and (host[1] == SENT).all()
                assert (host[:, :, per:] == SENT).all()
                got = host[[0, 2], :, :per].reshape(2, 1, ROWS, f)
                _check(good, wants, got, e.value.valid[[0, 2]], f, p)
        # bad arguments: nothing is written
        big, view = cg.destination("device", 1, 1, (ROWS, f))
        src = [(s["48k"], cg.ref("48k")[0], 0)]
        nan_window = np.ones(2048, dtype=np.float32)
        nan_window[123] = np.nan
        for bad_p in (dict(n_fft=1024), dict(n_fft=8192), dict(n_fft=400), dict(hop=0), dict(hop=2049), dict(win_length=2049), dict(window=nan_window),
                      dict(roll_percent=0.0), dict(roll_percent=1.0), dict(roll_percent=float("nan")), dict(amin=0.0), dict(amin=-1.0),
                      dict(amin=float("inf")), dict(zcr_threshold=-1e-3), dict(zcr_threshold=float("nan")), dict(width=65)):
            with pytest.raises(RuntimeError):
                dec.decode_clips_spectral(src, f, out=view, **dict(p, **bad_p))
            assert (cg.host(big) == SENT).all(), bad_p
        with pytest.raises(RuntimeError):
            dec.decode_clips_spectral([(s["48k"], cg.ref("48k")[0], -1)], f, out=view, **p)
        with pytest.raises(RuntimeError):            # (rate 0 and clips of different rates)
            dec.decode_clips_spectral(src + [(s["32k"], cg.ref("32k")[0], 0)], f, **dict(p, sample_rate=0))
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
    clips = [(name, j_all + 5 * p["n_fft"]), (name, j_all + 1000000)]
    src = cg.src(clips)
    dec = cg.decoder()
    try:
        got, valid = _run(dec, "device", clips, f, p)
        assert (valid == 0).all() and (got[:, :, :5].view(np.uint32) == 0).all()     # rows 0 .. 4 exactly +0.0
        # row 5 of silence: every power is the floor, whose logarithm logf gives within LOG_C u |ln amin| -- exp of that at the most
        assert (np.abs(got[:, :, 5].astype(np.float64) - 1.0) <= 2.0 * spref.LOG_C * U * abs(np.log(1e-10))).all()
        out, valid = dec.decode_clips_spectral(src, f, sample_rate=0)
        assert tuple(out.shape) == (2, 2, ROWS, f) and out.is_cuda and out.dtype == torch.float32 and (valid == 0).all()
        out, valid = dec.decode_clips_spectral([], 10)
        assert tuple(out.shape) == (0, 1, ROWS, 10) and valid.size == 0
        out, valid = dec.decode_clips_spectral(src, 0, sample_rate=0, n_fft=4096, channels=1)
        assert tuple(out.shape) == (2, 1, ROWS, 0) and (valid == 0).all()
    finally:
        dec.close()


def test_more_clips_than_one_grid():
    """32 768 + 5 clips of one frame at (2048, 2048) in one call: pdmp3_hip_clip_spectral launches the kernel twice (a grid's y
    extent), the second time from descriptor 32 768 on.  Sixty-four distinct clips are held against the definition, every row is
    bit-equal to its twin among them; the last five are other clips than rows 0 .. 4, one of them behind the end"""
    name, k = "32k", 32768 + 5
    p = dict(PC, roll_percent=0.005)
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
        base, valid64 = _run(dec, "device", first, 1, p)
        worst, und, frames = _check(first, wants, base, valid64, 1, p)
        assert 0.0 < worst[0] <= 1.0 and und <= spref.UNDECIDED_CAP * frames
        assert list(valid64[61:]) == [1, 0, 1]
        big, view = cg.destination("device", k, 1, (ROWS, 1))
        out, valid = dec.decode_clips_spectral([(mp3, ix, int(starts[t])) for t in twin], 1, out=view, **p)
        host = cg.host(big)
        assert (host[:, :, ROWS:] == SENT).all(), "written behind a row's floats"
        assert np.array_equal(valid, valid64[twin]) and list(valid[32768:]) == [0, 1, 1, 1, 1]
        bad = np.flatnonzero((host[:, 0, :ROWS].view(np.uint32) != base[twin, 0, :, 0].view(np.uint32)).any(axis=1))
        assert bad.size == 0, "%d rows differ from their twins, %d of them in the second launch: %s" % (bad.size, int((bad >= 32768).sum()), bad[:8].tolist())
        assert np.unique(base[:62, 0, 2, 0]).size > 32
    finally:
        dec.close()


def test_one_decoder_through_this_call_the_other_calls_and_this_call_again():
    """the new call, decode_clips_stft_long, decode_clips_mel_long, decode_clips_audio, the new call with other parameters and
    with the other n_fft -- and all of it again: every call is bit-equal to its first answer; the transform's tables are shared
    with the spectrum and the log-mel call"""
    small = [("32k", 500), ("8k", 1234)]
    pa = dict(PA, sample_rate=16000, channels=1)
    pb = dict(pa, roll_percent=0.5, amin=1e-6, zcr_threshold=1e-3, win_length=1764, window=W1764)
    pd = dict(PD, sample_rate=16000)
    dec = cg.decoder()
    try:
        def once():
            return [_run(dec, "device", small, 9, pa),
                    calls.stft_long_run(dec, "device", small, 9, dict(calls.STFT_LONG_PA, sample_rate=16000, channels=1), "complex"),
                    calls.mel_long_run(dec, "device", small, 9, dict(calls.MEL_LONG_PA, sample_rate=16000, channels=1), "log10"),
                    calls.audio_run(dec, "device", [("48k", 700), ("22k", 9000)], 6000, 16000, 1),
                    _run(dec, "device", small, 9, pb),
                    _run(dec, "numpy", small, 5, pd)]
        a, b = once(), once()
        for i, ((x, vx), (y, vy)) in enumerate(zip(a, b)):
            assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)) and np.array_equal(vx, vy), i
            assert np.abs(x.astype(np.float64)).sum() > 0, i
        assert not np.array_equal(a[0][0], a[4][0])
        sig = _signal(dec, small, 9, pa)
        worst, und, frames = _check(small, _wants(small, sig, 9, pa), a[0][0], a[0][1], 9, pa)
        print("after the other calls: worst error / bound %s, roll-off undecided in %d of %d frames" % (np.round(worst, 4).tolist(), und, frames))
    finally:
        dec.close()
