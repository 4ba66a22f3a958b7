"""Kaldi-style MFCC features of clips on the GPU (include/pdmp3_bulk.h pdmp3_amd_bulk_decode_clips_mfcc, k_clip_mfcc; DESIGN.md
section 12).

The reference is made from the product's own signal: for every clip decode_clips_audio gives the binary32 samples its frames
read (the span from `start` on), tests/clip_mfcc_ref.py evaluates the definition on them step by step in binary64, and the mfcc
call's output has to agree within the binary32 bound derived there -- every value, none left out -- and to differ from it
wherever a row holds signal (a thing compared with itself cannot pass).  Destinations are filled with a sentinel first:
nothing outside a row's F * num_ceps floats may change.  Each device step runs once.

Streams and helpers: those of test_gpu_clip_audio.py; destinations: those of test_gpu_clip_fbank.py."""
import numpy as np
import pytest

import clip_audio_ref as aref
import clip_fbank_ref as fref
import clip_mfcc_ref as ref
import clip_streams
import test_gpu_clip_audio as tga
import test_gpu_clip_fbank as tgf
from clip_streams import ISO_LSF

pytestmark = pytest.mark.gpu
SENT, GUARD = tgf.SENT, tgf.GUARD

P16 = dict(sample_rate=16000, win_length=400, hop=160, num_mel_bins=23, num_ceps=13, channels=1)
P8 = dict(sample_rate=8000, win_length=200, hop=80, num_mel_bins=23, num_ceps=13, channels=1, use_energy=True, scale=32768.0)
POWN = dict(sample_rate=0, win_length=1024, hop=480, num_mel_bins=80, num_ceps=40, channels=2)         # the own rate (the 48 kHz stream), stereo
SMALL_N = dict(sample_rate=8000, win_length=16, hop=16, num_mel_bins=40, num_ceps=40, channels=1, low_freq=0.0)  # cepstra [tile][49], powers [tile][18]
SIX = tgf.SIX


def _definition(y, start, f, p, w, nv):
    return ref.mfcc(y, start, start, f, p["win_length"], p["hop"], w, nv, p["num_ceps"], p.get("cepstral_lifter", 22.0),
                    p.get("round_to_power_of_two", True), p.get("remove_dc_offset", True), p.get("preemphasis_coefficient", 0.97),
                    p.get("window_type", "povey"), p.get("blackman_coeff", 0.42), p.get("use_energy", False), p.get("htk_compat", False),
                    p.get("energy_floor", 1.0), p.get("subtract_mean", False), p.get("scale", 1.0))


def _src(clips):
    return [(tga._streams()[n], tga._ref(n)[0], s) for n, s in clips]


def _run(dec, kind, clips, f, p):
    """clips: (stream name, start) -> (host copy [k, c, f, num_ceps], valid)"""
    k, c, d = len(clips), p["channels"], p["num_ceps"]
    big, view = tgf._destination(kind, k, c, f, d)
    out, valid = dec.decode_clips_mfcc(_src(clips), f, out=view, **p)
    assert out is view
    host = tga._host(big)
    assert (host[:, :, f * d:] == SENT).all(), "written behind a row's floats"
    return host[:, :, :f * d].reshape(k, c, f, d), valid


def _check(clips, sig, got, valid, f, p):
    """every row against the definition on `sig`; -> worst error / bound over the rows that hold signal"""
    worst = 0.0
    for i, (n, s) in enumerate(clips):
        ix = tga._ref(n)[0]
        j_all = aref.out_length(ix.samples, ix.rate, tgf._rate(p, n))
        nv = fref.valid(j_all, s, p["win_length"], p["hop"], f)
        assert int(valid[i]) == nv, (n, s, valid[i], nv)
        want, bound = _definition(sig[i], s, f, p, tgf._filterbank(p, n), nv)
        assert np.isfinite(got[i]).all()
        err = np.abs(got[i].astype(np.float64) - want)
        assert (err <= bound).all(), "%s at %d: error beyond the bound by %g at %s" % (
            n, s, float((err - bound).max()), np.unravel_index(np.argmax(err - bound), err.shape))
        if p.get("subtract_mean", False) and nv == 1 and f == 1:
            # the only frame minus the mean of that one frame: x - x / 1, exactly 0.0 in the definition and in binary32 alike
            assert (want == 0.0).all() and (got[i] == 0.0).all(), (n, s)
        elif np.abs(sig[i]).sum() > 0:
            r = float((err / bound).max())
            assert 0.0 < r <= 1.0, (n, s, r)
            worst = max(worst, r)
    return worst


CASES = {
    # parameters, streams, frames, destinations
    "16k-23-bands-13-cepstra": (P16, SIX, 70, ("device", "numpy")),                       # three tiles of 32, the last partial
    "80-bands-80-cepstra": (dict(P16, num_mel_bins=80, num_ceps=80), ["48k", "22k"], 40, ("device",)),   # five column tiles over four waves
    "17-cepstra": (dict(P16, num_ceps=17), ["32k", "8k"], 40, ("device",)),               # a partial column tile
    "1-cepstrum": (dict(P16, num_ceps=1), ["32k", "8k"], 40, ("device",)),
    "8k-energy-first-int16": (P8, ["48k", "8k"], 45, ("device",)),
    "8k-energy-last-htk-int16": (dict(P8, htk_compat=True), ["48k", "8k"], 45, ("device",)),
    "htk-sqrt-2": (dict(P16, htk_compat=True), ["48k", "16k-mono"], 40, ("device",)),
    "no-lifter": (dict(P16, cepstral_lifter=0.0), ["48k", "16k-mono"], 40, ("device",)),
    "own-rate-1024-stereo": (POWN, ["48k"], 21, ("device",)),
    "n-equals-nw": (dict(P16, num_mel_bins=40, num_ceps=20, round_to_power_of_two=False), ["32k", "16k-mono"], 40, ("device",)),
    "cepstra-outgrow-powers": (SMALL_N, ["48k", "8k"], 70, ("device",)),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_against_binary64_on_the_products_own_signal(case):
    from pdmp3_amd import api
    p, names, f, kinds = CASES[case]
    assert api.mfcc_check(**dict(p, sample_rate=tgf._rate(p, names[0])))
    clips = [(n, s) for n in names for s in tgf._starts(n, p, f)]
    tile, _, lds = api.mfcc_tile(p["win_length"], tgf._n(p), p["hop"], p["num_mel_bins"], p["num_ceps"])
    if case == "own-rate-1024-stereo":
        assert tile == 16 and lds > 64 * 1024      # the static-array kernel
    else:
        assert tile == 32 and lds <= 64 * 1024
    if case == "cepstra-outgrow-powers":
        assert lds > api.fbank_tile(p["win_length"], tgf._n(p), p["hop"], p["num_mel_bins"])[2]
    dec = tga._decoder()
    try:
        sig = tgf._signal(dec, clips, f, p)
        for kind in kinds:
            got, valid = _run(dec, kind, clips, f, p)
            worst = _check(clips, sig, got, valid, f, p)
            print("%s (tile %d, LDS %d), %s: worst error / bound %.4f over %d clips of %d frames" % (case, tile, lds, kind, worst, len(clips), f))
            assert 0.0 < worst <= 1.0
    finally:
        dec.close()


def test_subtract_mean_and_the_edges_of_valid():
    """valid inside the second tile, valid = 0 (nothing is subtracted) and F = 1 (exactly 0.0)"""
    p = dict(P16, subtract_mean=True, use_energy=True)
    name = "32k"
    j_all = tgf._j(name, p)
    nw, hop = p["win_length"], p["hop"]
    dec = tga._decoder()
    try:
        f = 70
        clips = [(name, j_all - nw - (40 - 1) * hop - 1), (name, 777), (name, j_all - nw + 1), (name, j_all + 5)]
        sig = tgf._signal(dec, clips, f, p)
        got, valid = _run(dec, "device", clips, f, p)
        assert list(valid) == [40, 70, 0, 0]
        print("subtract_mean, valid 40 / 70 / 0 / 0 of 70: worst error / bound %.4f" % _check(clips, sig, got, valid, f, p))
        again, valid2 = _run(dec, "device", clips, f, p)
        assert np.array_equal(got.view(np.uint32), again.view(np.uint32)) and np.array_equal(valid, valid2)
        plain, _ = _run(dec, "device", clips[2:], f, dict(p, subtract_mean=False))
        assert np.array_equal(got[2:].view(np.uint32), plain.view(np.uint32))          # valid = 0: the same as without
        assert np.abs(plain[0]).sum() > 0
        for q in (p, dict(p, use_energy=False, htk_compat=True)):
            clips = [(name, 777), (name, 0)]
            sig = tgf._signal(dec, clips, 1, q)
            got, valid = _run(dec, "device", clips, 1, q)
            assert list(valid) == [1, 1] and (got == 0.0).all()
            _check(clips, sig, got, valid, 1, q)
    finally:
        dec.close()


@pytest.mark.parametrize("p", [P16, dict(P8, energy_floor=0.0, htk_compat=True), POWN], ids=["16k", "8k-energy-htk", "own-rate-tile-16"])
def test_slices_are_slices(p):
    """a clip at start + 5 H is, bit for bit, frames 5 .. of the clip at `start`: a frame's values do not depend on its place in a
    tile or on the clip it is in"""
    from pdmp3_amd import api
    tile = api.mfcc_tile(p["win_length"], tgf._n(p), p["hop"], p["num_mel_bins"], p["num_ceps"])[0]
    name, start = "48k", 4321
    assert start % p["hop"] != 0
    f_long = 2 * tile + 7
    dec = tga._decoder()
    try:
        long, _ = _run(dec, "device", [(name, start)], f_long, p)
        short, _ = _run(dec, "device", [(name, start + 5 * p["hop"]), (name, start + (tile - 1) * p["hop"])], f_long - tile, p)
        assert np.array_equal(long[0, :, 5:5 + f_long - tile].view(np.uint32), short[0].view(np.uint32))
        assert np.array_equal(long[0, :, tile - 1:f_long - 1].view(np.uint32), short[1, :, :f_long - tile].view(np.uint32))
        assert np.abs(long).sum() > 0
    finally:
        dec.close()


def test_a_refused_clip_in_the_middle_of_a_batch():
    from pdmp3_amd import api
    p, f = P16, 35
    d = p["num_ceps"]
    bad = clip_streams.replay_stream()
    bix = api.StreamIndex(bad, ISO_LSF)
    assert bix.replay
    mix = tga._ref("mixed/mpeg1-lsf")[0]
    assert not mix.one_format
    s = tga._streams()
    good = [("48k", 100), ("22k", 3000)]
    dec = tga._decoder()
    try:
        sig = tgf._signal(dec, good, f, p)
        for kind in ("device", "numpy"):
            for mid, exc, code in (((s["mixed/mpeg1-lsf"], mix, 0), api.MixedFormat, -3), ((bad, bix, 10), api.RingReplay, -2)):
                big, view = tgf._destination(kind, 3, 1, f, d)
                src = [(s["48k"], tga._ref("48k")[0], 100), mid, (s["22k"], tga._ref("22k")[0], 3000)]
                with pytest.raises(exc) as e:
                    dec.decode_clips_mfcc(src, f, out=view, **p)
                host = tga._host(big)
                assert e.value.valid[1] == code and (host[1] == SENT).all()
                assert (host[:, :, f * d:] == SENT).all()
                got = host[[0, 2], :, :f * d].reshape(2, 1, f, d)
                _check(good, sig, got, e.value.valid[[0, 2]], f, p)
        # bad arguments: nothing is written
        big, view = tgf._destination("device", 1, 1, f, d)
        src = [(s["48k"], tga._ref("48k")[0], 0)]
        for bad_p in (dict(cepstral_lifter=-1.0), dict(cepstral_lifter=float("nan")), dict(use_log_fbank=False), dict(win_length=1025), dict(hop=0),
                      dict(high_freq=8000.5), dict(scale=0.0), dict(width=65), dict(dither=1.0), dict(use_power=False), dict(raw_energy=False),
                      dict(snip_edges=False), dict(vtln_warp=1.1)):
            with pytest.raises(RuntimeError):
                dec.decode_clips_mfcc(src, f, out=view, **dict(p, **bad_p))
        for nc in (0, 24):
            with pytest.raises(RuntimeError):
                dec.decode_clips_mfcc(src, f, out=tgf._destination("device", 1, 1, f, nc)[1], **dict(p, num_ceps=nc))
        with pytest.raises(RuntimeError):            # (rate 0 and clips of different rates)
            dec.decode_clips_mfcc(src + [(s["32k"], tga._ref("32k")[0], 0)], f, **dict(p, sample_rate=0))
        assert (tga._host(big) == SENT).all()
    finally:
        dec.close()
        bix.close()


def test_host_destinations_with_a_guard_behind_the_last_row():
    """a dense numpy array (its rows leave the stage in one copy) and stereo rows with a guard between the channels"""
    p, f = P16, 37
    clips = [(n, s) for n in ("48k", "22k", "16k-mono") for s in tgf._starts(n, p, f)[1:4]]
    k, d = len(clips), p["num_ceps"]
    dec = tga._decoder()
    try:
        sig = tgf._signal(dec, clips, f, p)
        flat = np.full(k * f * d + GUARD, SENT, dtype=np.float32)
        dense = flat[:k * f * d].reshape(k, 1, f, d)
        out, valid = dec.decode_clips_mfcc(_src(clips), f, out=dense, **p)
        assert out is dense and (flat[k * f * d:] == SENT).all()
        print("dense numpy rows: worst error / bound %.4f" % _check(clips, sig, dense, valid, f, p))
        on_device, valid_dev = _run(dec, "device", clips, f, p)
        assert np.array_equal(dense.view(np.uint32), on_device.view(np.uint32)) and np.array_equal(valid, valid_dev)
        p2 = dict(p, channels=2, subtract_mean=True, use_energy=True)
        sig2 = tgf._signal(dec, clips, f, p2)
        got, valid = _run(dec, "numpy", clips, f, p2)
        print("strided stereo numpy rows: worst error / bound %.4f" % _check(clips, sig2, got, valid, f, p2))
        got_dev, valid_dev = _run(dec, "device", clips, f, p2)
        assert np.array_equal(got.view(np.uint32), got_dev.view(np.uint32)) and np.array_equal(valid, valid_dev)
    finally:
        dec.close()


def test_one_decoder_through_mfcc_fbank_mel_audio_and_plain_clips():
    """each call's result is what a fresh decoder gives, whatever ran on the decoder before it"""
    import test_gpu_clip_mel as tgm
    p = dict(P16, subtract_mean=True, use_energy=True)
    two = [("48k", 700), ("22k", 9000)]
    ix = tga._ref("48k")[0]
    fresh = tga._decoder()
    try:
        plain_before = fresh.decode_range(tga._streams()["48k"], ix, 33, 50).copy()
        audio_before, av = tga._run(fresh, "device", two, 6000, 16000, 1)
        mel_before, mv = tgm._run(fresh, "device", two, 40, tgm.P16, "log10")
        fbank_before, fv = tgf._run(fresh, "device", two, 40, tgf.P16)
    finally:
        fresh.close()
    fresh = tga._decoder()
    try:
        mfcc_before, cv = _run(fresh, "device", two, 40, p)
    finally:
        fresh.close()
    dec = tga._decoder()
    try:
        a, va = _run(dec, "device", two, 40, p)
        assert np.array_equal(a.view(np.uint32), mfcc_before.view(np.uint32)) and np.array_equal(va, cv)
        fbank_after, fv2 = tgf._run(dec, "device", two, 40, tgf.P16)
        assert np.array_equal(fbank_before.view(np.uint32), fbank_after.view(np.uint32)) and np.array_equal(fv, fv2)
        _run(dec, "device", two, 9, dict(P16, num_ceps=17, cepstral_lifter=0.5, htk_compat=True))      # (another table on the same decoder)
        mel_after, mv2 = tgm._run(dec, "device", two, 40, tgm.P16, "log10")
        assert np.array_equal(mel_before.view(np.uint32), mel_after.view(np.uint32)) and np.array_equal(mv, mv2)
        b, vb = _run(dec, "numpy", two, 40, p)
        assert np.array_equal(b.view(np.uint32), mfcc_before.view(np.uint32)) and np.array_equal(vb, cv)
        audio_after, av2 = tga._run(dec, "device", two, 6000, 16000, 1)
        assert np.array_equal(audio_before.view(np.uint32), audio_after.view(np.uint32)) and np.array_equal(av, av2)
        plain_after = dec.decode_range(tga._streams()["48k"], ix, 33, 50)
        assert np.array_equal(plain_before, plain_after)
        c, vc = _run(dec, "device", two, 40, p)
        assert np.array_equal(c.view(np.uint32), mfcc_before.view(np.uint32)) and np.array_equal(vc, cv)
    finally:
        dec.close()


def test_made_output_and_empty_calls():
    dec = tga._decoder()
    try:
        # torchaudio's defaults: 25 ms frames every 10 ms, 23 bins, 13 cepstra, lifter 22
        src = _src([("32k", 1000)])
        out, valid = dec.decode_clips_mfcc(src, 50)
        assert tuple(out.shape) == (1, 1, 50, 13) and out.is_cuda and valid[0] == 50
        sig = tgf._signal(dec, [("32k", 1000)], 50, P16)
        _check([("32k", 1000)], sig, tga._host(out), valid, 50, P16)
        out, valid = dec.decode_clips_mfcc([], 10)
        assert tuple(out.shape) == (0, 1, 10, 13) and valid.size == 0
        out, valid = dec.decode_clips_mfcc(src, 0)
        assert tuple(out.shape) == (1, 1, 0, 13) and valid[0] == 0
        big, view = tgf._destination("numpy", 1, 1, 0, 13)
        dec.decode_clips_mfcc(src, 0, out=view)
        assert (big == SENT).all()
    finally:
        dec.close()


def test_the_mfcc_call_against_the_fbank_call_through_the_inverse_dct():
    """two paths of the product: with every cepstrum kept, no lifter, no htk_compat and no energy the DCT rows are an orthonormal
    basis, so the mfcc output times B (binary64, on the host) is the log filterbank again, which decode_clips_fbank gives for the
    same clips.  Tolerance: both calls' bounds, the mfcc call's pushed through |B^T|."""
    f, nm = 40, 23
    p = dict(P16, num_ceps=nm, cepstral_lifter=0.0)
    pf = dict(tgf.P16, num_mel_bins=nm)
    clips = [(n, s) for n in ("48k", "8k") for s in tgf._starts(n, p, f)[1:5]]
    b = ref.dct_rows(nm, nm)                           # [c, m]
    assert np.abs(b.T @ b - np.eye(nm)).max() < 1e-14
    dec = tga._decoder()
    try:
        sig = tgf._signal(dec, clips, f, p)
        cep, valid = _run(dec, "device", clips, f, p)
        lg, valid_f = tgf._run(dec, "device", clips, f, pf)
        assert np.array_equal(valid, valid_f)
        worst = 0.0
        for i, (n, s) in enumerate(clips):
            w = tgf._filterbank(p, n)
            _, dc = _definition(sig[i], s, f, p, w, int(valid[i]))
            _, dl = tgf._definition(sig[i], s, f, pf, w, int(valid[i]))
            back = cep[i].astype(np.float64) @ b
            tol = dc @ np.abs(b) + dl
            err = np.abs(back - lg[i].astype(np.float64))
            assert (err <= tol).all(), (n, s, float((err - tol).max()))
            if np.abs(sig[i]).sum() > 0:
                worst = max(worst, float((err / tol).max()))
        print("mfcc times B against fbank: worst difference / tolerance %.4f" % worst)
        assert 0.0 < worst <= 1.0
    finally:
        dec.close()
