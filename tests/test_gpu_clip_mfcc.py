"""Kaldi-style MFCC features of clips on the GPU (include/pdmp3_bulk.h pdmp3_amd_bulk_decode_clips_mfcc, k_clip_mfcc; DESIGN.md
section 12).

The reference is made from the product's own signal: for every clip decode_clips_audio gives the binary32 samples its frames
read (the span from `start` on), tests/clip_mfcc_ref.py evaluates the definition on them step by step in binary64, and the mfcc
call's output has to agree within the binary32 bound derived there -- every value, none left out -- and to differ from it
wherever a row holds signal (a thing compared with itself cannot pass).  Destinations are filled with a sentinel first:
nothing outside a row's F * num_ceps floats may change.  Each device step runs once.

Streams and helpers: tests/clip_gpu.py and tests/clip_gpu_calls.py."""
import numpy as np
import pytest

import clip_forms_cases as cases
import clip_gpu as cg
import clip_gpu_calls as calls
import clip_mfcc_ref as ref
import clip_streams
from clip_forms_cases import MFCC_CASES as CASES, MFCC_P8 as P8, MFCC_P16 as P16, MFCC_POWN as POWN
from clip_gpu import GUARD, SENT
from clip_gpu_calls import mfcc_check as _check, mfcc_definition as _definition, mfcc_run as _run
from clip_streams import ISO_LSF

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", sorted(CASES))
def test_against_binary64_on_the_products_own_signal(case):
    from pdmp3_amd import api
    p, names, f, kinds = CASES[case]
    assert api.mfcc_check(**dict(p, sample_rate=cg.rate(p, names[0])))
    clips = [(n, s) for n in names for s in calls.fbank_starts(n, p, f)]
    tile, _, lds = api.mfcc_tile(p["win_length"], calls.fbank_n(p), p["hop"], p["num_mel_bins"], p["num_ceps"])
    if case == "own-rate-1024-stereo":
        assert tile == 16 and lds > 64 * 1024      # the static-array kernel
    else:
        assert tile == 32 and lds <= 64 * 1024
    if case == "cepstra-outgrow-powers":
        assert lds > api.fbank_tile(p["win_length"], calls.fbank_n(p), p["hop"], p["num_mel_bins"])[2]
    dec = cg.decoder()
    try:
        sig = calls.fbank_signal(dec, clips, f, p)
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
    j_all = cg.j_all(p, name)
    nw, hop = p["win_length"], p["hop"]
    dec = cg.decoder()
    try:
        f = 70
        clips = [(name, j_all - nw - (40 - 1) * hop - 1), (name, 777), (name, j_all - nw + 1), (name, j_all + 5)]
        sig = calls.fbank_signal(dec, clips, f, p)
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
            sig = calls.fbank_signal(dec, clips, 1, q)
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
    tile = api.mfcc_tile(p["win_length"], calls.fbank_n(p), p["hop"], p["num_mel_bins"], p["num_ceps"])[0]
    name, start = "48k", 4321
    assert start % p["hop"] != 0
    f_long = 2 * tile + 7
    dec = cg.decoder()
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
    mix = cg.ref("mixed/mpeg1-lsf")[0]
    assert not mix.one_format
    s = cg.streams()
    good = [("48k", 100), ("22k", 3000)]
    dec = cg.decoder()
    try:
        sig = calls.fbank_signal(dec, good, f, p)
        for kind in ("device", "numpy"):
            for mid, exc, code in (((s["mixed/mpeg1-lsf"], mix, 0), api.MixedFormat, -3), ((bad, bix, 10), api.RingReplay, -2)):
                big, view = cg.destination(kind, 3, 1, (f, d))
                src = [(s["48k"], cg.ref("48k")[0], 100), mid, (s["22k"], cg.ref("22k")[0], 3000)]
                with pytest.raises(exc) as e:
                    dec.decode_clips_mfcc(src, f, out=view, **p)
                host = cg.host(big)
                assert e.value.valid[1] == code and (host[1] == SENT).all()
                assert (host[:, :, f * d:] == SENT).all()
                got = host[[0, 2], :, :f * d].reshape(2, 1, f, d)
                _check(good, sig, got, e.value.valid[[0, 2]], f, p)
        # bad arguments: nothing is written
        big, view = cg.destination("device", 1, 1, (f, d))
        src = [(s["48k"], cg.ref("48k")[0], 0)]
        for bad_p in (dict(cepstral_lifter=-1.0), dict(cepstral_lifter=float("nan")), dict(use_log_fbank=False), dict(win_length=1025), dict(hop=0),
                      dict(high_freq=8000.5), dict(scale=0.0), dict(width=65), dict(dither=1.0), dict(use_power=False), dict(raw_energy=False),
                      dict(snip_edges=False), dict(vtln_warp=1.1)):
            with pytest.raises(RuntimeError):
                dec.decode_clips_mfcc(src, f, out=view, **dict(p, **bad_p))
        for nc in (0, 24):
            with pytest.raises(RuntimeError):
                dec.decode_clips_mfcc(src, f, out=cg.destination("device", 1, 1, (f, nc))[1], **dict(p, num_ceps=nc))
        with pytest.raises(RuntimeError):            # (rate 0 and clips of different rates)
            dec.decode_clips_mfcc(src + [(s["32k"], cg.ref("32k")[0], 0)], f, **dict(p, sample_rate=0))
        assert (cg.host(big) == SENT).all()
    finally:
        dec.close()
        bix.close()


def test_host_destinations_with_a_guard_behind_the_last_row():
    """a dense numpy array (its rows leave the stage in one copy) and stereo rows with a guard between the channels"""
    p, f = P16, 37
    clips = [(n, s) for n in ("48k", "22k", "16k-mono") for s in calls.fbank_starts(n, p, f)[1:4]]
    k, d = len(clips), p["num_ceps"]
    dec = cg.decoder()
    try:
        sig = calls.fbank_signal(dec, clips, f, p)
        flat = np.full(k * f * d + GUARD, SENT, dtype=np.float32)
        dense = flat[:k * f * d].reshape(k, 1, f, d)
        out, valid = dec.decode_clips_mfcc(cg.src(clips), f, out=dense, **p)
        assert out is dense and (flat[k * f * d:] == SENT).all()
        print("dense numpy rows: worst error / bound %.4f" % _check(clips, sig, dense, valid, f, p))
        on_device, valid_dev = _run(dec, "device", clips, f, p)
        assert np.array_equal(dense.view(np.uint32), on_device.view(np.uint32)) and np.array_equal(valid, valid_dev)
        p2 = dict(p, channels=2, subtract_mean=True, use_energy=True)
        sig2 = calls.fbank_signal(dec, clips, f, p2)
        got, valid = _run(dec, "numpy", clips, f, p2)
        print("strided stereo numpy rows: worst error / bound %.4f" % _check(clips, sig2, got, valid, f, p2))
        got_dev, valid_dev = _run(dec, "device", clips, f, p2)
        assert np.array_equal(got.view(np.uint32), got_dev.view(np.uint32)) and np.array_equal(valid, valid_dev)
    finally:
        dec.close()


def test_one_decoder_through_mfcc_fbank_mel_audio_and_plain_clips():
    """each call's result is what a fresh decoder gives, whatever ran on the decoder before it"""
    p = dict(P16, subtract_mean=True, use_energy=True)
    two = [("48k", 700), ("22k", 9000)]
    ix = cg.ref("48k")[0]
    fresh = cg.decoder()
    try:
        plain_before = fresh.decode_range(cg.streams()["48k"], ix, 33, 50).copy()
        audio_before, av = calls.audio_run(fresh, "device", two, 6000, 16000, 1)
        mel_before, mv = calls.mel_run(fresh, "device", two, 40, cases.MEL_P16, "log10")
        fbank_before, fv = calls.fbank_run(fresh, "device", two, 40, cases.FBANK_P16)
    finally:
        fresh.close()
    fresh = cg.decoder()
    try:
        mfcc_before, cv = _run(fresh, "device", two, 40, p)
    finally:
        fresh.close()
    dec = cg.decoder()
    try:
        a, va = _run(dec, "device", two, 40, p)
        assert np.array_equal(a.view(np.uint32), mfcc_before.view(np.uint32)) and np.array_equal(va, cv)
        fbank_after, fv2 = calls.fbank_run(dec, "device", two, 40, cases.FBANK_P16)
        assert np.array_equal(fbank_before.view(np.uint32), fbank_after.view(np.uint32)) and np.array_equal(fv, fv2)
        _run(dec, "device", two, 9, dict(P16, num_ceps=17, cepstral_lifter=0.5, htk_compat=True))      # (another table on the same decoder)
        mel_after, mv2 = calls.mel_run(dec, "device", two, 40, cases.MEL_P16, "log10")
        assert np.array_equal(mel_before.view(np.uint32), mel_after.view(np.uint32)) and np.array_equal(mv, mv2)
        b, vb = _run(dec, "numpy", two, 40, p)
        assert np.array_equal(b.view(np.uint32), mfcc_before.view(np.uint32)) and np.array_equal(vb, cv)
        audio_after, av2 = calls.audio_run(dec, "device", two, 6000, 16000, 1)
        assert np.array_equal(audio_before.view(np.uint32), audio_after.view(np.uint32)) and np.array_equal(av, av2)
        plain_after = dec.decode_range(cg.streams()["48k"], ix, 33, 50)
        assert np.array_equal(plain_before, plain_after)
        c, vc = _run(dec, "device", two, 40, p)
        assert np.array_equal(c.view(np.uint32), mfcc_before.view(np.uint32)) and np.array_equal(vc, cv)
    finally:
        dec.close()


def test_made_output_and_empty_calls():
    dec = cg.decoder()
    try:
        # torchaudio's defaults: 25 ms frames every 10 ms, 23 bins, 13 cepstra, lifter 22
        src = cg.src([("32k", 1000)])
        out, valid = dec.decode_clips_mfcc(src, 50)
        assert tuple(out.shape) == (1, 1, 50, 13) and out.is_cuda and valid[0] == 50
        sig = calls.fbank_signal(dec, [("32k", 1000)], 50, P16)
        _check([("32k", 1000)], sig, cg.host(out), valid, 50, P16)
        out, valid = dec.decode_clips_mfcc([], 10)
        assert tuple(out.shape) == (0, 1, 10, 13) and valid.size == 0
        out, valid = dec.decode_clips_mfcc(src, 0)
        assert tuple(out.shape) == (1, 1, 0, 13) and valid[0] == 0
        big, view = cg.destination("numpy", 1, 1, (0, 13))
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
    pf = dict(cases.FBANK_P16, num_mel_bins=nm)
    clips = [(n, s) for n in ("48k", "8k") for s in calls.fbank_starts(n, p, f)[1:5]]
    b = ref.dct_rows(nm, nm)                           # [c, m]
    assert np.abs(b.T @ b - np.eye(nm)).max() < 1e-14
    dec = cg.decoder()
    try:
        sig = calls.fbank_signal(dec, clips, f, p)
        cep, valid = _run(dec, "device", clips, f, p)
        lg, valid_f = calls.fbank_run(dec, "device", clips, f, pf)
        assert np.array_equal(valid, valid_f)
        worst = 0.0
        for i, (n, s) in enumerate(clips):
            w = calls.fbank_filterbank(p, n)
            _, dc = _definition(sig[i][1], s, f, p, w, int(valid[i]))
            _, dl = calls.fbank_definition(sig[i][1], s, f, pf, w, int(valid[i]))
            back = cep[i].astype(np.float64) @ b
            tol = dc @ np.abs(b) + dl
            err = np.abs(back - lg[i].astype(np.float64))
            assert (err <= tol).all(), (n, s, float((err - tol).max()))
            if np.abs(sig[i][1]).sum() > 0:
                worst = max(worst, float((err / tol).max()))
        print("mfcc times B against fbank: worst difference / tolerance %.4f" % worst)
        assert 0.0 < worst <= 1.0
    finally:
        dec.close()
