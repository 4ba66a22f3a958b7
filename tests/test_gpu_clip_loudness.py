"""The loudness of clips on the GPU (include/pdmp3_bulk.h pdmp3_amd_bulk_decode_clips_loudness, csrc/loudness.hip; DESIGN.md
section 18).

The reference is made from the product's own signal, as in the other feature tests: decode_clips_audio gives the binary32
samples of a clip's row, tests/clip_loudness_ref.py measures them in binary64 by a plain sample loop and evaluates the bound of
the device's blocked binary32 product from its own quantities.  Every field of stats and every momentary value has to lie within
its bound; the counts, J and the sample peak are exact; the audio is the audio call's row times the g of stats, bit for bit.  A
clip whose gates the bound cannot decide is held to M, P, J, the momentary curve and the audio alone, and at most one clip in
ten of a test may be such.  Destinations are filled with a sentinel first: nothing outside a row's floats may change."""
import functools

import numpy as np
import pytest

import clip_gpu as cg
import clip_loudness_ref as ref
import clip_streams
from clip_gpu import GUARD, SENT
from clip_gpu_calls import LOUDNESS_CASES as CASES, audio_rows as _signal, loud_rate as _fs, loudness_check as _check, loudness_run as _run
from clip_streams import ISO_LSF

pytestmark = pytest.mark.gpu
BIG = 5 * ref.B * ref.CHUNK + ref.B + 5            # five scan chunks, a block and five samples: J >= 1 at every rate used


@functools.lru_cache(maxsize=None)
def _gate_stream():
    """a loud part and a quiet part end to end: both gates bite (J = 54, |A| = 52, |Gt| = 24, L = -10.96 with the CPU oracle)"""
    from pdmp3_amd import api
    from pdmp3_amd.packer import packer
    mp3 = packer.generate(n_frames=120, seed=11, sfreq=1, mode=0, bitrate_index=10, gain=(150, 150)) + \
        packer.generate(n_frames=120, seed=12, sfreq=1, mode=0, bitrate_index=10, gain=(130, 130))
    return mp3, api.StreamIndex(mp3, ISO_LSF)


cg.STREAMS["gate"] = _gate_stream


@pytest.mark.parametrize("case", sorted(CASES))
def test_against_binary64(case):
    """1.5 s and a length of five chunks, a block and five samples; starts 0, mid-stream and with the stream's end inside the
    clip; device and numpy destinations -- the reference of a length made once for both"""
    names, rate, channels = CASES[case]
    dec = cg.decoder()
    try:
        fs = _fs([(names[0], 0)], rate)
        for t in (fs * 3 // 2, BIG):
            clips = []
            for n in names:
                ix = cg.source(n)[1]
                j_all = ix.samples * fs // ix.rate
                clips += [(n, 0), (n, j_all // 2 + 331), (n, j_all - t // 3)]
            x, valid = _signal(dec, clips, t, rate, channels, channels)
            got = _run(dec, "device", clips, t, rate, channels)
            refs, worst, _, _ = _check(x, valid, got, fs)
            assert 0.0 < worst <= 1.0 and refs[0].J >= 1 and any(np.isfinite(m.L) for m in refs)
            host = _run(dec, "numpy", clips, t, rate, channels)
            for a, b in zip(got, host):
                assert np.array_equal(np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype),
                                      np.ascontiguousarray(b).view(np.uint32 if b.dtype == np.float32 else b.dtype))
    finally:
        dec.close()


@functools.lru_cache(maxsize=None)
def _gate_case():
    """the whole gate stream at its own rate: (t, the audio call's rows, valid) -- made once"""
    dec = cg.decoder()
    try:
        ix = _gate_stream()[1]
        t = int(ix.samples)
        x, valid = _signal(dec, [("gate", 0)], t, 0, 0, 2)
        return t, x, valid
    finally:
        dec.close()


def test_both_gates_bite():
    t, x, valid = _gate_case()
    dec = cg.decoder()
    try:
        got = _run(dec, "device", [("gate", 0)], t, c=2)
        refs, worst, margin, undecided = _check(x, valid, got, 48000)
        m = refs[0]
        assert m.nGt < m.nA < m.J and not undecided and margin > 1.0, (m.J, m.nA, m.nGt, margin)
        assert m.J == 54
        print("J %d, |A| %d, |Gt| %d, L %.2f" % (m.J, m.nA, m.nGt, m.L))
        assert 0.0 < worst <= 1.0
    finally:
        dec.close()


def test_no_target_is_the_audio_call_and_the_gain_is_in_stats():
    fs = 48000
    t = fs * 3 // 2
    clips = [("gate", 0), ("48k", 0), ("48k", 8 * fs)]       # (the last one: behind the stream's end)
    dec = cg.decoder()
    try:
        x, valid = _signal(dec, clips, t, 0, 0, 2)
        audio, stats, mom, v = _run(dec, "device", clips, t, c=2)
        assert np.array_equal(audio.view(np.uint32), x.view(np.uint32)) and (stats[:, 3] == 1.0).all() and np.array_equal(v, valid)
        assert (stats[2] == np.array([-np.inf, -np.inf, 0, 1, -np.inf, 12, 0, 0], dtype=np.float32)).all()
        assert (audio[2] == 0).all() and not np.signbit(audio[2]).any() and (mom[2] == -np.inf).all()
        for kind in ("device", "numpy"):
            got = _run(dec, kind, clips, t, c=2, target=-14.0, peak_limit=0.9)
            refs, _, _, undecided = _check(x, valid, got, fs, target=-14.0, peak_limit=0.9)
            assert not undecided and [m.limited for m in refs] == [False, True, False], [(m.g, m.P) for m in refs]
            assert got[1][0, 3] != 1.0 and got[1][1, 3] == np.float32(0.9 / refs[1].P) and got[1][2, 3] == 1.0
    finally:
        dec.close()


def test_order_and_batch_independence():
    fs, q = 32000, 3200
    t = 9 * q + 77
    clips = [("32k", 4321), ("48k", 100), ("32k", 150000)]
    dec = cg.decoder()
    try:
        one = _run(dec, "device", clips, t, fs, 2, target=-20.0)
        two = _run(dec, "device", clips, t, fs, 2, target=-20.0)
        for a, b in zip(one, two):
            assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
        alone = _run(dec, "device", [clips[2]], t, fs, 2, target=-20.0)
        for a, b in zip(one[:3], alone[:3]):
            assert np.array_equal(a[2].view(np.uint32), b[0].view(np.uint32)), "a clip's numbers depend on its batch"
        # block j of a clip and block 0 of the clip of four sub-blocks that begins j q later: the filter's history differs, so
        # the two agree as far as their references do -- bounded, and not required to be bit-equal
        j = 3
        short = [(clips[0][0], clips[0][1] + j * q)]
        xs, vs = _signal(dec, short, 4 * q, fs, 2, 2)
        xl, vl = _signal(dec, clips[:1], t, fs, 2, 2)
        got = _run(dec, "device", short, 4 * q, fs, 2)
        ms, ml = ref.measure(xs[0], fs), ref.measure(xl[0], fs)
        ref.check_stats(ms, got[1][0], got[2][0])
        assert ms.J == 1 and np.isfinite(ms.l[0])
        apart = abs(float(got[2][0, 0]) - float(one[2][0, j]))
        assert apart <= abs(ms.l[0] - ml.l[j]) + ms.dl[0] + ml.dl[j] + 1e-5
        print("block %d of the long clip and block 0 of the short one: %.3g dB apart (references: %.3g dB)" % (j, apart, abs(ms.l[0] - ml.l[j])))
    finally:
        dec.close()


def test_behind_the_end_refusals_and_a_refused_clip_in_the_middle_of_a_batch():
    from pdmp3_amd import api
    fs, t = 48000, 6 * 4800 + 11
    J = ref.plan(fs, t)["J"]
    bad = clip_streams.replay_stream()
    bix = api.StreamIndex(bad, ISO_LSF)
    assert bix.replay
    mix = cg.ref("mixed/mpeg1-lsf")[0]
    assert not mix.one_format
    s = cg.streams()
    good = [("48k", 100), ("48k", 30000)]
    dec = cg.decoder()
    try:
        x, valid = _signal(dec, good, t, fs, 2, 2)
        for kind in ("device", "numpy"):
            for mid, exc, code in (((s["mixed/mpeg1-lsf"], mix, 0), api.MixedFormat, -3), ((bad, bix, 10), api.RingReplay, -2)):
                big, view = cg.destination(kind, 3, 2, (t,))
                mom = np.full((3, J), SENT, dtype=np.float32)
                if kind == "device":
                    import torch
                    mom = torch.full((3, J), float(SENT), dtype=torch.float32, device="cuda")
                src = [cg.src(good)[0], mid, cg.src(good)[1]]
                c0, h0 = dec.clip_stats()
                with pytest.raises(exc) as e:
                    dec.decode_clips_loudness(src, t, fs, 2, target=-23.0, out=view, momentary=mom)
                host, m, st = cg.host(big), cg.host(mom), np.array(cg.host(e.value.stats))
                assert e.value.valid[1] == code and (host[1] == SENT).all() and (m[1] == SENT).all() and np.isnan(st[1]).all()
                assert (host[:, :, t:] == SENT).all()
                got = (host[[0, 2], :, :t], st[[0, 2]], m[[0, 2]], e.value.valid[[0, 2]])
                _, worst, _, _ = _check(x, valid, got, fs, target=-23.0)
                assert 0.0 < worst <= 1.0
                c1, h1 = dec.clip_stats()
                assert c1 > c0 and h1 >= h0
        # the counts are the audio call's for the same clips
        c0, h0 = dec.clip_stats()
        _signal(dec, good, t, fs, 2, 2)
        c1, h1 = dec.clip_stats()
        _run(dec, "device", good, t, fs, 2)
        c2, h2 = dec.clip_stats()
        assert (c2 - c1, h2 - h1) == (c1 - c0, h1 - h0)
        # bad arguments: nothing is written
        big, view = cg.destination("device", 1, 2, (t,))
        src = cg.src(good[:1])
        for kw in (dict(target=-70.5), dict(target=0.5), dict(target=float("inf")), dict(peak_limit=-1.0), dict(peak_limit=float("inf")),
                   dict(peak_limit=float("nan")), dict(dual_mono=True), dict(dual_mono=2), dict(width=65), dict(sample_rate=7999),
                   dict(sample_rate=192001)):
            with pytest.raises(RuntimeError):
                dec.decode_clips_loudness(src, t, **dict(dict(sample_rate=fs, channels=2, out=view), **kw))
            assert (cg.host(big) == SENT).all(), kw
        with pytest.raises(RuntimeError):
            dec.decode_clips_loudness([(s["48k"], cg.ref("48k")[0], -1)], t, fs, 2, out=view)
        with pytest.raises(RuntimeError):            # (rate 0 and clips of different rates)
            dec.decode_clips_loudness(src + cg.src([("32k", 0)]), t)
        assert (cg.host(big) == SENT).all()
        # dual mono on a mono call: + 3.01 dB
        xm, vm = _signal(dec, good[:1], t, fs, 1, 1)
        got = _run(dec, "device", good[:1], t, fs, 1, dual_mono=True)
        refs, _, _, _ = _check(xm, vm, got, fs, dual_mono=True)
        plain = _run(dec, "device", good[:1], t, fs, 1)
        assert abs(float(got[1][0, 0]) - float(plain[1][0, 0]) - 10.0 * np.log10(2.0)) <= 2.0 * refs[0].dL + 1e-5
    finally:
        dec.close()
        bix.close()


def test_more_clips_than_one_grid():
    """32 768 + 5 clips of one block's sub-blocks in one call: pdmp3_hip_clip_loudness launches its kernels twice (a grid's y
    extent), the second time from descriptor 32 768 on.  Sixty-four distinct clips are held against the definition, every row is
    bit-equal to its twin among them; the last five are other clips than rows 0 .. 4, one of them behind the end"""
    name, k, t = "8k", 32768 + 5, 3200
    mp3, ix = cg.source(name)
    assert ix.rate == 8000
    j_all = int(ix.samples)
    starts = [1000 + 3001 * i for i in range(62)] + [j_all + 9, j_all - 5]
    assert starts[61] + t < j_all
    twin = (np.arange(k, dtype=np.int64) * 7) % 62
    twin[32768:] = [62, 63, 61, 60, 59]
    dec = cg.decoder()
    try:
        first = [(name, s) for s in starts]
        x, valid64 = _signal(dec, first, t, 0, 1, 1)
        base = _run(dec, "device", first, t, 0, 1, target=-16.0)
        _, worst, _, _ = _check(x, valid64, base, 8000, target=-16.0)
        assert 0.0 < worst <= 1.0 and list(valid64[61:]) == [t, 0, 5]
        import torch
        out = torch.full((k, 1, t + GUARD), float(SENT), dtype=torch.float32, device="cuda")
        mom = torch.full((k + 1, 1), float(SENT), dtype=torch.float32, device="cuda")
        audio, stats, valid = dec.decode_clips_loudness([(mp3, ix, int(starts[i])) for i in twin], t, 0, 1, target=-16.0, out=out[:, :, :t], momentary=mom)
        torch.cuda.synchronize()
        assert np.array_equal(valid, valid64[twin]) and list(valid[32768:]) == [0, 5, t, t, t]
        assert bool((out[:, :, t:] == float(SENT)).all()) and bool((mom[k] == float(SENT)).all())
        tw = torch.from_numpy(twin).cuda()
        for got, want in ((out[:, 0, :t], base[0][:, 0]), (stats, base[1]), (mom[:k], base[2])):
            w = torch.from_numpy(np.ascontiguousarray(want)).cuda()[tw]
            same = (got.contiguous().view(torch.int32) == w.contiguous().view(torch.int32)).all(dim=1)
            bad = torch.nonzero(~same).flatten().cpu().numpy()
            assert bad.size == 0, "%d rows differ from their twins, %d of them in the second launch: %s" % (bad.size, int((bad >= 32768).sum()), bad[:8].tolist())
        assert np.unique(base[1][:62, 0]).size > 8
    finally:
        dec.close()


def test_return_types_defaults_and_empty_calls():
    import torch
    src = cg.src([("48k", 1000)])
    dec = cg.decoder()
    try:
        audio, stats, valid = dec.decode_clips_loudness(src, 30000)          # the stream's rate and channels, no target, no momentary
        assert tuple(audio.shape) == (1, 2, 30000) and audio.is_cuda and audio.dtype == torch.float32 and valid[0] == 30000
        assert tuple(stats.shape) == (1, 8) and stats.is_cuda and stats.dtype == torch.float32 and float(stats[0, 3]) == 1.0
        plain, _ = dec.decode_clips_audio(src, 30000)
        assert torch.equal(audio.view(torch.int32), plain.view(torch.int32))
        got = _run(dec, "numpy", [("48k", 1000)], 30000, c=2)
        assert np.array_equal(got[1].view(np.uint32), cg.host(stats).view(np.uint32)) and got[1][0, 5] == 3
        audio, stats, valid = dec.decode_clips_loudness([], 10, channels=1)
        assert tuple(audio.shape) == (0, 1, 10) and tuple(stats.shape) == (0, 8) and valid.size == 0
        audio, stats, valid = dec.decode_clips_loudness(src, 0, channels=1)
        assert tuple(audio.shape) == (1, 1, 0) and valid[0] == 0 and bool(torch.isnan(stats).all())
    finally:
        dec.close()
