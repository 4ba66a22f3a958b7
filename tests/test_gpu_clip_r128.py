"""True peak, short-term loudness and loudness range of clips on the GPU (include/pdmp3_bulk.h pdmp3_amd_bulk_decode_clips_r128,
csrc/loudness.hip k_loud_blocks<true> / k_loud_gate<true>).

The reference is made from the product's own signal, as in tests/test_gpu_clip_loudness.py: decode_clips_audio gives the
binary32 samples of a clip's row, tests/clip_r128_ref.py evaluates the definition in binary64 and the derived bounds from its
own quantities.  Every field of stats, every momentary and short-term value has to lie within its bound; the counts, Js, Jr and
the sample peak are exact, TP >= P exactly; the audio is the audio call's row times the g of stats, bit for bit.  A clip whose
gates the bounds cannot decide is held to what does not depend on them, and at most one clip in ten of a test may be such.
Destinations are filled with a sentinel first: nothing outside a row's floats may change."""
import functools

import numpy as np
import pytest

import clip_gpu as cg
import clip_gpu_calls as calls
import clip_r128_ref as ref
import clip_streams
from clip_gpu import GUARD, SENT
from clip_gpu_calls import LOUDNESS_CASES as CASES, audio_rows as _signal, loud_rate as _fs, r128_check as _check, r128_run as _run
from clip_streams import ISO_LSF

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _range_stream():
    """four segments of MPEG-2.5 stereo at 8 kHz end to end, global_gain 152 / 146 / 128 / 90: 158 976 samples (19.9 s).  With
    the CPU oracle's PCM: Js = 169, Jr = 17, |Ar| = 15 (the last two windows lie under -70), |Gr| = 12 (three more under
    Gamma_r = -31.60), LRA = 9.10, Smax = -7.19, TP = 1.59 over P = 1.00; the window of the range nearest to a gate is 2.65 dB =
    14 600 bounds away from it"""
    from pdmp3_amd import api
    from pdmp3_amd.packer import packer
    mp3 = b"".join(packer.generate(n_frames=n, seed=s, version=2, sfreq=2, mode=0, bitrate_index=6, iso_strict=True, gain=(g, g))
                   for n, s, g in ((84, 31, 152), (70, 32, 146), (62, 33, 128), (62, 34, 90)))
    return mp3, api.StreamIndex(mp3, ISO_LSF)


cg.STREAMS["range"] = _range_stream


def _case_clips(names, fs, t):
    clips = []
    for n in names:
        ix = cg.source(n)[1]
        j_all = ix.samples * fs // ix.rate
        clips += [(n, 0), (n, j_all // 2 + 331), (n, j_all - t // 3)]
    return clips


def _lengths(fs):
    return (30 * ((fs + 5) // 10), 14 * fs + 64 + 5)


@pytest.mark.parametrize("case", sorted(CASES))
def test_against_binary64(case):
    """3 s (the first length with a short-term window) and 14 s, a block and five samples; starts 0, mid-stream and with the
    stream's end inside the clip; device and numpy destinations -- the reference of a length made once for both"""
    names, rate, channels = CASES[case]
    dec = cg.decoder()
    try:
        fs = _fs([(names[0], 0)], rate)
        for t in _lengths(fs):
            clips = _case_clips(names, fs, t)
            x, valid = _signal(dec, clips, t, rate, channels, channels)
            got = _run(dec, "device", clips, t, rate, channels)
            refs, worst, _, _ = _check(x, valid, got, fs, target=-23.0, peak_limit=10 ** (-1 / 20))
            assert 0.0 < worst <= 1.0 and refs[0].Js >= 1 and any(np.isfinite(m.Smax) for m in refs) and any(m.TP > m.P for m in refs)
            host = _run(dec, "numpy", clips, t, rate, channels)
            for a, b in zip(got, host):
                assert np.array_equal(cg.bits(a), cg.bits(b))
    finally:
        dec.close()


@pytest.mark.parametrize("case", sorted(CASES))
def test_without_the_limit_the_first_eight_are_the_loudness_calls(case):
    names, rate, channels = CASES[case]
    dec = cg.decoder()
    try:
        fs = _fs([(names[0], 0)], rate)
        for t in _lengths(fs):
            clips = _case_clips(names, fs, t)
            for kw in (dict(target=None, peak_limit=0.0), dict(target=-14.0, peak_limit=0.5)):
                audio, stats, mom, st, valid = _run(dec, "device", clips, t, rate, channels, limit_true_peak=False, **kw)
                want = calls.loudness_run(dec, "device", clips, t, rate, channels, **kw)
                assert np.array_equal(cg.bits(audio), cg.bits(want[0])) and np.array_equal(cg.bits(stats[:, :8]), cg.bits(want[1]))
                assert np.array_equal(cg.bits(mom), cg.bits(want[2])) and np.array_equal(valid, want[3])
            assert (stats[:, 3] != 1.0).any()
    finally:
        dec.close()


@functools.lru_cache(maxsize=None)
def _range_case():
    """the whole range stream at its own rate: (t, the audio call's rows, valid) -- made once"""
    dec = cg.decoder()
    try:
        t = int(_range_stream()[1].samples)
        x, valid = _signal(dec, [("range", 0)], t, 0, 0, 2)
        return t, x, valid
    finally:
        dec.close()


def test_both_gates_of_the_range_bite():
    t, x, valid = _range_case()
    assert _range_stream()[1].rate == 8000 and t == 158976
    dec = cg.decoder()
    try:
        got = _run(dec, "device", [("range", 0)], t, c=2)
        refs, worst, margin, undecided = _check(x, valid, got, 8000, target=-23.0, peak_limit=10 ** (-1 / 20))
        m = refs[0]
        print("Js %d, Jr %d, |Ar| %d, |Gr| %d, LRA %.2f, Gamma_r %.2f, Smax %.2f, TP %.3f, P %.3f, margin %.3g dB" %
              (m.Js, m.Jr, m.nAr, m.nGr, m.LRA, m.gamma_r, m.Smax, m.TP, m.P, m.r_margin))
        assert m.Jr == 17 and m.nGr < m.nAr < m.Jr and m.LRA > 3.0 and not undecided and margin >= 10.0, (m.Jr, m.nAr, m.nGr, m.LRA, margin)
        assert 0.0 < worst <= 1.0
    finally:
        dec.close()


def test_the_history_across_waves_and_chunks():
    """the largest interpolated value of a stretch of the stream, put d samples behind the start of a wave's 1024 samples and of a
    chunk's 4096 by where the clips begin: the interpolator needs the 11 - d samples in front of the boundary from another wave
    or another chunk.  The inputs are held to two conditions first -- the reference's largest value lies where it was meant
    to, and forgetting the history at the boundary would move TP by more than four bounds for at least one clip"""
    name, fs = "48k", 48000
    offs = [b + d for b in (1024, 3072, 4096) for d in (0, 5, 11)]
    t = max(offs) + 64 + 6
    assert t % 4
    dec = cg.decoder()
    try:
        n_all = int(cg.source(name)[1].samples)
        whole, _ = _signal(dec, [(name, 0)], n_all, 0, 0, 2)
        y = np.abs(ref.oversample(whole[0])[0][:, :, 1:]).max(axis=(0, 2))       # per sample, phases 1 .. 3, both channels
        p = None
        for cand in np.argsort(-y):
            lo, hi = int(cand) - max(offs), int(cand) - min(offs) + t
            if lo >= 0 and hi <= n_all and y[lo:hi].max() == y[cand] and y[cand] > 1.005 * np.abs(whole[0][:, lo:hi]).max():      # (thousands of bounds over the sample peak)
                p = int(cand)
                break
        assert p is not None
        clips = [(name, p - o) for o in offs]
        x, valid = _signal(dec, clips, t, 0, 0, 2)
        moved = 0
        for i, o in enumerate(offs):
            tp, dtp, at = ref.true_peak(x[i])
            assert at[1] == o and at[2] != 0, (o, at)
            cut = max(ref.true_peak(x[i], cuts=(o - o % 1024,))[0], float(np.abs(x[i]).max()))
            moved += tp - cut > 4.0 * dtp
        assert moved >= 1
        print("history: the peak at sample %d of the stream, %d of %d clips lose more than four bounds without it" % (p, moved, len(offs)))
        got = _run(dec, "device", clips, t, c=2)
        _, worst, _, _ = _check(x, valid, got, fs, target=-23.0, peak_limit=10 ** (-1 / 20))
        assert 0.0 < worst <= 1.0
    finally:
        dec.close()


def test_the_gain_is_held_to_the_true_peak():
    t, x, valid = _range_case()
    m0 = ref.measure(x[0], 8000, target=-20.0)
    assert m0.TP > 1.05 * m0.P and not m0.tp_limited
    between, above = m0.g * (m0.P * m0.TP) ** 0.5, m0.g * m0.TP * 1.2
    dec = cg.decoder()
    try:
        got = _run(dec, "device", [("range", 0)], t, c=2, curves=False, target=-20.0, peak_limit=between)
        refs, _, _, undecided = _check(x, valid, got, 8000, curves=False, target=-20.0, peak_limit=between)
        big, view = cg.destination("device", 1, 2, (t,))
        plain = float(dec.decode_clips_loudness(cg.src([("range", 0)]), t, target=-20.0, peak_limit=between, out=view)[1][0, 3])
        g, tp = float(got[1][0, 3]), float(got[1][0, 8])
        assert refs[0].tp_limited and not undecided and g < plain and abs(plain - m0.g) <= m0.dg + 2.0 ** -23 * m0.g      # (the sample peak holds nothing)
        assert g * tp <= between * (1.0 + 2.0 ** -22) + g * refs[0].dTP
        got = _run(dec, "device", [("range", 0)], t, c=2, curves=False, target=-20.0, peak_limit=above)
        refs, _, _, undecided = _check(x, valid, got, 8000, curves=False, target=-20.0, peak_limit=above)
        assert not refs[0].tp_limited and not undecided and abs(float(got[1][0, 3]) - m0.g) <= m0.dg + 2.0 ** -23 * m0.g
    finally:
        dec.close()


def test_order_and_batch_independence():
    fs, q = 32000, 3200
    t = 41 * q + 77
    clips = [("32k", 4321), ("48k", 100), ("32k", 150000)]
    dec = cg.decoder()
    try:
        one = _run(dec, "device", clips, t, fs, 2)
        two = _run(dec, "device", clips, t, fs, 2)
        for a, b in zip(one, two):
            assert np.array_equal(cg.bits(a), cg.bits(b))
        alone = _run(dec, "device", [clips[2]], t, fs, 2)
        for a, b in zip(one[:4], alone[:4]):
            assert np.array_equal(cg.bits(a[2]), cg.bits(b[0])), "a clip's numbers depend on its batch"
        assert np.isfinite(one[1][:, 9]).all() and (one[1][:, 12] == 12).all() and (one[1][:, 13] == 2).all()
    finally:
        dec.close()


def test_a_refused_clip_in_the_middle_of_a_batch_and_bad_arguments():
    from pdmp3_amd import api
    fs, t = 48000, 31 * 4800 + 11
    p = ref.plan(fs, t)
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
                mom, st = cg.filled(kind, (3, p["J"])), cg.filled(kind, (3, p["Jsmax"]))
                src = [cg.src(good)[0], mid, cg.src(good)[1]]
                c0, h0 = dec.clip_stats()
                with pytest.raises(exc) as e:
                    dec.decode_clips_r128(src, t, fs, 2, out=view, momentary=mom, short_term=st)
                host, m, sh, stt = cg.host(big), cg.host(mom), cg.host(st), np.array(cg.host(e.value.stats))
                assert e.value.valid[1] == code and (host[1] == SENT).all() and (m[1] == SENT).all() and (sh[1] == SENT).all() and np.isnan(stt[1]).all()
                assert (host[:, :, t:] == SENT).all() and stt.shape == (3, 16)
                got = (host[[0, 2], :, :t], stt[[0, 2]], m[[0, 2]], sh[[0, 2]], e.value.valid[[0, 2]])
                _, worst, _, _ = _check(x, valid, got, fs, target=-23.0, peak_limit=10 ** (-1 / 20))
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
                   dict(peak_limit=float("nan")), dict(dual_mono=True), dict(dual_mono=2), dict(limit_true_peak=2), dict(limit_true_peak=-1),
                   dict(width=65), dict(sample_rate=7999), dict(sample_rate=192001)):
            with pytest.raises(RuntimeError):
                dec.decode_clips_r128(src, t, **dict(dict(sample_rate=fs, channels=2, out=view), **kw))
            assert (cg.host(big) == SENT).all(), kw
        with pytest.raises(RuntimeError):
            dec.decode_clips_r128([(s["48k"], cg.ref("48k")[0], -1)], t, fs, 2, out=view)
        with pytest.raises(RuntimeError):            # (rate 0 and clips of different rates)
            dec.decode_clips_r128(src + cg.src([("32k", 0)]), t)
        assert (cg.host(big) == SENT).all()
        # a clip wholly behind the end
        got = _run(dec, "device", [("48k", 8 * fs)], t, fs, 2)
        want = [-np.inf, -np.inf, 0, 1, -np.inf, p["J"], 0, 0, 0, -np.inf, 0, -np.inf, p["Js"], p["Jr"], 0, 0]
        assert (got[1][0] == np.array(want, dtype=np.float32)).all() and (got[0] == 0).all() and (got[3] == -np.inf).all() and got[4][0] == 0
    finally:
        dec.close()
        bix.close()


def test_more_clips_than_one_grid():
    """32 768 + 5 clips of 0.4 s in one call: pdmp3_hip_clip_r128 launches its kernels twice (a grid's y extent), the second time
    from descriptor 32 768 on.  Sixty-four distinct clips are held against the definition, every row is bit-equal to its twin
    among them; the last five are other clips than rows 0 .. 4, one of them behind the end"""
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
        base = _run(dec, "device", first, t, 0, 1)
        _, worst, _, _ = _check(x, valid64, base, 8000, target=-23.0, peak_limit=10 ** (-1 / 20))
        assert 0.0 < worst <= 1.0 and list(valid64[61:]) == [t, 0, 5] and base[2].shape == (64, 1) and base[3].shape == (64, 0)
        import torch
        out = torch.full((k, 1, t + GUARD), float(SENT), dtype=torch.float32, device="cuda")
        mom = torch.full((k + 1, 1), float(SENT), dtype=torch.float32, device="cuda")
        audio, stats, valid = dec.decode_clips_r128([(mp3, ix, int(starts[i])) for i in twin], t, 0, 1, out=out[:, :, :t], momentary=mom)
        torch.cuda.synchronize()
        assert np.array_equal(valid, valid64[twin]) and list(valid[32768:]) == [0, 5, t, t, t]
        assert bool((out[:, :, t:] == float(SENT)).all()) and bool((mom[k] == float(SENT)).all())
        tw = torch.from_numpy(twin).cuda()
        for got, want in ((out[:, 0, :t], base[0][:, 0]), (stats, base[1]), (mom[:k], base[2])):
            w = torch.from_numpy(np.ascontiguousarray(want)).cuda()[tw]
            same = (got.contiguous().view(torch.int32) == w.contiguous().view(torch.int32)).all(dim=1)
            bad = torch.nonzero(~same).flatten().cpu().numpy()
            assert bad.size == 0, "%d rows differ from their twins, %d of them in the second launch: %s" % (bad.size, int((bad >= 32768).sum()), bad[:8].tolist())
        assert np.unique(base[1][:62, 8]).size > 8
    finally:
        dec.close()


def test_return_types_defaults_and_empty_calls():
    import torch
    src = cg.src([("48k", 1000)])
    dec = cg.decoder()
    try:
        c0, _ = dec.clip_stats()
        audio, stats, valid = dec.decode_clips_r128(src, 30000)             # the stream's rate and channels, R128's target and limit, no curves
        assert dec.clip_stats()[0] > c0
        assert tuple(audio.shape) == (1, 2, 30000) and audio.is_cuda and audio.dtype == torch.float32 and valid[0] == 30000
        assert tuple(stats.shape) == (1, 16) and stats.is_cuda and stats.dtype == torch.float32
        same = dec.decode_clips_r128(src, 30000, target=-23.0, peak_limit=10 ** (-1 / 20), limit_true_peak=True)
        assert torch.equal(stats.view(torch.int32), same[1].view(torch.int32)) and torch.equal(audio.view(torch.int32), same[0].view(torch.int32))
        g, tp = float(stats[0, 3]), float(stats[0, 8])
        assert g != 1.0 and g * tp <= 10 ** (-1 / 20) * (1.0 + 2.0 ** -22) and float(stats[0, 12]) == 0 and float(stats[0, 9]) == -np.inf
        audio, stats, valid = dec.decode_clips_r128(src, 30000, target=None)
        plain, _ = dec.decode_clips_audio(src, 30000)
        assert torch.equal(audio.view(torch.int32), plain.view(torch.int32)) and float(stats[0, 3]) == 1.0
        got = _run(dec, "numpy", [("48k", 1000)], 30000, c=2, target=None)
        assert np.array_equal(got[1].view(np.uint32), cg.host(stats).view(np.uint32)) and got[1][0, 5] == 3
        audio, stats, valid = dec.decode_clips_r128([], 10, channels=1)
        assert tuple(audio.shape) == (0, 1, 10) and tuple(stats.shape) == (0, 16) and valid.size == 0
        audio, stats, valid = dec.decode_clips_r128(src, 0, channels=1)
        assert tuple(audio.shape) == (1, 1, 0) and valid[0] == 0 and bool(torch.isnan(stats).all())
    finally:
        dec.close()
