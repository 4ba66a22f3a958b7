"""pYIN pitch tracking of clips on the device: decode_clips_pyin's observation mode against the definition
evaluated on decode_clips_pitch's own curve (positions, bins and the set of non-zero entries exact, values within the derived
bound, v bit for bit), its path mode against the definition's Viterbi decode of its own observation (the score within eps of the
best, the state equal wherever the max-marginal's margin exceeds 2 eps); a periodic stream that must be voiced at one bin with a
decided margin; slices, determinism, a refused clip in a batch, bad arguments, guards, empty calls."""
import functools

import numpy as np
import pytest

import clip_gpu as cg
import clip_gpu_calls as cc
import clip_pitch_ref as pref
import clip_pyin_ref as ref
import clip_streams
from clip_gpu import GUARD, SENT
from clip_streams import ISO_LSF

pytestmark = pytest.mark.gpu

SMALL = ref.args(sample_rate=16000, frame_length=256, win_length=128, hop=64, fmin=16000 / 137.5, fmax=16000 / 2.5)     # lags 2 .. 127, 694 bins
PERIODIC = ref.args(sample_rate=16000, frame_length=2048, win_length=512, hop=256, fmin=7.0, fmax=13.92)                # lags 1149 .. 1535, 120 bins


tables = cc.pyin_tables
_pitch_args, _run, _curve, _check_both = cc.pyin_pitch_args, cc.pyin_run, cc.pyin_curve, cc.pyin_check_both

CASES = {"n256-16k": (SMALL, "16k-mono"), "defaults-22k": (ref.args(), "22k")}


@pytest.mark.parametrize("f", [9, 17])
@pytest.mark.parametrize("case", sorted(CASES))
def test_both_modes_against_the_definition(case, f):
    a, name = CASES[case]
    k = ref.numbers(a)
    dec = cg.decoder()
    try:
        for channels in (1, 2):
            j_all = cg.j_all(dict(a, channels=channels), name)
            clips = [(name, s) for s in (k["N"] // 2 - 7, j_all // 3 + 11, j_all - (f // 2) * k["H"] - 3)]
            curve, valid_c = _curve(dec, clips, f, a, channels)
            obs, valid1 = _run(dec, "device", clips, f, a, channels, "observation")
            planes, valid0 = _run(dec, "device", clips, f, a, channels, "pitch")
            assert np.array_equal(valid_c, valid1) and np.array_equal(valid1, valid0) and valid0[0] == f and 0 < valid0[2] < f
            worst, most, open_frames, frames = _check_both(clips, curve, obs, planes, a, channels)
            print("%s, F %d, %d channel(s): observation worst error / bound %.3f, troughs up to %d a frame; %d of %d frames without the "
                  "margin (share %.2f)" % (case, f, channels, worst, most, open_frames, frames, open_frames / frames))
            assert worst <= 1.0 and most >= 2
            for mode, dev in (("observation", obs), ("pitch", planes)):
                host, valid2 = _run(dec, "numpy", clips, f, a, channels, mode)
                assert np.array_equal(host.view(np.uint32), dev.view(np.uint32)) and np.array_equal(valid0, valid2)
            # frames behind the stream's end: zeros, a curve of 1, no trough, unvoiced
            assert (obs[2, :, :, -1] == 0).all() and (planes[2, :, 1, -1] == 0).all() and np.isnan(planes[2, :, 0, -1]).all()
    finally:
        dec.close()


@functools.lru_cache(maxsize=None)
def _periodic():
    """one chunk of two MPEG-2 frames at 16 kHz, mono, no bit reservoir, forty times: once the first chunk's overlap has settled
    the decoded row repeats every 1152 samples exactly (the test asserts it on the product's own row)"""
    from pdmp3_amd import api
    from pdmp3_amd.packer import packer
    chunk = packer.generate(n_frames=2, seed=7, version=1, sfreq=2, mode=3, bitrate_index=6, iso_strict=True, reservoir=False)
    mp3 = b"".join([chunk] * 40)
    return mp3, api.StreamIndex(mp3, ISO_LSF)


cg.STREAMS["pyin/periodic-16k"] = _periodic


def test_a_periodic_stream_is_voiced_at_its_bin_with_a_decided_margin():
    """N 2048, W 512 at 16 kHz; the row repeats every 1152 samples (13.89 Hz), so d'(1152) is exactly 0.  The stream's curve has
    a broad valley around that lag with ripples a few hundredths deep -- troughs at 1139 and 1144 in front of it, at 1160 and
    1165 behind it.  With fmin 10.5, fmax 21 and half-semitone bins the reference's own decode (the CPU oracle's row through the
    definition) is not decided at the period's bin, and cannot be made so by fmin / fmax alone: the troughs in front take the
    Boltzmann prior's first places under every threshold above 0.03, and a half-semitone bin (34 lags) holds 1160 and 1165 too,
    whose probabilities stand in place of the period's (the larger lag stands).  A range can only start between 1145 and 1151
    and keep 1152 out of the dropped top bin n_b where the bins are narrower than that gap.  So: fmin 7, fmax 13.92 -- lags
    1149 .. 1535, the period the first trough -- and the default tenth-semitone bins, hop 256 so that the band of 71 fits the
    120 bins.  There the reference alone (on the binary64 curve of the product's row, rounded to binary32) is voiced at the
    period's bin on every frame with a margin of 2 against 2 eps = 1e-11; asserted first.  Then the device's two modes."""
    a = PERIODIC
    k, t = ref.numbers(a), tables(a)
    assert (k["tmin"], k["tmax"], k["n_b"], k["Wd"]) == (1149, 1535, 120, 71)
    want = int((1152.0 <= t["T"]).sum())
    assert want == 119 and abs(t["f0"][want] / (16000.0 / 1152.0) - 1.0) < 2.0 ** (0.5 / 120) - 1.0
    f, start = 11, 4608
    clips = [("pyin/periodic-16k", start)]
    dec = cg.decoder()
    try:
        (s0, y), = cg.signal(dec, clips, f, _pitch_args(a, 1))
        row = y[0]
        assert s0 == start - 1024 and np.abs(row).max() > 0.01
        assert np.array_equal(row[:-1152].view(np.uint32), row[1152:].view(np.uint32)), "the product's row is not periodic in 1152 samples"
        z = pref.frames(row, 0, 2048, 256, f)
        c64 = np.stack([pref.curve(z[i], 512, k["tmax"])[0] for i in range(f)], axis=1).astype(np.float32)
        o64 = np.stack([np.concatenate([o, [v]]) for o, v, _, _ in (ref.observe(c64[:, i], k["tmin"], k["tmax"], t, a["no_trough_prob"]) for i in range(f))],
                       axis=1).astype(np.float32)
        best, mm, _, _, _ = ref.decode(o64, t)
        top = np.sort(mm, axis=1)
        assert (mm.argmax(axis=1) == want).all() and (top[:, -1] - top[:, -2] > 2 * ref.epsilon(f)).all(), "the reference's own decode is not decided"
        curve, _ = _curve(dec, clips, f, a, 1)
        obs, _ = _run(dec, "device", clips, f, a, 1, "observation")
        planes, valid = _run(dec, "device", clips, f, a, 1, "pitch")
        worst, most, open_frames, frames = _check_both(clips, curve, obs, planes, a, 1)
        print("periodic stream: observation worst error / bound %.3f, troughs up to %d a frame, %d of %d frames without the margin; v %s"
              % (worst, most, open_frames, frames, planes[0, 0, 2, :4]))
        assert open_frames == 0 and valid[0] == f
        assert (planes[0, 0, 1] == 1).all() and (planes[0, 0, 3] == want).all() and (planes[0, 0, 0] == t["f0"][want]).all()
    finally:
        dec.close()


def test_observation_slices_and_determinism():
    """Mode 1 of (s, F) equals the columns of (s - a H, F + a) bit for bit: a frame's observation depends on its samples alone.
    Mode 0 is not required to, and is not asserted to: the path depends on where the clip starts.  Twice the same call gives the
    same bits in both modes, and a clip alone gives what it gives in a batch."""
    a, name, f, shift = SMALL, "16k-mono", 9, 4
    k = ref.numbers(a)
    dec = cg.decoder()
    try:
        s = 20000
        short, _ = _run(dec, "device", [(name, s)], f, a, 1, "observation")
        longer, _ = _run(dec, "device", [(name, s - shift * k["H"])], f + shift, a, 1, "observation")
        assert np.array_equal(short.view(np.uint32), longer[:, :, :, shift:].view(np.uint32)) and np.count_nonzero(short) > f
        batch = [(name, x) for x in (1000, 50000, 7, 123456, 90000)]
        for mode in ("pitch", "observation"):
            one, v1 = _run(dec, "device", batch, f, a, 2, mode)
            two, v2 = _run(dec, "device", batch, f, a, 2, mode)
            assert np.array_equal(one.view(np.uint32), two.view(np.uint32)) and np.array_equal(v1, v2)
            for i in (0, 3):
                alone, va = _run(dec, "device", [batch[i]], f, a, 2, mode)
                assert np.array_equal(alone[0].view(np.uint32), one[i].view(np.uint32)) and va[0] == v1[i]
    finally:
        dec.close()


def test_fill_and_the_bins_frequency():
    a, name, f = SMALL, "16k-mono", 9
    t = tables(a)
    clips = [(name, 30000)]
    dec = cg.decoder()
    try:
        nan, _ = _run(dec, "device", clips, f, a, 1, "pitch")
        minus, _ = _run(dec, "device", clips, f, a, 1, "pitch", fill=-1.0)
        bins, _ = _run(dec, "device", clips, f, a, 1, "pitch", fill=None)
        assert np.array_equal(nan[0, 0, 1:].view(np.uint32), minus[0, 0, 1:].view(np.uint32)) and np.array_equal(nan[0, 0, 1:], bins[0, 0, 1:])
        voiced = nan[0, 0, 1] == 1
        assert np.isnan(nan[0, 0, 0][~voiced]).all() and (minus[0, 0, 0][~voiced] == -1.0).all()
        assert np.array_equal(bins[0, 0, 0], t["f0"][bins[0, 0, 3].astype(int)]) and np.array_equal(nan[0, 0, 0][voiced], bins[0, 0, 0][voiced])
    finally:
        dec.close()


def test_a_refused_clip_in_the_middle_of_a_batch_and_bad_arguments():
    from pdmp3_amd import api
    a, f = SMALL, 9
    bad = clip_streams.replay_stream()
    bix = api.StreamIndex(bad, ISO_LSF)
    assert bix.replay
    mix = cg.ref("mixed/mpeg1-lsf")[0]
    assert not mix.one_format
    s = cg.streams()
    good = [("48k", 100), ("22k", 3000)]
    dec = cg.decoder()
    try:
        want_p, _ = _run(dec, "device", good, f, a, 1, "pitch")
        want_o, valid = _run(dec, "device", good, f, a, 1, "observation")
        for kind, mode, want in (("device", "pitch", want_p), ("numpy", "observation", want_o)):
            rows = want.shape[2]
            for mid, exc, code in (((s["mixed/mpeg1-lsf"], mix, 0), api.MixedFormat, -3), ((bad, bix, 10), api.RingReplay, -2)):
                big, view = cg.destination(kind, 3, 1, (rows, f))
                src = [cg.source("48k") + (100,), mid, cg.source("22k") + (3000,)]
                with pytest.raises(exc) as e:
                    dec.decode_clips_pyin(src, f, out_mode=mode, out=view, channels=1, **a)
                host = cg.host(big).reshape(3, 1, rows * f + GUARD)
                assert e.value.valid[1] == code and (host[1] == SENT).all() and (host[:, :, rows * f:] == SENT).all()
                got = host[[0, 2], :, :rows * f].reshape(2, 1, rows, f)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and np.array_equal(e.value.valid[[0, 2]], valid)
        # bad arguments: nothing is written
        src = [cg.source("48k") + (0,)]
        for mode, rows in (("pitch", 4), ("observation", ref.numbers(a)["n_b"] + 1)):
            big, view = cg.destination("device", 1, 1, (rows, f))
            for bad_a in (dict(frame_length=255), dict(win_length=3), dict(hop=257), dict(fmin=0.0), dict(fmax=8000.5), dict(n_thresholds=0),
                          dict(n_thresholds=257), dict(boltzmann=0.0), dict(switch_prob=0.0), dict(switch_prob=1.0), dict(no_trough_prob=0.0),
                          dict(no_trough_prob=1.0), dict(beta=(2.5, 18)), dict(max_transition_rate=4000.0), dict(threshold_weights=[0.5] * 7),
                          dict(width=65)):
                with pytest.raises(RuntimeError):
                    dec.decode_clips_pyin(src, f, out_mode=mode, out=view, channels=1, **dict(a, **bad_a))
                assert (cg.host(big) == SENT).all(), bad_a
            for bad_mode in ("curve", 2, -1):
                with pytest.raises(RuntimeError):
                    dec.decode_clips_pyin(src, f, out_mode=bad_mode, out=view, channels=1, **a)
            with pytest.raises(RuntimeError):
                dec.decode_clips_pyin([cg.source("48k") + (-1,)], f, out_mode=mode, out=view, channels=1, **a)
            assert (cg.host(big) == SENT).all()
    finally:
        dec.close()
        bix.close()


def test_return_types_defaults_and_empty_calls():
    import torch
    from pdmp3_amd import api
    src = [cg.source("22k") + (30000,)]
    dec = cg.decoder()
    try:
        out, valid = dec.decode_clips_pyin(src, 20)
        assert tuple(out.shape) == (1, 2, 4, 20) and out.is_cuda and out.dtype == torch.float32 and valid[0] == 20 and valid.dtype == np.int64
        plain, _ = _run(dec, "device", [("22k", 30000)], 20, ref.args(), 2, "pitch")       # (the defaults, spelled out)
        assert np.array_equal(cg.host(out).view(np.uint32), plain.view(np.uint32))
        b = cg.host(out)[0, :, 3]
        assert ((b >= 0) & (b <= 600)).all() and np.isin(cg.host(out)[0, :, 1], (0.0, 1.0)).all()
        out, valid = dec.decode_clips_pyin(src, 20, out_mode="observation", channels=1)
        assert tuple(out.shape) == (1, 1, 602, 20) and api.pyin_plan(22050)["n_bins"] == 601
        out, valid = dec.decode_clips_pyin([], 10)
        assert tuple(out.shape) == (0, 1, 4, 10) and valid.size == 0
        out, valid = dec.decode_clips_pyin(src, 0)
        assert tuple(out.shape) == (1, 2, 4, 0) and valid[0] == 0
        out, valid = dec.decode_clips_pyin(src, 0, out_mode="observation")
        assert tuple(out.shape) == (1, 2, 602, 0) and valid[0] == 0
    finally:
        dec.close()
