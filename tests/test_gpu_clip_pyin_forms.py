"""Every launch form of pYIN's two kernels on the device, each named by the plan the test asserts:
k_clip_pyin_path_big (more states than a dynamic LDS request holds), two bins a thread (n_b > 1024), 4 and 2 frames a workgroup
of k_clip_pyin_obs, more frames than threads (the store's second turn, the walk back over hundreds of frames), the second grid
of a call with more than 32 768 clips, and the largest dynamic LDS request.  The comparisons are tests/test_gpu_clip_pyin.py's:
mode 1 against the definition on decode_clips_pitch's own curve, mode 0 against the definition's decode of mode 1's own output.

Streams do not steer the path into a thread's second bin: on noise it stays unvoiced or below bin 800 or so.  The planted curves
of tests/clip_pyin_cases.py do, handed to the kernels through the engine's C-ABI (tests/clip_engine_calls.py); there the
definition's own decode is decided in every frame (asserted first) and the device's path must be it."""
import time

import numpy as np
import pytest

import clip_engine_calls as ec
import clip_gpu as cg
import clip_gpu_calls as cc
import clip_pyin_cases as pc
import clip_pyin_ref as ref

pytestmark = pytest.mark.gpu

SMALL = ref.args(sample_rate=16000, frame_length=256, win_length=128, hop=64, fmin=16000 / 137.5, fmax=16000 / 2.5)     # lags 2 .. 127, 694 bins
WIDE = ref.args(sample_rate=16000, frame_length=2048, win_length=512, hop=256, fmin=10.5, fmax=21.0, resolution=0.5)      # lags 761 .. 1524, 25 bins
LDS_DYNAMIC = 65536                                # the most a launch asks for dynamically; above it the static 160 KB form


def _plan(a, f, mode="pitch"):
    from pdmp3_amd import api
    return api.pyin_plan(a["sample_rate"], n_frames=f, out_mode=mode, **pc.kw(a))


def _both_modes(a, name, f, channels, starts=None):
    """tests/test_gpu_clip_pyin.py's comparison of both modes on clips of the stream -> (obs, planes, worst, most, open, frames)"""
    k = ref.numbers(a)
    dec = cg.decoder()
    try:
        j_all = cg.j_all(dict(a, channels=channels), name)
        clips = [(name, s) for s in (starts or (k["N"] // 2 - 7, j_all // 3 + 11, j_all - (f // 2) * k["H"] - 3))]
        curve, valid_c = cc.pyin_curve(dec, clips, f, a, channels)
        obs, valid1 = cc.pyin_run(dec, "device", clips, f, a, channels, "observation")
        planes, valid0 = cc.pyin_run(dec, "device", clips, f, a, channels, "pitch")
    finally:
        dec.close()
    assert np.array_equal(valid_c, valid1) and np.array_equal(valid1, valid0)
    worst, most, open_frames, frames = cc.pyin_check_both(clips, curve, obs, planes, a, channels)
    return obs, planes, valid0, worst, most, open_frames, frames


# ---- 1. many bins ----
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("f", [9, 17])
@pytest.mark.parametrize("case", ["nb1025", "nb1201", "nb2048-obs4", "nb2048-nt256-obs2", "nb2048-tmax2000-obs2"])
def test_many_bins_against_the_definition(case, f, channels):
    """The big path kernel, with one bin over the threads (1025), a fifth over (1201) and two bins a thread (2048); the observation
    kernel at 8, 4 and 2 frames a workgroup.  Each on the stream whose own rate the shape names, three clips, the third over the
    stream's end.  The 1025th bin is narrower than a lag, so there alone no entry at a bin >= 1024 is asked for on a stream;
    test_a_planted_trough_in_the_1025th_bin puts one there."""
    a, frames_wg = pc.MANY[case]
    name = {48000: "48k", 16000: "16k-mono", 22050: "22k"}[a["sample_rate"]]
    k, plan = ref.numbers(a), _plan(a, f)
    assert plan["path_lds"] > LDS_DYNAMIC and plan["path_threads"] == 1024 < plan["n_bins"] == k["n_b"] and plan["obs_frames"] == frames_wg
    assert _plan(a, f, "observation")["obs_frames"] == frames_wg
    j_all = cg.j_all(dict(a, channels=channels), name)
    starts = [k["N"] // 2 - 7, j_all // 3 + 11, j_all - (f // 2) * k["H"] - 3]
    obs, planes, valid, worst, most, open_frames, frames = _both_modes(a, name, f, channels, starts)
    assert 0 < valid[-1] < f and valid[0] == f
    upper = int(np.count_nonzero(obs[:, :, 1024:-1]))
    print("%s, F %d, %d channel(s): observation worst error / bound %.3f, troughs up to %d a frame, %d entries at bins >= 1024; %d of %d "
          "frames without the margin; the path: %d voiced frames, largest bin %d" % (case, f, channels, worst, most, upper, open_frames, frames,
                                                                                    int((planes[:, :, 1] == 1).sum()), int(planes[:, :, 3].max())))
    assert worst <= 1.0 and most >= 2 and (upper > 0 or k["n_b"] == 1025)
    assert (obs[-1, :, :, -1] == 0).all() and (planes[-1, :, 1, -1] == 0).all() and np.isnan(planes[-1, :, 0, -1]).all()


# ---- 2. long clips ----
def test_more_frames_than_threads():
    """694 bins on 704 threads, F = 709 at hop 64: the store of the planes takes a second turn, the walk back goes over 708
    back-pointer rows and the two buffers change roles 708 times.  One clip, mono."""
    a, name, f = SMALL, "16k-mono", 709
    plan = _plan(a, f)
    assert plan["path_threads"] == 704 < f and plan["n_bins"] == 694 and plan["path_lds"] <= LDS_DYNAMIC
    assert cg.j_all(dict(a, channels=1), name) > 3000 + f * 64
    t0 = time.time()
    obs, planes, valid, worst, most, open_frames, frames = _both_modes(a, name, f, 1, [3000])
    print("F 709 at 694 bins: observation worst error / bound %.3f; %d of %d frames without the margin; %d voiced frames, bins %d .. %d (%.1f s)"
          % (worst, open_frames, frames, int((planes[0, 0, 1] == 1).sum()), int(planes[0, 0, 3].min()), int(planes[0, 0, 3].max()), time.time() - t0))
    assert worst <= 1.0 and valid[0] == f


def test_a_long_clip_at_25_bins():
    """25 bins on 64 threads, F = 131: two turns of the store and a third begun"""
    a, name, f = WIDE, "16k-mono", 131
    plan = _plan(a, f)
    assert plan["path_threads"] == 64 and 2 * 64 < f and plan["n_bins"] == 25
    obs, planes, valid, worst, most, open_frames, frames = _both_modes(a, name, f, 1, [20000])
    print("F 131 at 25 bins: observation worst error / bound %.3f; %d of %d frames without the margin" % (worst, open_frames, frames))
    assert worst <= 1.0 and valid[0] == f


# ---- 3. more clips than one grid ----
TINY = ref.args(sample_rate=8000, frame_length=64, win_length=32, hop=16, fmin=8000 / 30.5, fmax=4000.0, resolution=1.0)       # lags 2 .. 31


def test_more_clips_than_one_grid():
    """32 768 + 5 two-frame clips in one call of mode "pitch": pdmp3_hip_clip_pitch and pdmp3_hip_clip_pyin launch their kernels
    twice (a grid's y extent), the second time from descriptor 32 768 on.  Sixty-four distinct clips are held against the
    definition in both modes, every row is bit-equal to its twin among them; the last five are other clips than rows 0 .. 4, one
    of them behind the end"""
    a, name, k, f = TINY, "8k", 32768 + 5, 2
    nums = ref.numbers(a)
    assert (nums["tmin"], nums["tmax"]) == (2, 31)
    mp3, ix = cg.source(name)
    j_all = cg.j_all(dict(a, channels=1), name)
    starts = [1000 + 3001 * i for i in range(62)] + [j_all + 64 + 9, j_all - 5]
    assert starts[61] + 64 < j_all
    twin = (np.arange(k, dtype=np.int64) * 7) % 62
    twin[32768:] = [62, 63, 61, 60, 59]
    assert not np.any(twin[32768:] == twin[:5])
    dec = cg.decoder()
    try:
        first = [(name, s) for s in starts]
        curve, _ = cc.pyin_curve(dec, first, f, a, 1)
        obs, _ = cc.pyin_run(dec, "device", first, f, a, 1, "observation")
        base, valid64 = cc.pyin_run(dec, "device", first, f, a, 1, "pitch")
        held = [i for i in range(64) if i != 62]                    # (the clip behind the end has no frame to hold)
        worst, most, open_frames, frames = cc.pyin_check_both(held, curve[held], obs[held], base[held], a, 1)
        assert worst <= 1.0 and list(valid64[61:]) == [2, 0, 1]
        assert np.unique(base[:62, 0, 2, 0]).size > 8, "the sixty-two clips inside the stream must differ"
        big, view = cg.destination("device", k, 1, (4, f))
        out, valid = dec.decode_clips_pyin([(mp3, ix, int(starts[t])) for t in twin], f, out_mode="pitch", out=view, channels=1, **a)
        host = cg.host(big).reshape(k, 4 * f + cg.GUARD)
        assert (host[:, 4 * f:] == cg.SENT).all(), "written behind a row's floats"
        assert np.array_equal(valid, valid64[twin]) and list(valid[32768:]) == [0, 1, 2, 2, 2]
        bad = np.flatnonzero((host[:, :4 * f].view(np.uint32) != base[twin, 0].reshape(k, 4 * f).view(np.uint32)).any(axis=1))
        assert bad.size == 0, "%d rows differ from their twins, %d of them in the second launch: %s" % (bad.size, int((bad >= 32768).sum()), bad[:8].tolist())
    finally:
        dec.close()


# ---- 4. planted curves through the engine's C-ABI ----
def _planted(engine, a, curve):
    t = cc.pyin_tables(a)
    ec.check_sizes()
    with ec.stream(engine) as (lib, hs):
        obs, planes, plan = ec.pyin_path(lib, hs, curve, a, t)
    k = ref.numbers(a)
    worst, most = ref.check_observation(curve, obs, t, k["tmin"], k["tmax"], a["no_trough_prob"])
    open_frames, s, best = ref.check_path(obs, planes, t)
    return obs, planes, plan, open_frames


def test_a_planted_l0_jump_between_two_upper_bins(engine):
    """tests/test_clip_pyin_host.py's case of the same name on the device: 2048 bins, F = 9, one clip -- the narrowest launch of
    k_clip_pyin_path_big.  The definition alone first, then the device's path: the planted bins, all voiced, decided."""
    a, f = pc.BINS_2048, 9
    t = cc.pyin_tables(a)
    curve, bins = pc.jump(a, t, f, 4, 1200, 1700)
    assert bins[0] >= 1024 and bins[-1] - bins[0] > 8 * t["hb"]
    want, sure = pc.decided(pc.observation(curve, a, t), t)
    assert np.array_equal(want, bins) and sure.all(), "the reference's own decode does not take the jump"
    obs, planes, plan, open_frames = _planted(engine, a, curve)
    assert plan["path_lds"] > LDS_DYNAMIC and plan["path_threads"] == 1024 and plan["n_bins"] == 2048
    assert (obs[2048] == 1.0).all() and open_frames == 0 and np.array_equal(planes[3], bins) and (planes[1] == 1).all()
    assert np.array_equal(planes[0], t["f0"][bins])


def test_a_planted_glide_through_the_second_bin_of_a_thread(engine):
    """tests/test_clip_pyin_host.py's case of the same name on the device: the bin rises through 1024 by at most hb a frame"""
    a, f = pc.BINS_2048, 17
    t, k = cc.pyin_tables(a), ref.numbers(a)
    curve, bins = pc.glide(a, t, f, 900, 23)
    assert (np.abs(np.diff(bins)) <= k["hb"]).all() and (bins >= 1024).sum() >= 5 and (bins < 1024).sum() >= 5
    want, sure = pc.decided(pc.observation(curve, a, t), t)
    assert np.array_equal(want[1:], bins[1:]) and sure.all(), "the reference's own decode does not follow the planted bins"
    obs, planes, plan, open_frames = _planted(engine, a, curve)
    assert plan["path_lds"] > LDS_DYNAMIC and plan["path_threads"] == 1024 and plan["obs_frames"] == 4
    assert open_frames == 0 and np.array_equal(planes[3, 1:], bins[1:]) and (planes[1, 1:] == 1).all() and planes[1, 0] == 0
    assert (planes[3] >= 1024).sum() >= 5


def test_a_planted_trough_in_the_1025th_bin(engine):
    """tests/test_clip_pyin_host.py's case of the same name on the device.  The 1025-bin cases on streams have no entry at bin
    1024, which is narrower than a lag; here the observation's only entry lies there, is held to the definition, and the path is
    voiced at thread 0's second bin in every frame."""
    a, f = pc.BINS_1025, 9
    t = cc.pyin_tables(a)
    curve, b = pc.top_bin(a, t, f)
    o64 = pc.observation(curve, a, t)
    want, sure = pc.decided(o64, t)
    assert b == 1024 and (np.flatnonzero(o64[:-1, 0]) == [b]).all() and (want == b).all() and sure.all()
    obs, planes, plan, open_frames = _planted(engine, a, curve)
    assert plan["path_lds"] > LDS_DYNAMIC and plan["path_threads"] == 1024 and plan["n_bins"] == 1025
    assert open_frames == 0 and (planes[3] == b).all() and (planes[1] == 1).all() and (obs[b] == 1.0).all() and np.count_nonzero(obs[:-1]) == f


def test_a_planted_switch_of_voicing(engine):
    """tests/test_clip_pyin_host.py's test_the_optimum_switches_voicing_on_a_planted_curve on the device, 601 bins"""
    a, f = ref.args(), 17
    t = cc.pyin_tables(a)
    curve, b = pc.voiced_stretch(a, t, f, 5, 11, 300)
    o64 = pc.observation(curve, a, t)
    voiced, sure_v = pc.voicing(o64, t)
    want, sure = pc.decided(o64, t)
    assert voiced.tolist() == [False] * 5 + [True] * 6 + [False] * 6 and sure_v.all() and (want[5:11] == b).all() and sure[5:11].all()
    obs, planes, plan, open_frames = _planted(engine, a, curve)
    assert np.array_equal(planes[1] == 1, voiced) and (planes[3, 5:11] == b).all()
    assert np.isnan(planes[0, ~voiced]).all() and (planes[0, 5:11] == t["f0"][b]).all()


# ---- 5. the largest dynamic LDS request (last: the launch that asks for it raises the kernel's limit for the process) ----
# 8 (8 n_b + 2 hb + 97) bytes: at most 65 528, which takes hb = 3 (mod 4) -- fourteen bins a semitone, a band of one semitone
LARGEST = ref.args(sample_rate=16000, frame_length=1024, win_length=512, hop=256, fmin=40.0, fmax=40.0 * 2 ** (1009.5 / 168), resolution=0.0715,
                   max_transition_rate=5.2)


def test_the_largest_dynamic_lds_request():
    """1010 bins, hb 7: the path kernel's dynamic form with 65 528 bytes, the largest request there is below the static form"""
    a = LARGEST
    plan, k = _plan(a, 9), ref.numbers(a)
    assert plan["path_lds"] == LDS_DYNAMIC - 8 and (plan["n_bins"], plan["hb"], plan["path_threads"]) == (1010, 7, 1024) == (k["n_b"], k["hb"], 1024)
    obs, planes, valid, worst, most, open_frames, frames = _both_modes(a, "16k-mono", 9, 1)
    print("the largest dynamic request: observation worst error / bound %.3f; %d of %d frames without the margin" % (worst, open_frames, frames))
    assert worst <= 1.0 and 0 < valid[-1] < 9
