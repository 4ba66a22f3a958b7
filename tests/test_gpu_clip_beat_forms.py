"""Every launch form of the beat kernels on the device, each named by the plan the test asserts: the
programme's step at 32, 8, 4 lanes a frame and one, at h = 256 (the last step of one pass) and h > 256 (two passes); the frame
limit of 32 768, where the score kernel holds 513 block sums and the rank by counting goes over thousands of maxima; the second
grid of a call with more than 32 768 clips, with the tempo estimated, so that a (clip, channel)'s scratch row -- which
`first + blockIdx.y` indexes -- holds the period the tracker runs at, and the same through the C-ABI over a scratch of the
test's own, where the rows of the second launch are looked at; a tie among a frame's candidates decided on the device.
The comparisons are tests/test_gpu_clip_beat.py's: every stage bit for bit against the restatement on the stage before.

Ties hardly occur on real envelopes, so the tie rule is run on planted ones, handed to the three kernels through the engine's
C-ABI (tests/clip_engine_calls.py) with a flat transition cost in place of the product's."""
import functools

import numpy as np
import pytest

import clip_beat_cases as bc
import clip_beat_ref as ref
import clip_engine_calls as ec
import clip_gpu as cg
import clip_gpu_calls as cc
from clip_streams import ISO_LSF

pytestmark = pytest.mark.gpu

LONG = "beat-forms/44k-mono-1500"
P64 = dict(cc.BEAT_P0, sample_rate=0, hop=64, n_mels=8)                 # the stream's own rate: 689 frames a second
P32 = dict(P64, hop=32)


@functools.lru_cache(maxsize=None)
def _long():
    """1500 MPEG-1 frames at 44.1 kHz, mono: 1 728 000 samples, 27 000 frames at hop 64"""
    from pdmp3_amd import api
    from pdmp3_amd.packer import packer
    mp3 = packer.generate(n_frames=1500, seed=4415, sfreq=0, mode=3, bitrate_index=7)
    return mp3, api.StreamIndex(mp3, ISO_LSF)


cg.STREAMS[LONG] = _long


def _plan(p, f, period):
    from pdmp3_amd import api
    q = {a: p[a] for a in cc.BEAT_P0 if a not in ("sample_rate", "channels")}
    return api.beat_plan(44100, n_frames=f, bpm=cc.beat_bpm_of(period, 44100, p["hop"]), **q)


# ---- 4. every lane count ----
FORMS = {12: (6, 32), 45: (22, 8), 100: (50, 4), 300: (150, 1), 513: (256, 1), 515: (258, 1), 1023: (512, 1)}      # P -> (h, lanes)


@pytest.mark.parametrize("period", sorted(FORMS))
def test_every_form_of_the_programmes_step(period):
    """one clip inside the stream with more than 2 P + 3 h frames: whole windows over more than two steps"""
    h, lanes = FORMS[period]
    f = 2 * period + 3 * h + 1 + 7
    plan = _plan(P64, f, period)
    assert (plan["period"], plan["h"], plan["lanes"], plan["frames"]) == (period, h, lanes, 256 // lanes) and plan["threads"] == 256
    assert plan["steps"] == -(-f // h) and (h > 256) == (period >= 515)
    dec = cg.decoder()
    try:
        res, valid = cc.beat_check_chain(dec, [(LONG, 5000)], f, P64, period)
        assert valid[0] == f
        stats = res[True][1]
        print("P %d, h %d, %d lanes: kept %d of %d beats, tail %d" % (period, h, lanes, stats[0, 0, 2], stats[0, 0, 3], stats[0, 0, 4]))
        assert stats[0, 0, 3] >= 1
    finally:
        dec.close()


def test_a_clip_over_the_end_with_fewer_frames_than_two_periods():
    """P = 1023 and 1500 valid frames of 1600: no frame has a whole window, the last step is cut by n"""
    period, f = 1023, 1600
    assert _plan(P64, f, period)["lanes"] == 1
    j_all = cg.j_all(P64, LONG)
    dec = cg.decoder()
    try:
        res, valid = cc.beat_check_chain(dec, [(LONG, j_all - 1499 * 64 - 3)], f, P64, period)
        assert valid[0] == 1500 < 2 * period
    finally:
        dec.close()


# ---- 5. the frame limit ----
@pytest.mark.parametrize("period", [2, 45])
def test_the_frame_limit(period):
    """F = 32 768 at hop 32: 513 block sums in the score kernel's LDS, 128 tiles of the score, thousands of local maxima for the
    rank by counting (asserted at P = 2 on the beats of the walk); one clip inside the stream, one that ends behind it"""
    from pdmp3_amd import api
    f = 32768
    assert not api.beat_check(44100, n_frames=f + 1, hop=32, n_mels=8) and _plan(P32, f, period)["period"] == period
    j_all = cg.j_all(P32, LONG)
    clips = [(LONG, 40000), (LONG, j_all - 20000 * 32 - 5)]
    assert clips[0][1] + f * 32 + 2048 < j_all
    dec = cg.decoder()
    try:
        res, valid = cc.beat_check_chain(dec, clips, f, P32, period)
        assert list(valid) == [f, 20001]
        stats = res[True][1]
        print("F 32768, P %d: kept %s of %s beats, tails %s" % (period, stats[:, 0, 2], stats[:, 0, 3], stats[:, 0, 4]))
        assert period != 2 or (stats[:, 0, 3] > 1000).all()
    finally:
        dec.close()


# ---- 6. more clips than one grid, the tempo estimated ----
def test_more_clips_than_one_grid_with_the_tempo_estimated():
    """32 768 + 5 clips of 24 frames, bpm = 0: pdmp3_hip_clip_beat launches its kernels twice, the second time from descriptor
    32 768 on and with `first` = 32 768, which is where a (clip, channel)'s scratch row lies -- and with it the period that the
    tempo call left there.  A wrong `first` makes clip 32 768 + i track at clip i's period: the five clips of the second launch
    are chosen, on the device's own sixty-four rows, to have another period than rows 0 .. 4.  (With bpm given the test could
    not see it: the scratch of rows 0 .. 4 is free by then.)  Every row and its stats are bit-equal to their twin's."""
    name, k, f = "8k", 32768 + 5, 24
    p = dict(cc.BEAT_P0, sample_rate=0, hop=64, n_mels=8, win_length=64)          # 125 frames a second: lags 24 .. 63 are tempi below 320
    mp3, ix = cg.source(name)
    j_all = cg.j_all(p, name)
    starts = [3000 + 3001 * i for i in range(63)] + [j_all - 15 * 64 - 5]
    assert starts[62] + f * 64 + 1024 < j_all
    dec = cg.decoder()
    try:
        first = [(name, s) for s in starts]
        base, stats64, valid64 = cc.beat_run(dec, "device", first, f, p, "beats")
        period = stats64[:, 0, 1]
        runs = (period > 0) & (stats64[:, 0, 3] >= 1)
        print("periods of the sixty-four: %s; the tracker runs on %d" % (period.astype(int).tolist(), int(runs.sum())))
        assert runs.sum() >= 32 and valid64[63] == 16 and (valid64[:63] == f).all()
        twin = (np.arange(k, dtype=np.int64) * 7) % 62
        # the last five: the clip over the end first, then others from the back, each with another period than its counterpart's
        free = [63, 62] + list(range(61, 34, -1))
        for i in range(5):
            pick = next(j for j in free if runs[j] and runs[twin[i]] and period[j] != period[twin[i]] and j not in twin[:5])
            free.remove(pick)
            twin[32768 + i] = pick
        assert 63 in twin[32768:] and (period[twin[32768:]] != period[twin[:5]]).all() and runs[twin[:5]].all() and runs[twin[32768:]].all()
        big, view = cg.destination("device", k, 1, (2, f))
        stats = cg.filled("device", (k + 1, 1, 8))
        out, st, valid = dec.decode_clips_beats([(mp3, ix, int(starts[t])) for t in twin], f, out_mode="beats", out=view, stats=stats[:k], **p)
        host = cg.host(big).reshape(k, 2 * f + cg.GUARD)
        got_stats = cg.host(stats)
        assert (host[:, 2 * f:] == cg.SENT).all() and (got_stats[k] == cg.SENT).all(), "written behind a row's floats"
        assert np.array_equal(valid, valid64[twin])
        want = base[twin, 0].reshape(k, 2 * f)
        bad = np.flatnonzero((host[:, :2 * f].view(np.uint32) != want.view(np.uint32)).any(axis=1) |
                             (got_stats[:k, 0].view(np.uint32) != stats64[twin, 0].view(np.uint32)).any(axis=1))
        assert bad.size == 0, "%d rows differ from their twins, %d of them in the second launch: %s" % (bad.size, int((bad >= 32768).sum()), bad[:8].tolist())
    finally:
        dec.close()


# ---- 8. a tie decided on the device ----
TIE_FORMS = {2: 64, 7: 64, 12: 32, 22: 16, 45: 8, 100: 4, 200: 2, 300: 1, 515: 1}          # P -> lanes; 515: two passes


@pytest.mark.parametrize("period", sorted(TIE_FORMS))
def test_a_tie_from_a_planted_envelope(engine, period):
    """tests/test_clip_beat_host.py's case of the same name on the device: 64, 32, 16, 8, 4, 2 lanes a frame, one, and two passes.
    First the restatement alone: frames whose best candidate is not alone.  Then mode "score" is the restatement's local score,
    mode "dp" its programme on that score, mode "beats" its track, all bit for bit."""
    n = 3 * period + 41
    o = bc.tie_envelope(period, n)
    g, tx = cc.beat_tables(period)[0], np.zeros(2 * period + 1)
    want = ref.track(o, n, period, g, tx, True)
    cum, back = ref.programme(want["score"], period, tx)
    ties = bc.tied_frames(cum, period)
    assert ties >= 1 and want["stats"][1] >= 2
    ec.check_sizes()
    with ec.stream(engine) as (lib, hs):
        score, s0, plan = ec.beat_track(lib, hs, o, n, period, g, tx, 0)
        dp, s1, _ = ec.beat_track(lib, hs, o, n, period, g, tx, 1)
        beats, s2, _ = ec.beat_track(lib, hs, o, n, period, g, tx, 2)
    print("P %d, %d lanes: %d frames with a tie among their candidates" % (period, plan["lanes"], ties))
    assert (plan["period"], plan["lanes"], plan["h"] > 256) == (period, TIE_FORMS[period], period == 515)
    cc.beat_same(score, want["score"], "score")
    cc.beat_same(dp, want["dp"], "dp")
    cc.beat_same(dp[1], back.astype(np.float32), "back")
    cc.beat_same(beats, want["beats"], "beats")
    cc.beat_same(s2[2:], want["stats"], "stats")
    cc.beat_same(s0, s1, "stats of modes 0 and 1")
    assert s2[1] == period


# ---- 9. where the scratch of a non-zero `first` lies ----
def test_the_scratch_rows_of_the_second_launch(engine):
    """32 768 + 2 planted clips through pdmp3_hip_clip_beat, bpm given (P 2, the product's tables), F = 47: the engine launches
    twice, the second time with `first` = 32 768, and row_of must find clip 32 768 + i's scratch at row 32 768 + i.  The scratch
    is the test's own, sentinel-filled, with a guard behind row 32 769.  The first launch's clips share one envelope, the two of
    the second launch have one each, so a row says whose it is: every row's header flag is set and its cum is the restatement's
    programme of the clip that belongs there, in binary64 -- with `first` = 0 in the second launch rows 0 and 1 would hold the
    last two clips' and rows 32 768 and 32 769 the sentinel.  Rows and stats are the restatement's track, bit for bit."""
    period, f, k = 2, 47, 32768 + 2
    envs = np.stack([bc.tie_envelope(period, f, seed=s) for s in (2, 77, 78)])
    g, tx = cc.beat_tables(period)
    want = [ref.track(o, f, period, g, tx, True) for o in envs]
    cums = np.stack([ref.programme(w["score"], period, tx)[0] for w in want])
    assert all(w["stats"][1] >= 2 for w in want) and not np.array_equal(cums[1], cums[2]) and not np.array_equal(cums[0], cums[1])
    which = np.zeros(k, dtype=np.int64)
    which[32768:] = [1, 2]
    ec.check_sizes()
    with ec.stream(engine) as (lib, hs):
        rows, stats, work, p, plan = ec.beat_track_many(lib, hs, envs, which, f, period, g, tx)
    assert plan["period"] == period and p.work_stride == 8 + 2 * f + (3 * f + 1) // 2
    assert not (work[:, 8:8 + f] == -7.25).any() and (work[:, 3] == 1.0).all(), "a clip's scratch row was not written"
    norms = np.array([w["stats"][3] for w in want], dtype=np.float32)
    assert np.array_equal(work[:, 2].astype(np.float32), norms[which])
    bad = np.flatnonzero((work[:, 8:8 + f] != cums[which]).any(axis=1))
    assert bad.size == 0, "%d scratch rows do not hold their clip's cum, %d of them in the second launch: %s" % (bad.size, int((bad >= 32768).sum()), bad[:8].tolist())
    cc.beat_same(rows, np.stack([w["beats"] for w in want])[which], "beats")
    cc.beat_same(stats[:, 2:], np.stack([w["stats"] for w in want])[which], "stats")
    assert (stats[:, 1] == period).all()
