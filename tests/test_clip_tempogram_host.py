"""Onset strength, tempogram and tempo of clips on the host, no GPU: the refusals of the check, the
window, the prior and the plan against their restatement, the restatement of steps 4-5 against numpy.correlate, and the kernels'
own phases (pdmp3_amd/csrc/tempogram_core.h, compiled here with g++ into tests/host_emul/tempogram_emul.cpp and run thread by
thread on wave_emul.h's fibers over a poisoned LDS) against the binary64 definition within the derived bounds, on synthetic
log-mel arrays: every band count, neighbourhood and lag of the flux, every geometry of lag tiles and workgroups, silence, a click
train, and item 7's consistency of the three modes."""
import ctypes as C

import numpy as np
import pytest

import clip_tempogram_ref as ref
from clip_host import build_emul, run_sanitizer_program

LDS_MAX = ref.LDS_MAX


class TgDesc(C.Structure):                         # include/pdmp3_hip.h pdmp3_tempogram_desc
    _fields_ = [("mel", C.c_uint64), ("env", C.c_uint64), ("tg", C.c_uint64), ("dst", C.c_uint64), ("dst_chan_stride", C.c_uint64)]


class TgParams(C.Structure):                       # include/pdmp3_hip.h pdmp3_tempogram_params
    _fields_ = [("sr", C.c_double), ("n_mels", C.c_int32), ("lag", C.c_int32), ("half", C.c_int32), ("hop", C.c_int32), ("win", C.c_int32),
                ("tiles", C.c_int32), ("ksteps", C.c_int32), ("n_frames", C.c_int32), ("frames_wg", C.c_int32), ("n_mel_frames", C.c_int32),
                ("n_env", C.c_int32), ("channels", C.c_int32), ("out_mode", C.c_int32), ("env_stride", C.c_uint32), ("ext", C.c_uint32),
                ("span_floats", C.c_uint32), ("lds_bytes", C.c_uint32)]


def _api():
    from pdmp3_amd import api
    return api


def _emul():
    lib = build_emul("tempogram")
    lib.emul_clip_tempogram.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    assert lib.emul_tempogram_params_bytes() == C.sizeof(TgParams) and lib.emul_tempogram_desc_bytes() == C.sizeof(TgDesc)
    return lib


SR, HOP = 22050, 512
GUARD = 8


def emulate(l, f, lag, max_size, wt, mode, sr=SR, hop=HOP, **prior_kw):
    """l: the log-mel [n_mels, n_env + lag] of one channel -> the emulated kernels' output of `mode`: [f], [wt, f] or [4]"""
    api = _api()
    l = np.ascontiguousarray(l, dtype=np.float32)
    nm = l.shape[0]
    n_env = f if mode == 0 else f + wt - 1
    assert l.shape[1] == n_env + lag
    front, back, tiles, ksteps, frames, lds = api.tempogram_plan(sr, hop=hop, n_mels=nm, lag=lag, max_size=max_size, win_length=wt, out_mode=mode, **prior_kw)
    assert (front, back, tiles, ksteps, frames, lds) == ref.plan(lag, wt, mode)
    ext, span = ref.geometry(wt, frames)
    env_stride = (n_env + 3) & ~3
    per = (f, wt * f, 4)[mode]
    dst = np.full(per + GUARD, -5.0, dtype=np.float32)
    env = dst if mode == 0 else np.full(env_stride + GUARD, 7e29, dtype=np.float32)
    tg = dst if mode == 1 else np.full(wt * f + GUARD, 7e29, dtype=np.float32)
    w = api.tempogram_window(wt)
    pr = api.tempogram_prior(sr, hop=hop, n_mels=nm, win_length=wt, **prior_kw)[0]
    P = TgParams(float(sr), nm, lag, (max_size - 1) // 2, hop, wt, tiles, ksteps, f, frames, n_env + lag, n_env, 1, mode, env_stride, ext, span, lds)
    d = TgDesc(l.ctypes.data, env.ctypes.data, tg.ctypes.data, dst.ctypes.data, per + GUARD)
    assert _emul().emul_clip_tempogram(C.byref(d), 1, w.ctypes.data, pr.ctypes.data, C.byref(P)) == 0, "the emulated kernel read LDS it must not read"
    assert (dst[per:] == -5.0).all()
    if mode != 0:
        assert (env[n_env:] == np.float32(7e29)).all()
    if mode == 2:
        assert (tg[wt * f:] == np.float32(7e29)).all()
    return dst[:per].reshape((f,) if mode == 0 else (wt, f) if mode == 1 else (4,)).copy()


def log_mel(nm, frames, seed):
    """a log-mel that moves: noise around -4 with a slow swell and sudden rises every 11 frames"""
    rng = np.random.default_rng(seed)
    l = -4.0 + 0.5 * rng.standard_normal((nm, frames)) + 0.7 * np.sin(np.arange(frames) / 9.0)[None, :]
    l[:, ::11] += 1.5
    return l.astype(np.float32)


# ---- 1. the check ----
def test_the_checks_refusals_one_by_one():
    api = _api()
    ok = dict(n_fft=2048, hop=512, n_mels=128, lag=1, max_size=1, win_length=384, start_bpm=120.0, std_bpm=1.0, max_tempo=320.0, out_mode="tempogram")
    assert api.tempogram_check(22050, **ok) and api.tempogram_check(22050)
    assert api.tempogram_check(22050, **dict(ok, n_fft=4096, lag=16, max_size=9, win_length=1024, out_mode="tempo"))
    assert api.tempogram_check(22050, **dict(ok, win_length=16, out_mode="onset"))
    for bad in (dict(lag=0), dict(lag=17), dict(lag=-1), dict(max_size=0), dict(max_size=2), dict(max_size=11), dict(max_size=-1),
                dict(win_length=14), dict(win_length=17), dict(win_length=385), dict(win_length=1026), dict(win_length=0),
                dict(start_bpm=0.0), dict(start_bpm=-120.0), dict(start_bpm=float("nan")), dict(start_bpm=float("inf")),
                dict(std_bpm=0.0), dict(std_bpm=float("nan")), dict(std_bpm=float("inf")),
                dict(max_tempo=0.0), dict(max_tempo=-1.0), dict(max_tempo=float("nan")), dict(max_tempo=float("inf")),
                dict(out_mode=3), dict(out_mode=-1), dict(out_mode="bpm"), dict(n_frames=-1),
                # whatever the log-mel check refuses
                dict(n_fft=1024), dict(n_fft=2047), dict(hop=0), dict(hop=2049), dict(n_mels=0), dict(n_mels=257), dict(floor=0.0),
                dict(f_min=-1.0), dict(f_max=20000.0), dict(fft_win_length=2049),
                # a prior that is -inf at every lag: the first lag under max_tempo lies beyond the window
                dict(max_tempo=60.0 * 22050 / (512 * 16.0), win_length=16), dict(max_tempo=1.0),
                # a row beyond 31 bits
                dict(n_frames=2 ** 31 // 384 + 1), dict(n_frames=2 ** 31 // 128, out_mode="onset")):
        assert not api.tempogram_check(22050, **dict(ok, **bad)), bad
    # the edge that passes: lag 15 is the only admissible one of a window of 16
    kw = dict(ok, win_length=16, max_tempo=60.0 * 22050 / (512 * 14.5))
    assert api.tempogram_check(22050, **kw) and api.tempogram_prior(22050, **kw)[1] == 15
    assert not api.tempogram_check(0, **ok)
    assert api.tempogram_check(22050, **dict(ok, n_frames=2 ** 31 // 384 - 400))


# ---- 2. window, prior, plan ----
@pytest.mark.parametrize("wt", [16, 256, 272, 384, 1024])
def test_window_prior_and_plan_against_the_restatement(wt):
    api = _api()
    w = api.tempogram_window(wt)
    assert w.dtype == np.float32 and np.array_equal(w.view(np.uint32), ref.window(wt).view(np.uint32)) and w[0] == 0.0 and w[wt // 2] == 1.0
    for sr, hop, kw in ((22050, 512, {}), (44100, 512, dict(start_bpm=90.0, std_bpm=0.5, max_tempo=200.0)), (48000, 64, dict(max_tempo=3000.0))):
        want, first = ref.prior(sr, hop, wt, **kw)
        if not first:
            assert not api.tempogram_check(sr, hop=hop, win_length=wt, **kw)
            continue
        got, first_got = api.tempogram_prior(sr, hop=hop, win_length=wt, **kw)
        assert first_got == first and got[0] == -np.inf and np.array_equal(np.isfinite(got), np.isfinite(want))
        fin = np.isfinite(want)
        assert np.abs(got[fin] - want[fin]).max() <= 1e-12 and (got[fin] <= 0.0).all()
    for lag in (1, 16):
        for mode in (0, 1, 2):
            got = api.tempogram_plan(22050, lag=lag, win_length=wt, out_mode=mode)
            assert got == ref.plan(lag, wt, mode) and got[4] == 8 and got[5] <= LDS_MAX and got[2] == -(-wt // 256) and got[3] == -(-(wt + 15) // 4)
    with pytest.raises(ValueError):
        api.tempogram_plan(22050, win_length=wt + 1)
    with pytest.raises(ValueError):
        api.tempogram_window(wt + 1)
    assert api.tempogram_plan(22050)[:4] == (193, 191, 2, 100)          # the defaults: 200 matrix instructions a frame


# ---- 3. the restatement ----
def test_the_restatement_is_numpys_correlation():
    rng = np.random.default_rng(21)
    for wt in (16, 272, 384):
        f = 5
        o = np.abs(rng.standard_normal(f + wt - 1)).astype(np.float32)
        x = ref.frames_of(o, wt, f)
        assert x.dtype == np.float32 and np.array_equal(x[2], ref.window(wt) * o[2:2 + wt])
        t, b = ref.tempogram(o, wt, f)
        for i in range(f):
            xd = x[i].astype(np.float64)
            full = np.correlate(xd, xd, mode="full")[wt - 1:]
            assert np.abs(t[:, i] - full / full[0]).max() <= 1e-12
        assert (t[0] == 1.0).all() and (np.abs(t) <= 1.0).all() and (b > 0).all() and b.max() < 4e-4
    t, b = ref.tempogram(np.zeros(20 + 15, dtype=np.float32), 16, 20)
    assert (t == 0.0).all() and (b == 0.0).all()
    x = np.array([[-3.0, 0.0, 1.0], [2.0, 5.0, 4.0], [1.0, 1.0, 9.0], [0.0, -1.0, 2.0]])
    assert np.array_equal(ref.band_max(x, 1), x)
    assert np.array_equal(ref.band_max(x, 3), np.array([[2.0, 5.0, 4.0], [2.0, 5.0, 9.0], [2.0, 5.0, 9.0], [1.0, 1.0, 9.0]]))
    assert np.array_equal(ref.band_max(x, 9), np.broadcast_to(x.max(axis=0), x.shape))


# ---- 4. the flux ----
@pytest.mark.parametrize("nm", [1, 40, 128])
def test_onset_strength_over_bands_neighbourhoods_and_lags(nm):
    worst = 0.0
    for max_size in (1, 3, 9):
        for lag in (1, 3, 16):
            f = 300                                     # (more than one workgroup of 256 lanes on the device)
            l = log_mel(nm, f + lag, 100 * nm + 10 * max_size + lag)
            got = emulate(l, f, lag, max_size, 384, 0)
            want, bound = ref.onset(l, lag, max_size)
            err = np.abs(got.astype(np.float64) - want)
            assert (err <= bound).all(), (nm, max_size, lag, float((err / bound).max()))
            assert (got >= 0.0).all() and (got > 0.0).sum() > f // 4      # (one band alone rises about every other frame)
            worst = max(worst, float((err / bound).max()))
            if max_size == 1 and lag == 1:              # the plain mean of the rectified difference in dB
                plain = 10.0 * np.maximum(0.0, np.diff(l.astype(np.float64), axis=1)).mean(axis=0)
                assert np.abs(got - plain).max() <= 1e-5 * max(1.0, plain.max())
    print("n_mels %d: worst error / bound %.4f" % (nm, worst))
    assert worst <= 1.0


# ---- 5. every geometry of lag tiles and workgroups ----
@pytest.mark.parametrize("wt", [16, 256, 272, 384, 1024])
def test_tempogram_geometries(wt):
    worst = 0.0
    for f in (1, 7, 8, 9, 17):
        lag = 2
        l = log_mel(40, f + wt - 1 + lag, wt + f)
        env = emulate(l, f + wt - 1, lag, 3, wt, 0)      # mode 0 of the widened clip
        got = emulate(l, f, lag, 3, wt, 1)
        want, bound = ref.tempogram(env, wt, f)
        err = np.abs(got.astype(np.float64) - want)
        assert (err <= bound).all(), (wt, f, float((err / bound).max()), np.unravel_index(np.argmax(err / bound), err.shape))
        assert (got[0] == 1.0).all() and (np.abs(got) <= 1.0).all()
        worst = max(worst, float((err / bound).max()))
        # mode 2 averages mode 1's values bit for bit
        dev = emulate(l, f, lag, 3, wt, 2)
        pr = _api().tempogram_prior(SR, n_mels=40, win_length=wt)[0]
        decided, r = ref.check_tempo(ref.tempo(got, pr, SR, HOP), dev)
        assert r <= 1.0
    print("Wt %d: worst error / bound %.4f" % (wt, worst))
    assert 0.0 < worst <= 1.0


# ---- 6. silence, a click train ----
def test_an_all_zero_envelope_gives_exact_zeros():
    for l in (np.full((40, 9 + 383 + 1), -10.0, dtype=np.float32), -np.arange(40 * 393, dtype=np.float32).reshape(393, 40).T / 100.0):
        assert (emulate(l, 9 + 383, 1, 1, 384, 0) == 0.0).all()
        tg = emulate(l, 9, 1, 1, 384, 1)
        assert (tg == 0.0).all() and not np.signbit(tg).any()
    # a frame whose window holds one rise only: lag 0 alone
    l = np.full((8, 20 + 15 + 1), -3.0, dtype=np.float32)
    l[:, 20:] = -1.0
    tg = emulate(l, 20, 1, 1, 16, 1)
    live = (tg[0] == 1.0)
    assert live.any() and not live.all() and (tg[1:] == 0.0).all() and (tg[0][~live] == 0.0).all()


def test_a_click_train_of_period_45_frames():
    f, wt, lag = 200, 384, 1
    l = np.full((128, f + wt - 1 + lag), -6.0, dtype=np.float32)
    l[:, 7::45] = -2.0                                  # a rise of 40 dB every 45 frames; the fall is rectified away
    env = emulate(l, f + wt - 1, lag, 1, wt, 0)
    clicks = np.flatnonzero(env)
    assert (np.diff(clicks) == 45).all() and clicks.size >= 12 and np.allclose(env[clicks], 40.0)
    tg = emulate(l, f, lag, 1, wt, 1)
    pr = _api().tempogram_prior(SR, win_length=wt)[0]
    want = ref.tempo(tg, pr, SR, HOP)
    got = emulate(l, f, lag, 1, wt, 2)
    decided, r = ref.check_tempo(want, got)
    print("click train: tau* %d, %.3f bpm, s %.4f, margin %.4f, bound %.3g" % (got[1], got[0], got[2], got[3], want["bound"]))
    assert decided and want["tau"] == 45 and got[1] == 45.0 and got[0] == np.float32(60.0 * SR / (HOP * 45.0)) and got[3] > 1.0 and r <= 1.0
    # ... against the definition on the envelope too, through the tempogram's bound
    t64, b64 = ref.tempogram(env, wt, f)
    chain = ref.tempo(t64, pr, SR, HOP, b64)
    # (where A = 0 the score is log1p(1e6 . 0): the tempogram's bound of 5e-5 moves it by log1p(50), more than the margin -- through
    # the whole chain the clip is not decided by the rule; the lag's own score is held to its own bound)
    assert chain["tau"] == 45 and chain["bounds"][45] < 1e-3 and abs(chain["s"][45] - got[2]) <= chain["bounds"][45] + 2e-6
    assert chain["bound"] > 1.0


# ---- 7. the sanitizer program ----
def test_the_sanitizer_program_of_the_planning_calls(tmp_path):
    """tools/sanitize/tempogram_plan.c: pdmp3_amd/host/clip_tempogram.c's check, window, prior and plan over the refusals and the
    edge values under AddressSanitizer and UBSan, a stand-alone program on the CPU"""
    run_sanitizer_program(tmp_path, "tempogram_plan", ("clip_tempogram.c", "clip_mel_long.c", "clip_mel.c", "clip_stft_long.c", "clip_stft.c"))
