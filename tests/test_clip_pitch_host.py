"""The pitch of clips on the host, no GPU: the refusals of the check, the lag range and the plan against
their restatement, the restatement against the plain double loop, and the kernel's own phases (pdmp3_amd/csrc/pitch_core.h,
compiled here with g++ into tests/host_emul/pitch_emul.cpp and run thread by thread on wave_emul.h's fibers over a poisoned LDS)
against the binary64 definition within the derived bound: impulses at the window's edges and the tiles' edges, noise, a sine
between two lags, a glide, every geometry of lag tiles and workgroups, silence, and item 7's self-consistency of the two modes."""
import ctypes as C

import numpy as np
import pytest

import clip_pitch_ref as ref
import test_clip_cqt_host as tch
from clip_host import build_emul, run_sanitizer_program

LDS_MAX = 160 * 1024 - 64
CAP = 0.1                                          # the share of a test's frames that may be undecided


class PitchParams(C.Structure):                    # include/pdmp3_hip.h pdmp3_pitch_params
    _fields_ = [("n_in", C.c_int64), ("sr", C.c_double), ("threshold", C.c_double), ("n", C.c_int32), ("win", C.c_int32), ("hop", C.c_int32),
                ("tmin", C.c_int32), ("tmax", C.c_int32), ("tiles", C.c_int32), ("ksteps", C.c_int32), ("n_frames", C.c_int32),
                ("frames_wg", C.c_int32), ("channels", C.c_int32), ("out_mode", C.c_int32), ("ext", C.c_uint32), ("span_floats", C.c_uint32),
                ("q_doubles", C.c_uint32), ("lds_bytes", C.c_uint32)]


def _api():
    from pdmp3_amd import api
    return api


def _emul():
    lib = build_emul("pitch")
    lib.emul_clip_pitch.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.emul_pitch_at.restype = C.c_uint
    assert lib.emul_pitch_params_bytes() == C.sizeof(PitchParams) and lib.emul_pitch_desc_bytes() == C.sizeof(tch.MelDesc)
    return lib


def geometry(sr, n, w, hop, tmin, tmax, threshold=0.1):
    """the call's arguments that give these lags at sr: the quotients lie half a sample from an integer"""
    g = dict(sample_rate=sr, frame_length=n, win_length=w, hop=hop, fmin=sr / (tmax - 0.5), fmax=sr / (tmin + 0.5), threshold=threshold)
    if tmax == n - w - 1:
        g["fmin"] = sr / (tmax + 10.5)               # (the frame's own limit is what holds)
    got = _api().pitch_lags(**{k: v for k, v in g.items() if k != "threshold"})
    assert got[:2] == (tmin, tmax), (got, tmin, tmax)
    return g


def lds_bytes(n, w, hop, tmax, frames):
    """the restatement of the plan's LDS (include/pdmp3_bulk.h pdmp3_amd_pitch_plan) -> (ext, span floats, bytes)"""
    tiles, ksteps = (tmax + 256) // 256, (w + 18) // 4
    reach, first = 4 * (ksteps + 1) + 240 + 256 * (tiles - 1), (frames - 1) * hop
    ext = 16 + first + max(reach, n)
    span = (ext + 2 * (ext >> 4) + 3) & ~3
    doubles = span // 2 + first + n + 1 + 64 * frames + 64
    return ext, span, ((2 * doubles + frames * (256 * tiles + 8) + 4 * frames) * 4 + 15) & ~15


def params_of(g, f, mode, t):
    api = _api()
    kw = {k: v for k, v in g.items() if k != "threshold"}
    sr = kw.pop("sample_rate")
    tmin, tmax, tiles = api.pitch_lags(sr, **kw)
    frames, span, lds, ksteps = api.pitch_plan(sr, **kw)
    n, w, hop = ref.defaults(g["frame_length"], g["win_length"], g["hop"])
    ext, span2, lds2 = lds_bytes(n, w, hop, tmax, frames)
    assert (span, lds) == (span2, lds2)
    return PitchParams(t, float(sr), g["threshold"], n, w, hop, tmin, tmax, tiles, ksteps, f, frames, 1, mode, ext, span, (frames - 1) * hop + n + 1, lds)


def row_of(y, start, n, hop, f):
    """the stream y (binary32, the time line from 0 on) as the call's row for a clip at `start` -> (row [T], lead)"""
    s0 = max(0, start - n // 2)
    t = (f - 1) * hop + n
    row = np.zeros(t, dtype=np.float32)
    part = np.asarray(y[s0:s0 + t], dtype=np.float32)
    row[:part.size] = part
    return row, s0 - (start - n // 2)


def emulate(row, lead, g, f):
    """-> (pitch [3, f], curve [tmax + 1, f]) of the emulated kernel, one channel"""
    t = row.size
    ts = (t + 3) & ~3
    src = np.full(ts, 7e29, dtype=np.float32)        # (the floats behind a row's end are not the kernel's to read)
    src[:t] = row
    outs = []
    for mode in (0, 1):
        P = params_of(g, f, mode, t)
        rows = 3 if mode == 0 else P.tmax + 1
        out = np.full(rows * f + 8, -5.0, dtype=np.float32)
        d = tch.MelDesc(src.ctypes.data, out.ctypes.data, ts, rows * f + 8, lead, 0)
        assert _emul().emul_clip_pitch(C.byref(d), 1, C.byref(P)) == 0, "the emulated kernel read LDS it must not read"
        assert (out[rows * f:] == -5.0).all()
        outs.append(out[:rows * f].reshape(rows, f).copy())
    return outs[0], outs[1]


def run_and_check(row, lead, g, f, tmin, tmax):
    """emulate, hold every value to its bound and every frame to item 7 -> (worst error / bound, undecided, frames with signal)"""
    n, w, hop = ref.defaults(g["frame_length"], g["win_length"], g["hop"])
    pitch, curve = emulate(row, lead, g, f)
    res = ref.check(row, lead, float(g["sample_rate"]), n, w, hop, f, tmin, tmax, g["threshold"], pitch, curve)
    ulps = ref.self_consistent(row, lead, g["sample_rate"], n, hop, f, tmin, tmax, g["threshold"], pitch, curve)
    assert ulps == 0, "plane 0 is not numpy's binary64 evaluation of rule 6 rounded once (%d ulp)" % ulps
    return res


# ---- 1. the check ----
def test_the_checks_refusals_one_by_one():
    api = _api()
    ok = dict(frame_length=2048, hop=512, fmin=65.406, fmax=2093.0, threshold=0.1)
    assert api.pitch_check(22050, **ok)
    assert api.pitch_check(22050) and api.pitch_check(22050, frame_length=64, fmin=700.0, fmax=11025.0)
    for bad in (dict(frame_length=2047), dict(frame_length=62), dict(frame_length=2050), dict(frame_length=4096), dict(win_length=3),
                dict(win_length=2047), dict(hop=2049), dict(hop=-1), dict(fmin=0.0), dict(fmin=-3.0), dict(fmin=float("nan")),
                dict(fmax=65.406), dict(fmax=60.0), dict(fmax=11025.1), dict(fmax=float("inf")), dict(threshold=0.0), dict(threshold=1.5),
                dict(threshold=float("nan")), dict(out_mode=2), dict(out_mode=-1), dict(out_mode="contour"), dict(n_frames=-1),
                dict(frame_length=64, win_length=61, hop=16, fmax=8000.0)):           # tmin 2 >= tmax 2 = N - W - 1
        assert not api.pitch_check(22050, **dict(ok, **bad)), bad
    # the narrowest ranges that pass: two lags from the frequencies, two from the frame
    assert api.pitch_lags(22050, **dict(ok, fmin=2000.0)) == (10, 12, 1)
    assert api.pitch_lags(22050, frame_length=64, win_length=60, hop=16, fmin=65.406, fmax=8000.0) == (2, 3, 1)
    assert not api.pitch_check(0, **ok) and api.pitch_check(22050, **dict(ok, threshold=1.0, out_mode="curve", win_length=4))


# ---- 2. the lags ----
def test_lags_against_the_restatement():
    api = _api()
    n, w = 2048, 1024
    count = 0
    for sr in (8000, 11025, 16000, 22050, 32000, 44100, 48000):
        for fmin in (20.0, 31.25, 50.0, 65.406, 100.0, 110.0, 441.0, 1000.0):
            for fmax in (80.0, 125.0, 400.0, 1000.0, 2093.0, 4000.0, 5512.5, sr / 2.0):
                want = ref.lags(sr, fmin, fmax, n, w)
                kw = dict(frame_length=n, fmin=fmin, fmax=fmax)
                assert api.pitch_check(sr, **kw) == (want is not None), (sr, fmin, fmax, want)
                if want is not None:
                    assert api.pitch_lags(sr, **kw) == want, (sr, fmin, fmax)
                    count += 1
    assert count > 150
    # quotients that are exact integers
    assert api.pitch_lags(16000, frame_length=1024, fmin=100.0, fmax=4000.0) == (4, 160, 1) == ref.lags(16000, 100.0, 4000.0, 1024, 512)
    assert api.pitch_lags(8000, frame_length=1024, fmin=31.25, fmax=2000.0) == (4, 256, 2) == ref.lags(8000, 31.25, 2000.0, 1024, 512)
    # ... and quotients that are not, closer to one than 1e-9: nothing is known about their side
    for kw in (dict(fmin=100.0 * (1 + 1e-13), fmax=4000.0), dict(fmin=100.0, fmax=4000.0 * (1 - 1e-13))):
        assert ref.lags(16000, kw["fmin"], kw["fmax"], 1024, 512) is None and not api.pitch_check(16000, frame_length=1024, **kw)
    assert api.pitch_lags(16000, frame_length=1024, fmin=100.0 * (1 - 1e-8), fmax=4000.0)[1] == 161
    assert api.pitch_lags(22050) == (10, 338, 2)


# ---- 3. the plan ----
@pytest.mark.parametrize("n", [64, 256, 2048])
def test_the_plan_over_all_hops(n):
    api = _api()
    seen = set()
    tmax = api.pitch_lags(8000, frame_length=n, fmin=30.0, fmax=4000.0)[1]
    assert tmax == min(n - n // 2 - 1, 267)
    for hop in range(1, n + 1):
        frames, span, lds, ksteps = api.pitch_plan(8000, frame_length=n, hop=hop, fmin=30.0, fmax=4000.0)
        assert frames in (8, 4, 2, 1) and lds <= LDS_MAX and ksteps == (n // 2 + 18) // 4
        assert (span, lds) == lds_bytes(n, n // 2, hop, tmax, frames)[1:]
        assert frames == 8 or lds_bytes(n, n // 2, hop, tmax, 2 * frames)[2] > LDS_MAX
        seen.add(frames)
    assert seen == ({8, 4} if n == 2048 else {8}), seen
    with pytest.raises(ValueError):
        api.pitch_plan(8000, frame_length=n, hop=n + 1, fmin=30.0, fmax=4000.0)


def test_the_span_layout_keeps_the_operands_apart():
    at = _emul().emul_pitch_at
    assert [at(x) for x in (0, 15, 16, 31, 32, 256)] == [0, 15, 18, 33, 36, 288]
    for base in range(0, 40):
        for ks in range(0, 5):
            # half a wave of the A operand: rows m = 0 .. 15 at k = 0, 1: 32 banks of a 4-byte read, each once
            banks = sorted(at(base + 4 * ks + kq + 16 * m) % 32 for m in range(16) for kq in (0, 1))
            assert banks == list(range(32)), (base, ks)
            banks = sorted(at(base + 4 * ks + kq + 16 * m) % 32 for m in range(16) for kq in (2, 3))
            assert banks == list(range(32)), (base, ks)
            # the B operand: 17 consecutive positions, every one in a bank of its own
            pos = sorted(set(base + 16 + 4 * ks + kq - j for j in range(16) for kq in (0, 1)))
            assert len(set(at(p) % 32 for p in pos)) == len(pos) == 17


# ---- 4. the restatement ----
def test_the_restatement_is_the_plain_double_loop():
    rng = np.random.default_rng(5)
    for n, w, tmax in ((64, 32, 31), (256, 127, 128), (256, 100, 60)):
        z = rng.standard_normal(n).astype(np.float32).astype(np.float64)
        dp, bound = ref.curve(z, w, tmax)
        assert np.abs(dp - ref.plain_curve(z, w, tmax)).max() <= 1e-12
        assert dp[0] == 1.0 and bound[0] == 0.0 and (bound[1:] > 0).all() and bound[1:].max() < 1e-3
    assert (ref.curve(np.zeros(64), 32, 31)[0] == 1.0).all() and (ref.curve(np.zeros(64), 32, 31)[1] == 0.0).all()
    assert ref.decide(np.array([1.0, 1.0, 0.5, 0.05, 0.04, 0.3, 0.02, 1.0]), 1, 7, 0.1) == 4
    assert ref.decide(np.array([1.0, 1.0, 0.5, 0.25, 0.24, 0.3, 0.2, 0.2]), 1, 7, 0.1) == 6
    assert ref.decide(np.array([1.0, 0.01, 0.5, 0.25, 0.24, 0.3, 0.2, 0.2]), 1, 7, 0.1) == 1


# ---- 5. impulses at the window's and the tiles' edges ----
@pytest.mark.parametrize("p_name", ["0", "W-2", "W-1", "W"])
def test_two_unit_impulses(p_name):
    n, w, tmin, tmax, sr = 1024, 512, 2, 511, 16000
    g = geometry(sr, n, w, 256, tmin, tmax)
    p = {"0": 0, "W-2": w - 2, "W-1": w - 1, "W": w}[p_name]
    for tau0 in (1, 15, 16, 17, 255, 256, 257, tmax):
        y = np.zeros(n, dtype=np.float32)
        y[p] = y[p + tau0] = 1.0
        row, lead = row_of(y, n // 2, n, 256, 1)
        assert lead == 0 and (row == y).all()
        pitch, curve = emulate(row, lead, g, 1)
        dp, bound = ref.curve(y.astype(np.float64), w, tmax)
        # r and e are exact integers on both sides: the curve is the definition's up to the one rounding of the quotient
        want = dp.astype(np.float32)
        ulp = np.abs(curve[:, 0].view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
        assert ulp.max() <= 1, (p, tau0, int(ulp.max()), int(np.argmax(ulp)))
        assert ref.self_consistent(row, lead, sr, n, 256, 1, tmin, tmax, 0.1, pitch, curve) == 0
        # an impulse at the window's edge: with the edge one sample off, d' is off by far more than a hundred bounds
        if p + tau0 >= w - 1 or p >= w - 1:
            fin = np.isfinite(bound)
            moved = max(np.abs(ref.curve(y.astype(np.float64), w + s, tmax)[0] - dp)[fin].max() for s in (-1, 1))
            assert moved > 100.0 * bound[fin].max(), (p, tau0, moved, bound[fin].max())


# ---- 6. noise, a sine between two lags, a glide ----
def glide(sr=22050, seconds=2.1, seed=11):
    """one second of noise, then five harmonics gliding from 110 to 440 Hz over a 1 % noise floor"""
    rng = np.random.default_rng(seed)
    t = np.arange(int(seconds * sr)) / sr
    f = 110.0 * (440.0 / 110.0) ** np.clip((t - 1.0) / (seconds - 1.0), 0.0, 1.0)
    ph = 2.0 * np.pi * np.cumsum(f) / sr
    y = sum(np.sin(h * ph) / h for h in range(1, 6)) * 0.3 + 0.003 * rng.standard_normal(t.size)
    y[:sr] = 0.1 * rng.standard_normal(sr)
    return y.astype(np.float32)


def test_noise_within_the_bound():
    g = geometry(16000, 1024, 512, 256, 4, 400)
    y = (0.2 * np.random.default_rng(3).standard_normal(9 * 256 + 1024)).astype(np.float32)
    row, lead = row_of(y, 700, 1024, 256, 10)
    worst, und, live = run_and_check(row, lead, g, 10, 4, 400)
    print("noise: worst error / bound %.4f, %d of %d frames undecided" % (worst, und, live))
    assert 0.0 < worst <= 1.0 and live == 10 and und <= CAP * live


def test_a_sine_with_period_100_5_samples():
    """The period lies half way between two lags: d'(100) and d'(101) differ by a hundredth of themselves, about 5e-6, a fifth of
    the bound that the chain of 516 binary32 additions allows them -- which of the two is the trough is undecided against the
    binary64 definition on every frame, by construction.  So this signal is held to what undecided frames are held to -- the
    whole curve within its bound, item 7 -- and to the refinement finding the half sample; the share is printed, not capped."""
    g = geometry(16000, 1024, 512, 256, 4, 400)
    y = (0.5 * np.sin(2.0 * np.pi * np.arange(12 * 256 + 1024) / 100.5)).astype(np.float32)
    row, lead = row_of(y, 800, 1024, 256, 12)
    pitch, curve = emulate(row, lead, g, 12)
    worst, und, live = run_and_check(row, lead, g, 12, 4, 400)
    print("sine: worst error / bound %.4f, %d of %d frames undecided; f0 %s" % (worst, und, live, pitch[0, :4]))
    assert 0.0 < worst <= 1.0 and live == 12
    assert (np.abs(pitch[0] - 16000 / 100.5) < 0.05).all() and ((pitch[2] == 100) | (pitch[2] == 101)).all() and (pitch[1] < 0.01).all()


def test_the_glide_at_the_defaults():
    sr = 22050
    g = dict(sample_rate=sr, frame_length=2048, win_length=None, hop=512, fmin=65.406, fmax=2093.0, threshold=0.1)
    y = glide()
    f = 64
    row, lead = row_of(y, sr // 2, 2048, 512, f)
    worst, und, live = run_and_check(row, lead, g, f, 10, 338)
    pitch, _ = emulate(row, lead, g, f)
    print("glide: worst error / bound %.4f, %d of %d frames undecided; f0 from %.1f to %.1f" % (worst, und, live, pitch[0, 30], pitch[0, -1]))
    assert 0.0 < worst <= 1.0 and live == f and und <= CAP * live
    voiced = pitch[1, 26:] < 0.1
    assert voiced.all() and (np.diff(pitch[0, 26:]) > 0).all() and 110.0 <= pitch[0, 26] < 160.0 and 300.0 < pitch[0, -1] <= 440.0


# ---- 7. every geometry of lag tiles and workgroups ----
GEOMETRIES = [(64, 32, 31, 16), (256, 127, 128, 64), (1024, 512, 255, 256), (1024, 512, 256, 256), (1024, 512, 511, 256),
              (2048, 1024, 338, 512), (2048, 513, 1023, 2048)]


@pytest.mark.parametrize("n,w,tmax,hop", GEOMETRIES, ids=["%d-%d-%d-%d" % t for t in GEOMETRIES])
def test_geometries(n, w, tmax, hop):
    sr, tmin = (22050, 10) if (n, w, tmax) == (2048, 1024, 338) else (16000, 2)
    g = geometry(sr, n, w, hop, tmin, tmax) if tmax != 338 else dict(sample_rate=sr, frame_length=n, win_length=w, hop=hop, fmin=65.406,
                                                                     fmax=2093.0, threshold=0.1)
    tiles = _api().pitch_lags(**{k: v for k, v in g.items() if k != "threshold"})[2]
    assert tiles == {31: 1, 128: 1, 255: 1, 256: 2, 511: 2, 338: 2, 1023: 4}[tmax]
    j_all = 9 * hop + n // 2 + 37                    # the stream's samples
    rng = np.random.default_rng(n + tmax)
    t = np.arange(j_all)
    period = min(max(tmin + 3.25, tmax / 2.5), 37.3)     # (a trough sharp enough to be decided: its curvature falls with period^2)
    y = (0.4 * np.sin(2.0 * np.pi * t / period) + 0.2 * np.sin(4.0 * np.pi * t / period + 1.0) + 0.01 * rng.standard_normal(j_all)).astype(np.float32)
    worst, und, live, silent = 0.0, 0, 0, 0
    for f in (1, 7, 8, 9, 17):
        for start in (0, 1, n // 2 - 1, n // 2, j_all + 3 * n):
            row, lead = row_of(y, start, n, hop, f)
            assert lead == max(0, n // 2 - start)
            a, b, c = run_and_check(row, lead, g, f, tmin, tmax)
            worst, und, live = max(worst, a), und + b, live + c
            silent += f - c
    print("N %d W %d tmax %d H %d: worst error / bound %.4f, %d of %d frames undecided, %d frames of zeros" % (n, w, tmax, hop, worst, und, live, silent))
    assert 0.0 < worst <= 1.0 and live > 100 and silent >= 42 and und <= CAP * live


# ---- 8. silence ----
def test_silence_is_exactly_0_1_0():
    g = geometry(16000, 256, 127, 64, 2, 128)
    row = np.zeros(8 * 64 + 256, dtype=np.float32)
    pitch, curve = emulate(row, 0, g, 9)
    assert (pitch[0] == 0.0).all() and (pitch[1] == 1.0).all() and (pitch[2] == 0.0).all() and (curve == 1.0).all()
    row[700] = 1e-30                                 # not silence: the last frames hold one tiny sample
    pitch, curve = emulate(row, 0, g, 9)
    assert (pitch[2, :7] == 0).all() and (pitch[2, 7:] >= 2).all() and (pitch[0, 7:] > 0).all()


# ---- 9. the sanitizer program ----
def test_the_sanitizer_program_of_the_planning_calls(tmp_path):
    """tools/sanitize/pitch_plan.c: pdmp3_amd/host/clip_pitch.c's check, lags and plan over the refusals and the edge cases under
    AddressSanitizer and UBSan, a stand-alone program on the CPU"""
    run_sanitizer_program(tmp_path, "pitch_plan", ("clip_pitch.c",))
