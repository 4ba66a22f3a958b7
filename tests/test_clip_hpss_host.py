"""Harmonic-percussive separation of clips, the part that needs no GPU: the check and the plan of
pdmp3_amd/host/clip_hpss.c against the restatement (tests/clip_hpss_ref.py), their refusals, and k_clip_hpss's own layout,
reflection, selection network, masks and stores (pdmp3_amd/csrc/hpss_core.h, compiled here with g++ into
tests/host_emul/hpss_emul.cpp's loops) on random float32 spectrograms: the medians bit for bit against np.sort, the masks within
the rounding's bound (exactly at power inf), the modes against each other bit for bit -- no value left out."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import clip_hpss_ref as href
import clip_stft_ref as sref
from clip_host import MelDesc, build_emul, run_sanitizer_program

GUARD_VALUE = np.float32(-3e9)
INF = float("inf")
SIZES = [(31, 31), (3, 31), (31, 3), (17, 5)]


class HpssParams(C.Structure):                     # include/pdmp3_hip.h pdmp3_hpss_params
    _fields_ = [("n_fft", C.c_int32), ("bins", C.c_int32), ("n_frames", C.c_int32), ("n_stage", C.c_int32), ("kernel_harm", C.c_int32),
                ("kernel_perc", C.c_int32), ("tile_bins", C.c_int32), ("tile_frames", C.c_int32), ("pitch", C.c_int32), ("channels", C.c_int32),
                ("out_mode", C.c_int32), ("power", C.c_int32), ("margin_harm", C.c_double), ("margin_perc", C.c_double), ("lds_bytes", C.c_uint32),
                ("pad_", C.c_uint32)]


def _emul():
    lib = build_emul("hpss")
    lib.emul_clip_hpss.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.emul_hpss_lds_floats.restype = C.c_uint
    lib.emul_hpss_lds_at.restype = C.c_uint
    lib.emul_hpss_centre.restype = C.c_uint
    lib.emul_hpss_median.restype = C.c_float
    lib.emul_hpss_median.argtypes = [C.c_void_p, C.c_int, C.c_int]
    assert lib.emul_hpss_desc_bytes() == C.sizeof(MelDesc) and lib.emul_hpss_params_bytes() == C.sizeof(HpssParams)
    return lib


def _params(n_fft, f, lh, lp, power, margins, mode, channels, over=()):
    from pdmp3_amd import api
    front, back, tb, tf, pitch, lds = api.hpss_plan(lh, lp)
    assert front == back == lh // 2
    p = dict(n_fft=n_fft, bins=n_fft // 2 + 1, n_frames=f, n_stage=f + front + back, kernel_harm=lh, kernel_perc=lp, tile_bins=tb, tile_frames=tf,
             pitch=pitch, channels=channels, out_mode=mode, power=0 if math.isinf(power) else int(power), margin_harm=margins[0],
             margin_perc=margins[1], lds_bytes=lds)
    return HpssParams(**dict(p, **dict(over)))


def _emul_run(stage, f, lh, lp, power=2.0, margins=(1.0, 1.0), mode=0, n_fft=2048):
    """stage: float32 [C, K, F + 2 rh] magnitudes (mode 2: [C, K, F + 2 rh, 2]) -> the emulator's [C, 2, K, F] (mode 2: [.., 2])"""
    lib = _emul()
    channels, k = stage.shape[0], stage.shape[1]
    e = 2 if mode == 2 else 1
    assert k == n_fft // 2 + 1 and stage.shape[2] == f + lh - 1 and stage.dtype == np.float32 and stage.flags.c_contiguous
    per = 2 * k * f * e
    out = np.full((channels, per + 8), GUARD_VALUE, dtype=np.float32)
    d = MelDesc(src=stage.ctypes.data, dst=out.ctypes.data, src_chan_stride=stage[0].size, dst_chan_stride=per + 8, lead=0)
    P = _params(n_fft, f, lh, lp, power, margins, mode, channels)
    assert lib.emul_clip_hpss(C.byref(d), 1, C.byref(P)) == 0
    assert (out[:, per:] == GUARD_VALUE).all() and (out[:, :per] != GUARD_VALUE).all()
    return out[:, :per].reshape((channels, 2, k, f) + ((2,) if e == 2 else ()))


@functools.lru_cache(maxsize=None)
def _spectrogram(n_fft, f, lh, seed=5):
    """random float32 magnitudes [2, K, F + Lh - 1] with what a selection can trip over: ties (values drawn from a few), zeros,
    denormal magnitudes, rows and frames of silence, a frame with a single nonzero bin"""
    rng = np.random.default_rng(seed + n_fft + 7 * f + lh)
    k, fs = n_fft // 2 + 1, f + lh - 1
    s = (rng.random((2, k, fs), dtype=np.float32) * np.float32(3.0)).astype(np.float32)
    s[:, 100:260] = rng.choice(np.array([0.0, 0.25, 0.5, 1.0, 2.0], dtype=np.float32), size=(2, 160, fs))       # ties and zeros
    s[:, 300:420] *= np.float32(1e-41)                                                                              # denormal magnitudes
    s[:, 420:440] = rng.choice(np.array([0.0, 1e-45, 3e-45, 1.2e-38], dtype=np.float32), size=(2, 20, fs))
    s[:, 500:600] = 0.0                                                                                             # silence: a band ..
    s[:, :, 20:24] = 0.0                                                                                            # .. and frames
    s[:, :, 40] = 0.0
    s[:, 777, 40] = 1.5                                                                                             # a single nonzero bin
    s[0, :, fs - 3] = 0.0
    s[0, k - 1, fs - 3] = 2.5                                                                                       # ... the last one
    s[1, :40] = np.float32(1e30)                                                                                    # large values
    return s


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_refusals_write_nothing():
    from pdmp3_amd import api
    lib = api.load_library()
    assert api.HPSS_MODES == {m: i for i, m in enumerate(href.MODES)}
    assert api.hpss_check(22050) and api.hpss_check(48000, n_fft=4096, hop=1024, power=INF) and api.hpss_check(44100, hop=1, power=1.0)
    assert api.hpss_check(44100, hop=2048, kernel_size=(3, 31), margin=(2.0, 3.5), mode="complex")
    assert api.hpss_check(22050, win_length=1764, window=np.ones(1764, dtype=np.float32), kernel_size=(17, 5), mode="median")
    assert api.hpss_check(22050, n_fft=4096, hop=4096, n_frames=0, mode="magnitude", margin=1e300)
    bad_window = np.ones(2048, dtype=np.float32)
    bad_window[77] = np.nan
    nan = float("nan")
    refused = [dict(n_fft=1024), dict(n_fft=8192), dict(n_fft=2047), dict(n_fft=400), dict(n_fft=0), dict(hop=0), dict(hop=2049),
               dict(n_fft=4096, hop=4097), dict(hop=-1), dict(win_length=2049), dict(win_length=-1), dict(window=bad_window), dict(n_frames=-1),
               dict(kernel_size=30), dict(kernel_size=32), dict(kernel_size=33), dict(kernel_size=1), dict(kernel_size=0), dict(kernel_size=-31),
               dict(kernel_size=(31, 2)), dict(kernel_size=(4, 31)), dict(kernel_size=(31, 33)), dict(kernel_size=(35, 3)), dict(kernel_size=30.5),
               dict(margin=0.5), dict(margin=(1.0, 0.999)), dict(margin=(0.0, 1.0)), dict(margin=nan), dict(margin=INF), dict(margin=(1.0, -INF)),
               dict(power=0.0), dict(power=0.5), dict(power=1.5), dict(power=3.0), dict(power=-2.0), dict(power=nan), dict(power=-INF),
               dict(mode=4), dict(mode=-1), dict(mode="power"), dict(n_frames=2 ** 31 // 2050 + 1), dict(mode=2, n_frames=2 ** 31 // 4100 + 1)]
    for bad in refused:
        assert not api.hpss_check(22050, **bad), bad
    assert not api.hpss_check(0) and not api.hpss_check(-1)
    assert lib.pdmp3_amd_hpss_check(None, 22050) == -1
    for lh, lp in ((30, 31), (31, 32), (1, 3), (3, 1), (33, 3), (3, 33), (0, 0), (-3, 3)):
        with pytest.raises(ValueError):
            api.hpss_plan(lh, lp)
        v = [C.c_int(-5 - i) for i in range(5)]
        b = C.c_uint(77)
        assert lib.pdmp3_amd_hpss_plan(lh, lp, *[C.byref(x) for x in v], C.byref(b)) == -1
        assert [x.value for x in v] == [-5, -6, -7, -8, -9] and b.value == 77
    assert lib.pdmp3_amd_hpss_plan(31, 31, None, None, None, None, None, None) == 0
    spec, keep = api._hpss_spec()
    assert lib.pdmp3_amd_bulk_decode_clips_hpss(None, None, 0, C.byref(spec), None) == -1
    # the spectrum call's check: what it accepted and refused before
    assert api.stft_long_check(44100) and api.stft_long_check(48000, n_fft=4096, hop=4096, mode="log10")
    for bad in (dict(n_fft=1024), dict(hop=0), dict(hop=2049), dict(win_length=2049), dict(window=bad_window), dict(mode=5), dict(n_frames=-1)):
        assert not api.stft_long_check(44100, **bad), bad


def test_the_plan_is_the_restated_one_and_both_windows_and_the_load_meet_every_bank_once():
    from pdmp3_amd import api
    lib = _emul()
    for lh in range(3, 32, 2):
        for lp in range(3, 32, 2):
            got = api.hpss_plan(lh, lp)
            assert got == href.plan(lh, lp), (lh, lp)
            assert got[4] == lib.emul_hpss_pitch() and got[5] == 4 * lib.emul_hpss_lds_floats() and got[5] <= 64 * 1024
    assert api.hpss_plan(31, 31) == (15, 15, 64, 64, 94, 35344) and api.hpss_plan(3, 17)[:2] == (1, 1)
    # the banks (cdna_hip_programming: a 4-byte LDS access is served 32 lanes at a time over 32 banks): every step of both
    # windows and every store of the load, for every bin of the tile and every wave, puts a group's 32 lanes on 32 banks
    floats = lib.emul_hpss_lds_floats()
    centres = [[lib.emul_hpss_centre(b, lane) for lane in range(64)] for b in range(64)]
    for lh, lp in SIZES + [(3, 3), (5, 29)]:
        rh, rp, pitch = lh // 2, lp // 2, lib.emul_hpss_pitch()
        seen = set()
        for b in range(64):
            centre = centres[b]
            for step in [o for o in range(-15, 16)] + [o * pitch for o in range(-15, 16)]:
                at = [c + step for c in centre]
                assert min(at) >= 0 and max(at) < floats                     # all 31 places of both windows lie inside the LDS
                for half in (at[:32], at[32:]):
                    assert len({a % 32 for a in half}) == 32, (lh, lp, b, step)
        for r in range(64 + 2 * rp):
            for c0 in range(0, 64 + 2 * rh, 64):
                at = [lib.emul_hpss_lds_at(r, c, rh, rp) for c in range(c0, min(c0 + 64, 64 + 2 * rh))]
                assert max(at) < floats and not seen & set(at)
                seen |= set(at)
                for half in (at[:32], at[32:]):
                    assert len({a % 32 for a in half}) == len(half)
        # what the windows of these sizes read is what the load wrote
        need = {centres[b][lane] + o for b in range(64) for lane in range(64) for o in range(-rh, rh + 1)}
        need |= {centres[b][lane] + o * pitch for b in range(64) for lane in range(64) for o in range(-rp, rp + 1)}
        assert need <= seen


def test_the_reflection_at_both_ends():
    lib = _emul()
    for k in (1025, 2049):
        for i in range(-20, k + 20):
            assert lib.emul_hpss_reflect(i, k) == href.reflect(i, k), i
        assert [lib.emul_hpss_reflect(i, k) for i in (-2, -1, 0, 1)] == [1, 0, 0, 1]
        assert [lib.emul_hpss_reflect(i, k) for i in (k - 2, k - 1, k, k + 1)] == [k - 2, k - 1, k - 1, k - 2]
        pad = np.pad(np.arange(k), (15, 15), mode="symmetric")
        assert [lib.emul_hpss_reflect(i, k) for i in range(-15, k + 15)] == pad.tolist()
        assert all(0 <= lib.emul_hpss_reflect(i, k) < k for i in range(-3 * k, 4 * k, 97))          # (the clamp: never outside)


def test_the_selection_network_on_single_windows():
    """every odd size, both steps: ties, zeros, denormals, one nonzero value, sorted and reversed windows, whatever lies outside"""
    lib = _emul()
    rng = np.random.default_rng(31)
    pitch = lib.emul_hpss_pitch()
    pools = [np.array([0.0, 1.0], dtype=np.float32), np.array([0.0, 1e-45, 2e-45, 1.2e-38, 3.0], dtype=np.float32), None]
    for r in range(1, 16):
        for trial in range(40):
            pool = pools[trial % 3]
            w = rng.random(31, dtype=np.float32) if pool is None else rng.choice(pool, size=31)
            if trial == 3:
                w = np.sort(w)
            if trial == 4:
                w = np.sort(w)[::-1].copy()
            if trial == 5:
                w[:] = 0.0
                w[15 + rng.integers(-r, r + 1)] = 7.0
            want = np.sort(w[15 - r:16 + r])[r]
            outside = np.array([np.nan, -1.0, 3e38, -np.inf], dtype=np.float32)[trial % 4]
            row = w.copy()
            row[:15 - r] = outside
            row[16 + r:] = outside
            assert _bits(lib.emul_hpss_median(row.ctypes.data, 1, r)) == _bits(want), (r, trial)
            col = np.full(31 * pitch, outside, dtype=np.float32)
            col[(15 - r) * pitch:(16 + r) * pitch:pitch] = w[15 - r:16 + r]
            assert _bits(lib.emul_hpss_median(col.ctypes.data, pitch, r)) == _bits(want), (r, trial)


@pytest.mark.parametrize("lh,lp", SIZES, ids=lambda v: str(v))
def test_medians_are_exact_against_np_sort(lh, lp):
    f = 70                                          # one full tile of frames and a partial one; K = 64 x 16 + 1: a last tile of one bin
    s = _spectrogram(2048, f, lh)
    got = _emul_run(s, f, lh, lp, mode=3)
    hm, pm = href.medians(s, lh, lp)
    assert hm.dtype == np.float32 and np.array_equal(_bits(got[:, 0]), _bits(hm)) and np.array_equal(_bits(got[:, 1]), _bits(pm))
    assert (hm[:, 300:420] > 0).any() and (hm[:, 300:420] < 1.2e-38).all()          # denormal medians come through as they are
    # rho at bins 0, 1, K - 2, K - 1, spelled out
    k, rh, rp = 1025, lh // 2, lp // 2
    for b in (0, 1, k - 2, k - 1):
        rows = [href.reflect(i, k) for i in range(b - rp, b + rp + 1)]
        want = np.sort(s[:, rows, rh:rh + f], axis=1)[:, rp]
        assert np.array_equal(_bits(got[:, 1, b]), _bits(want)), b


def test_medians_against_scipy_away_from_the_time_edges():
    ndi = pytest.importorskip("scipy.ndimage")
    for lh, lp in ((31, 31), (17, 5)):
        f, rh = 70, lh // 2
        s = _spectrogram(2048, f, lh)
        got = _emul_run(s, f, lh, lp, mode=3)
        for ch in range(2):
            hm = ndi.median_filter(s[ch], size=(1, lh), mode="reflect")[:, rh:rh + f]         # (its time edges are cut off: no reflection is seen)
            pm = ndi.median_filter(s[ch], size=(lp, 1), mode="reflect")[:, rh:rh + f]
            assert np.array_equal(_bits(got[ch, 0]), _bits(hm)) and np.array_equal(_bits(got[ch, 1]), _bits(pm))


def _stated_mask(x32, o32, margin, power, unit):
    """hpss_core.h's hpss_mask operation by operation in numpy's binary64, rounded once to binary32"""
    x, r = x32.astype(np.float64), margin * o32.astype(np.float64)
    if math.isinf(power):
        return (x > r).astype(np.float32)
    a, b = (x * x, r * r) if power == 2.0 else (x, r)
    with np.errstate(invalid="ignore", over="ignore"):
        m = (a / (a + b)).astype(np.float32)
    return np.where(np.maximum(x, r) < 2.0 ** -126, np.float32(0.5 if unit else 0.0), m)


@pytest.mark.parametrize("margins", [(1.0, 1.0), (2.0, 3.5)], ids=["margins-1-1", "margins-2-3.5"])
@pytest.mark.parametrize("power", [1.0, 2.0, INF], ids=["power-1", "power-2", "power-inf"])
def test_masks_within_the_roundings_bound_and_exact_at_inf(power, margins):
    lh, lp, f = 17, 5, 70
    s = _spectrogram(2048, f, lh)
    got = _emul_run(s, f, lh, lp, power, margins, mode=0)
    med = _emul_run(s, f, lh, lp, power, margins, mode=3)
    want, bound = href.from_medians(med[:, 0], med[:, 1], margins[0], margins[1], power)
    err = np.abs(got.astype(np.float64) - want)
    assert (err <= bound).all(), (float((err - bound).max()), np.unravel_index(np.argmax(err - bound), err.shape))
    print("power %s margins %s: worst |mask - binary64| / bound %.4f" % (power, margins, float((err / np.maximum(bound, 1e-300)).max())))
    if math.isinf(power):
        assert np.array_equal(got, want.astype(np.float32)) and set(np.unique(got)) == {0.0, 1.0}
    unit = margins == (1.0, 1.0)
    # mode 0 is the stated function of mode 3, bit for bit
    stated = np.stack([_stated_mask(med[:, 0], med[:, 1], margins[0], power, unit), _stated_mask(med[:, 1], med[:, 0], margins[1], power, unit)], axis=1)
    assert np.array_equal(_bits(got), _bits(stated))
    # silence (both medians below 2^-126): 0.5 with unit margins at a finite power, else 0 -- and it occurs
    silent = np.maximum(med[:, 0].astype(np.float64), med[:, 1].astype(np.float64) * 1.0) == 0.0
    assert silent.sum() > 1000
    expect = np.float32(0.5) if unit and not math.isinf(power) else np.float32(0.0)
    assert (got[:, 0][silent] == expect).all() and (got[:, 1][silent] == expect).all()
    assert np.isfinite(got).all() and (got >= 0).all() and (got <= 1).all()
    if unit and not math.isinf(power):
        both = (med[:, 0] >= 2.0 ** -100) & (med[:, 1] >= 2.0 ** -100) & (med[:, 0] < 1e18)    # (where nothing under- or overflows the sum is 1)
        assert (np.abs(got[:, 0].astype(np.float64) + got[:, 1] - 1.0)[both] <= 2.0 ** -23).all()


def test_a_silent_spectrogram_gives_half_or_zero():
    f = 70
    s = np.zeros((1, 1025, f + 30), dtype=np.float32)
    assert (_emul_run(s, f, 31, 31, 2.0, (1.0, 1.0), 0) == np.float32(0.5)).all()
    assert (_emul_run(s, f, 31, 31, 1.0, (1.0, 1.0), 0) == np.float32(0.5)).all()
    assert (_bits(_emul_run(s, f, 31, 31, 2.0, (2.0, 1.0), 0)) == 0).all()
    assert (_bits(_emul_run(s, f, 31, 31, INF, (1.0, 1.0), 0)) == 0).all()
    assert (_bits(_emul_run(s, f, 31, 31, 2.0, (1.0, 1.0), 1)) == 0).all() and (_bits(_emul_run(s, f, 31, 31, 2.0, (1.0, 1.0), 3)) == 0).all()
    tiny = np.full((1, 1025, f + 30), np.float32(1e-39), dtype=np.float32)                    # below 2^-126, not zero
    assert (_emul_run(tiny, f, 31, 31, 2.0, (1.0, 1.0), 0) == np.float32(0.5)).all()
    assert (_bits(_emul_run(tiny, f, 31, 31, 2.0, (1.0, 1.5), 0)) == 0).all()


@pytest.mark.parametrize("n_fft", [2048, 4096])
def test_the_modes_agree_bit_for_bit(n_fft):
    lh, lp, f, power, margins = 5, 7, 66, 2.0, (1.0, 1.0)
    rng = np.random.default_rng(n_fft)
    k = n_fft // 2 + 1
    z = (rng.standard_normal((2, k, f + lh - 1, 2)) * 2.0).astype(np.float32)
    z[:, 200:260] = 0.0
    z[:, :, 30] *= np.float32(1e-22)                                                          # (powers that leave binary32's normal range)
    re, im = z[..., 0], z[..., 1]
    mag = np.sqrt(sref.power_as_the_product(re, im))                                           # sqrtf(fma(im, im, re re)), as the spectrum call's mode 1
    assert mag.dtype == np.float32
    m0 = _emul_run(mag, f, lh, lp, power, margins, 0, n_fft)
    m1 = _emul_run(mag, f, lh, lp, power, margins, 1, n_fft)
    m2 = _emul_run(z, f, lh, lp, power, margins, 2, n_fft)
    m3 = _emul_run(mag, f, lh, lp, power, margins, 3, n_fft)
    rh = lh // 2
    centre = mag[:, None, :, rh:rh + f]
    assert np.array_equal(_bits(m1), _bits(centre * m0))
    # mode 2 forms the same magnitudes from the pair on its way in
    assert np.array_equal(_bits(m2), _bits(z[:, None, :, rh:rh + f] * m0[..., None]))
    hm, pm = href.medians(mag, lh, lp)
    assert np.array_equal(_bits(m3[:, 0]), _bits(hm)) and np.array_equal(_bits(m3[:, 1]), _bits(pm))
    want0, bound = href.from_medians(m3[:, 0], m3[:, 1], 1.0, 1.0, power)
    assert (np.abs(m0.astype(np.float64) - want0) <= bound).all()


@pytest.mark.parametrize("lh,lp", [(31, 31), (3, 31), (17, 5)], ids=lambda v: str(v))
def test_frame_f_is_frame_0_of_the_shifted_clip_on_both_sides_of_a_tile_edge(lh, lp):
    f = 70
    s = _spectrogram(2048, f, lh)
    for mode in (0, 3):
        whole = _emul_run(s, f, lh, lp, 2.0, (2.0, 3.5), mode)
        assert np.abs(whole.astype(np.float64)).sum() > 0
        for at in (1, 62, 63, 64, 65, 69):
            one = _emul_run(np.ascontiguousarray(s[:, :, at:at + lh]), 1, lh, lp, 2.0, (2.0, 3.5), mode)
            assert np.array_equal(_bits(one[..., 0]), _bits(whole[..., at])), (mode, at)


def test_the_emulator_refuses_parameters_that_are_not_the_plans():
    lib = _emul()
    d = MelDesc()
    assert lib.emul_clip_hpss(C.byref(d), 1, C.byref(_params(2048, 0, 31, 31, 2.0, (1.0, 1.0), 0, 1))) == 0
    for bad in (dict(pitch=93), dict(pitch=95), dict(lds_bytes=35340), dict(lds_bytes=35348), dict(tile_bins=32), dict(tile_frames=32),
                dict(kernel_harm=33), dict(kernel_perc=4), dict(n_stage=29), dict(out_mode=4), dict(power=3), dict(bins=1024)):
        assert lib.emul_clip_hpss(C.byref(d), 1, C.byref(_params(2048, 0, 31, 31, 2.0, (1.0, 1.0), 0, 1, bad))) == -1, bad


def test_the_sanitizer_program_of_the_planning_calls(tmp_path):
    """tools/sanitize/hpss_plan.c: pdmp3_amd/host/clip_hpss.c's check and plan over the refusals, the windows' ends and every
    pair of kernel sizes under AddressSanitizer and UBSan, a stand-alone program on the CPU"""
    run_sanitizer_program(tmp_path, "hpss_plan", ("clip_hpss.c", "clip_stft_long.c"))
