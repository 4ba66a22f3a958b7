"""Spectral descriptors of clips at n_fft 2048 and 4096, the part that needs no GPU: the check and the plan
of pdmp3_amd/host/clip_spectral.c against the restatement (tests/clip_spectral_ref.py), their refusals, and k_clip_spectral's own
index maps, LDS layouts and lane arithmetic (pdmp3_amd/csrc/spectral_core.h, compiled here with g++ into
tests/host_emul/spectral_emul.cpp's loops) on random float32 rows against the definition in binary64, within the derived bounds
-- no value left out; the roll-off by the undecided rule, its share printed and held to the cap."""
import ctypes as C
import functools

import numpy as np
import pytest

import clip_spectral_ref as spref
import clip_stft_ref as sref
from clip_host import MelDesc, build_emul, run_sanitizer_program

U = spref.U
GUARD_VALUE = np.float32(-3e9)


class SpectralParams(C.Structure):                 # include/pdmp3_hip.h pdmp3_spectral_params
    _fields_ = [("n_in", C.c_int64), ("n_fft", C.c_int32), ("n2", C.c_int32), ("hop", C.c_int32), ("n_frames", C.c_int32),
                ("tile", C.c_int32), ("channels", C.c_int32), ("bin_hz", C.c_double), ("roll_percent", C.c_double), ("amin", C.c_float),
                ("zcr_threshold", C.c_float), ("span_floats", C.c_uint32), ("lds_bytes", C.c_uint32)]


def _emul():
    lib = build_emul("spectral")
    lib.emul_clip_spectral.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.emul_spectral_lds_floats.restype = C.c_uint
    lib.emul_spectral_col.restype = C.c_uint
    assert lib.emul_spectral_desc_bytes() == C.sizeof(MelDesc) and lib.emul_spectral_params_bytes() == C.sizeof(SpectralParams)
    return lib


def _window(nw, seed):
    return (np.random.default_rng(seed).random(nw, dtype=np.float32) * np.float32(1.5) - np.float32(0.25)).astype(np.float32)


def coloured(rng, channels, t):
    """random float32 rows with the falling spectrum of music: a few random low partials under noise whose level falls with
    frequency (a random walk's), so that the magnitudes around the roll-off stand clear of the transform's error bound"""
    n = np.arange(t, dtype=np.float64)
    rows = np.zeros((channels, t))
    for ch in range(channels):
        for _ in range(6):
            rows[ch] += rng.uniform(0.02, 0.12) * np.sin(2.0 * np.pi * rng.uniform(0.002, 0.06) * n + rng.uniform(0.0, 6.28))
        walk = np.cumsum(rng.standard_normal(t))
        walk -= np.linspace(walk[0], walk[-1], t)
        rows[ch] += 0.15 * walk / max(np.abs(walk).max(), 1e-9) + 0.002 * rng.standard_normal(t)
    return rows.astype(np.float32)


def tonal(rng, channels, t, n_fft):
    """random float32 rows whose roll-off at 0.85 the binary64 definition can decide within the derived bound: five partials at
    random bin centres and phases under weak noise, the highest one 40 % of the amplitudes -- through a Hann window its centre
    bin alone carries the cumulative sum from 70 % to 90 % of the total, far more than the threshold's interval is wide"""
    n = np.arange(t, dtype=np.float64)
    rows = np.zeros((channels, t))
    for ch in range(channels):
        ks = np.sort(rng.choice(np.arange(8, n_fft // 2 - 8, 16), size=5, replace=False) + rng.integers(0, 8, size=5))
        for k, a in zip(ks, (0.06, 0.06, 0.06, 0.06, 0.16)):
            rows[ch] += a * np.sin(2.0 * np.pi * k * n / n_fft + rng.uniform(0.0, 6.28))
        rows[ch] += 1e-5 * rng.standard_normal(t)
    return rows.astype(np.float32)


def _emul_run(n_fft, hop, nw, win, channels, F, rows_in, T, Ts, lead, sr, roll=0.85, amin=1e-10, zt=1e-10):
    from pdmp3_amd import api
    lib = _emul()
    n2 = n_fft // 64
    tab = np.concatenate([t.ravel() for t in api.stft_long_tables(n_fft, nw, win, False)])
    tile, _, lds_bytes = api.spectral_plan(n_fft, hop)
    per = 6 * F
    out = np.full((channels, per + 8), GUARD_VALUE, dtype=np.float32)
    d = MelDesc(src=rows_in.ctypes.data, dst=out.ctypes.data, src_chan_stride=Ts, dst_chan_stride=per + 8, lead=lead)
    span = ((tile - 1) * hop + n_fft + 3) // 4 * 4
    P = SpectralParams(n_in=T, n_fft=n_fft, n2=n2, hop=hop, n_frames=F, tile=tile, channels=channels, bin_hz=sr / n_fft, roll_percent=roll,
                       amin=amin, zcr_threshold=zt, span_floats=span, lds_bytes=lds_bytes)
    assert lib.emul_clip_spectral(C.byref(d), 1, tab.ctypes.data, C.byref(P)) == 0
    assert (out[:, per:] == GUARD_VALUE).all() and (out[:, :per] != GUARD_VALUE).all()
    return out[:, :per].reshape(channels, 6, F), tile


def test_refusals_write_nothing_and_the_older_checks_refuse_what_they_refused():
    from pdmp3_amd import api
    lib = api.load_library()
    assert api.SPECTRAL_ROWS == spref.ROWS and len(api.SPECTRAL_ROWS) == 6
    assert api.spectral_check(22050) and api.spectral_check(48000, n_fft=4096, hop=1024) and api.spectral_check(44100, hop=1)
    assert api.spectral_check(44100, hop=2048, roll_percent=0.01, amin=1e-30, zcr_threshold=0.0)
    assert api.spectral_check(22050, win_length=1764, window=_window(1764, 1)) and api.spectral_check(48000, win_length=1920, roll_percent=0.999)
    assert api.spectral_check(22050, n_fft=4096, hop=4096, zcr_threshold=0.25, n_frames=0)
    bad_window = _window(2048, 2)
    bad_window[77] = np.nan
    inf, nan = float("inf"), float("nan")
    refused = [dict(n_fft=1024), dict(n_fft=8192), dict(n_fft=2047), dict(n_fft=2049), dict(n_fft=4095), dict(n_fft=400), dict(n_fft=0),
               dict(hop=0), dict(hop=2049), dict(n_fft=4096, hop=4097), dict(hop=-1), dict(win_length=2049), dict(win_length=-1),
               dict(window=bad_window), dict(window=np.array([1.0, np.inf], dtype=np.float32)), dict(n_frames=-1),
               dict(roll_percent=0.0), dict(roll_percent=1.0), dict(roll_percent=-0.5), dict(roll_percent=1.5), dict(roll_percent=nan),
               dict(roll_percent=inf), dict(amin=0.0), dict(amin=-1e-10), dict(amin=nan), dict(amin=inf), dict(amin=1e-46), dict(amin=1e39),
               dict(zcr_threshold=-1e-10), dict(zcr_threshold=nan), dict(zcr_threshold=inf), dict(zcr_threshold=-inf)]
    for bad in refused:
        assert not api.spectral_check(22050, **bad), bad
    assert not api.spectral_check(0) and not api.spectral_check(-1)
    assert lib.pdmp3_amd_spectral_check(None, 22050) == -1
    for n_fft, hop in ((1024, 256), (8192, 512), (2048, 0), (2048, 2049), (4096, 4097), (2047, 512), (2048, -1), (0, 1)):
        with pytest.raises(ValueError):
            api.spectral_plan(n_fft, hop)
        t, p, b = C.c_int(-5), C.c_int(-6), C.c_uint(77)
        assert lib.pdmp3_amd_spectral_plan(n_fft, hop, C.byref(t), C.byref(p), C.byref(b)) == -1 and (t.value, p.value, b.value) == (-5, -6, 77)
    assert lib.pdmp3_amd_spectral_plan(2048, 512, None, None, None) == 0
    spec, keep = api._spectral_spec()
    assert lib.pdmp3_amd_bulk_decode_clips_spectral(None, None, 0, C.byref(spec), None) == -1
    # sections 13's, 14's and 15's checks: what they accepted and refused before
    assert api.stft_long_check(44100) and api.stft_long_check(48000, n_fft=4096, hop=4096, mode="log10")
    assert api.mel_long_check(22050) and api.mel_long_check(48000, n_fft=4096, hop=1024)
    for bad in (dict(n_fft=1024), dict(n_fft=8192), dict(hop=0), dict(hop=2049), dict(win_length=2049), dict(window=bad_window), dict(mode=5),
                dict(mode="log", floor=0.0), dict(n_frames=-1)):
        assert not api.stft_long_check(44100, **bad), bad
    for bad in (dict(n_fft=1024), dict(n_fft=8192), dict(hop=0), dict(hop=2049), dict(n_mels=0), dict(n_mels=257), dict(mode="whisper"),
                dict(floor=0.0), dict(win_length=2049), dict(window=bad_window), dict(f_max=22050 / 2 + 1.0)):
        assert not api.mel_long_check(22050, **bad), bad
    assert not api.stft_check(22050, n_fft=2048, hop=512) and not api.mel_check(22050, n_fft=2048, hop=512)
    assert api.stft_long_plan(2048, 512)[0] == 16 and api.mel_long_plan(4096, 4096, 128)[0] == 4


def test_the_plan_is_the_restated_one_over_all_hops_and_the_columns_are_a_bijection():
    from pdmp3_amd import api
    lib = _emul()
    for n_fft in spref.SIZES:
        n2, tile = n_fft // 64, 8 if n_fft == 2048 else 4
        worst = 0
        for hop in range(1, n_fft + 1):
            got = api.spectral_plan(n_fft, hop)
            want = spref.plan(n_fft, hop)
            assert got == want[:3] and want[3] in spref.PATHS, (n_fft, hop)
            assert got[0] == tile and got[1] == 0 and 64 * 1024 < got[2] <= spref.LDS_MAX and got[2] % 16 == 0
            assert got[2] == 4 * lib.emul_spectral_lds_floats(tile, hop, n_fft)
            first = ((tile - 1) * hop + n_fft + 3) // 4 * 4
            assert got[2] >= 4 * (first + tile * n2 * 32 + tile * (n_fft // 2 + 1) + 8 * tile)
            worst = max(worst, got[2])
        print("N %d: %d frames at every hop, %d B at hop 512, %d B at the most (hop %d)" % (n_fft, tile, api.spectral_plan(n_fft, 512)[2], worst, n_fft))
        assert worst == api.spectral_plan(n_fft, n_fft)[2]
        cols = [lib.emul_spectral_col(k) for k in range(n_fft // 2 + 1)]
        assert cols == [spref.col(k) for k in range(n_fft // 2 + 1)] and sorted(cols) == list(range(n_fft // 2 + 1)) and cols[-1] == n_fft // 2
        assert all(c >> 5 == k >> 5 for k, c in enumerate(cols))                # a block of 32 bins stays its block of 32 floats
        # the banks: a group of 32 lanes of stage 2's writes, and of the reduction's reads at every step, covers the 32 banks once
        for kt in range(4):
            for ct in range(n2 // 32):
                for r in range(4):
                    for half in range(2):
                        banks = {cols[16 * kt + 4 * kq + r + 64 * (16 * ct + j)] % 32 for j in range(16) for kq in (2 * half, 2 * half + 1)}
                        assert len(banks) == 32
        run = n_fft // 128
        for i in range(run):
            for half in range(2):
                assert len({cols[run * lane + i] % 32 for lane in range(32 * half, 32 * half + 32)}) == 32
    assert api.spectral_plan(2048, 512)[2] == 88352


EMUL_CASES = [
    # n_fft, hop, win_length, own window, channels, start, n_frames, J - start (None: all signal), sr, roll_percent
    # roll_percent 0.85 on tonal rows, 0.01 / 0.005 on noise-like ones and under a caller's random window, whose leakage makes
    # every frame noise-like: where the definition itself can decide the roll-off within the bound (clip_spectral_ref.py)
    (2048, 512, 2048, False, 2, 0, 11, None, 48000, 0.85),         # one full tile and a partial one; stereo
    (2048, 441, 1764, True, 1, 57, 11, 3000, 22050, 0.01),         # a caller's window of 1764; valid = 7 ends inside a tile
    (2048, 2048, 2048, False, 1, 5000, 11, 9000, 44100, 0.85),     # H = N; valid = 5
    (4096, 1024, 4096, False, 1, 300, 6, 2500, 48000, 0.005),      # N2 = 64, tile 4; valid = 3 ends inside a tile
    (4096, 2048, 4096, False, 1, 5000, 5, None, 44100, 0.85),      # N2 = 64 on tonal rows
    (4096, 4096, 1920, True, 2, 100, 5, None, 48000, 0.005),       # H = N, stereo, a caller's window of 1920
    (2048, 1, 2048, False, 1, 3, 11, None, 32000, 0.01),           # H = 1
    (4096, 3000, 4096, False, 1, 100000, 6, -7, 44100, 0.85),      # wholly behind J: silent frames only
]
@functools.lru_cache(maxsize=None)
def _case(case):
    """one case through the reference and the emulator, once: (got [C, 6, F], tile, spref.spectral's result)"""
    n_fft, hop, nw, own, channels, start, F, left, sr, roll = case
    rng = np.random.default_rng((n_fft * 131 + hop * 17 + start) & 0xffffffff)
    win = _window(nw, 3000 + nw) if own else None
    s0 = max(0, start - n_fft // 2)
    lead = s0 - (start - n_fft // 2)
    T = (F - 1) * hop + n_fft
    Ts = (T + 3) // 4 * 4
    stage = np.full(channels * Ts + 16, np.float32(7e8), dtype=np.float32)        # (guards: nothing outside [0, T) may be read)
    rows = stage[8:8 + channels * Ts].reshape(channels, Ts)
    rows[:, :T] = tonal(rng, channels, T, n_fft) if roll == 0.85 else coloured(rng, channels, T)
    if left is not None:
        rows[:, max(0, start + left - s0):T] = 0.0
    y = rows[:, :T].copy()
    res = spref.spectral(y, s0, start, F, n_fft, hop, sr, roll_percent=roll, win_length=nw, window=win)
    got, tile = _emul_run(n_fft, hop, nw, win, channels, F, rows, T, Ts, lead, sr, roll=roll)
    return got, tile, res


@pytest.mark.parametrize("case", EMUL_CASES, ids=lambda c: "N%d-H%d-Nw%d-C%d-s%d" % (c[0], c[1], c[2], c[4], c[5]))
def test_kernel_arithmetic_on_the_host_against_binary64(case):
    n_fft, hop, nw, own, channels, start, F, left, sr, roll = case
    got, tile, res = _case(case)
    assert tile < F < 2 * tile
    want, bound, signal = res["want"], res["bound"], res["signal"]
    err = np.abs(got.astype(np.float64) - want)
    for r, name in enumerate(spref.ROWS):
        if r == 4:
            continue
        assert (err[:, r] <= bound[:, r]).all(), (name, float((err[:, r] - bound[:, r]).max()))
        nz = bound[:, r] > 0
        ratio = float((err[:, r][nz] / bound[:, r][nz]).max()) if nz.any() else 0.0
        print("N %d H %d Nw %d C %d start %d tile %d, %s: worst error / bound %.4f" % (n_fft, hop, nw, channels, start, tile, name, ratio))
    assert np.array_equal(got[:, 1], want[:, 1].astype(np.float32))               # zcr: exact
    und, frames = spref.check_rolloff(got[:, 4], res, sr, n_fft)
    print("N %d H %d start %d: roll-off undecided in %d of %d frames" % (n_fft, hop, start, und, frames))
    assert und <= spref.UNDECIDED_CAP * frames
    # silent frames: rows 0 .. 4 exactly +0, row 5 within its bound of 1
    assert (got[:, :5].transpose(0, 2, 1)[~signal].view(np.uint32) == 0).all()
    assert (got[:, 5] > 0).all() and (got[:, 5] <= 1.0 + 1e-5).all()
    if left is not None:
        nv = sref.valid(start + left, start, hop, F)
        assert nv < F and not signal[:, nv + (n_fft // 2 + hop - 1) // hop:].any()


def test_the_cases_cover_both_launch_paths_and_the_edges():
    paths, stereo, own1764, hop1, hopn, inside, silent = set(), 0, 0, 0, 0, 0, 0
    for n_fft, hop, nw, own, channels, start, F, left, sr, roll in EMUL_CASES:
        paths.add(spref.plan(n_fft, hop)[3])
        stereo += channels == 2
        own1764 += own and nw == 1764
        hop1 += hop == 1
        hopn += hop == n_fft
        if left is not None:
            nv = sref.valid(start + left, start, hop, F)
            inside += 0 < nv < F and nv % spref.plan(n_fft, hop)[0] != 0
            silent += nv + (n_fft // 2 + hop - 1) // hop < F
    assert paths == set(spref.PATHS) and stereo and own1764 and hop1 and hopn >= 2 and inside >= 2 and silent >= 2


def test_zero_crossings_are_counted_exactly_with_a_dead_band():
    n_fft, hop, F, sr = 2048, 300, 9, 22050
    T = (F - 1) * hop + n_fft
    rng = np.random.default_rng(5)
    rows = np.zeros((1, T + 4), dtype=np.float32)
    rows[0, :T] = (rng.random(T, dtype=np.float32) * 2 - 1) * np.float32(0.01)
    rows[0, ::7] = 0.0
    rows[0, 3::11] = np.float32(-0.004)                                          # exactly on the threshold: not negative
    for zt in (0.0, 1e-10, 0.004, 0.005):
        got, _ = _emul_run(n_fft, hop, n_fft, None, 1, F, rows, T, T + 4, 0, sr, zt=zt)
        frames = np.stack([rows[0, f * hop:f * hop + n_fft] for f in range(F)])
        count = spref.zcr_count(frames, zt)
        assert np.array_equal(got[0, 1], (count / n_fft).astype(np.float32)) and count.min() > 0, zt
    assert np.float32(0.004) == -rows[0, 3]


def test_a_sine_at_a_bin_centre_and_white_noise():
    sr = 22050
    ones = {n: np.ones(n, dtype=np.float32) for n in spref.SIZES}
    rng = np.random.default_rng(11)
    for n_fft, hop, k0 in ((2048, 512, 200), (4096, 1024, 777)):
        F = 3
        T = (F - 1) * hop + n_fft
        rows = np.zeros((1, T + 4), dtype=np.float32)
        rows[0, :T] = (0.5 * np.sin(2.0 * np.pi * k0 * np.arange(T) / n_fft + 0.3)).astype(np.float32)
        sine, _ = _emul_run(n_fft, hop, n_fft, ones[n_fft], 1, F, rows, T, T + 4, 0, sr)      # (a window of ones: one bin holds the sine)
        f0 = k0 * sr / n_fft
        assert (np.abs(sine[0, 2] - f0) < 1.0).all() and (sine[0, 4] == np.float32(f0)).all()
        assert (sine[0, 3] < 0.01 * sr / 2).all() and (sine[0, 5] < 1e-6).all()
        assert (np.abs(sine[0, 0] - 0.5 / np.sqrt(2.0)) < 1e-3).all()
        rows[0, :T] = (rng.standard_normal(T) * 0.1).astype(np.float32)
        noise, _ = _emul_run(n_fft, hop, n_fft, None, 1, F, rows, T, T + 4, 0, sr)
        print("N %d: flatness of the sine %.3g, of white noise %.3f" % (n_fft, float(sine[0, 5].max()), float(noise[0, 5].min())))
        assert (noise[0, 5] > 0.3).all() and (noise[0, 5] > 1e5 * sine[0, 5]).all()
        assert (np.abs(noise[0, 2] - sr / 4) < 0.1 * sr).all()


@pytest.mark.parametrize("n_fft,hop", [(2048, 512), (2048, 2048), (4096, 1024), (4096, 4096)])
def test_a_frame_is_the_same_chains_wherever_it_lies_in_a_tile(n_fft, hop):
    """frame f of a row is bit-equal to frame 0 of the row shifted by f H: both sides of the tile's edge, on both paths"""
    tile = spref.plan(n_fft, hop)[0]
    F = tile + 2
    T = (F - 1) * hop + n_fft
    Ts = (T + 3) // 4 * 4
    rng = np.random.default_rng(n_fft + hop)
    rows = np.zeros((1, Ts + 4), dtype=np.float32)
    rows[0, :T] = coloured(rng, 1, T)[0]
    whole, _ = _emul_run(n_fft, hop, n_fft, None, 1, F, rows, T, Ts, 0, 44100)
    assert np.abs(whole).sum() > 0
    for f in (1, tile - 1, tile, tile + 1):
        sh = np.zeros((1, n_fft + 4), dtype=np.float32)
        sh[0, :n_fft] = rows[0, f * hop:f * hop + n_fft]
        one, _ = _emul_run(n_fft, hop, n_fft, None, 1, 1, sh, n_fft, n_fft, 0, 44100)
        assert np.array_equal(one[0, :, 0].view(np.uint32), whole[0, :, f].view(np.uint32)), f


def test_the_rolloff_follows_the_stated_order_on_the_spectrum_the_plane_holds():
    """the restated order (clip_spectral_ref.rolloff_stated) on the definition's magnitudes rounded to binary32 gives the
    emulator's bin wherever the frame is decided: the restatement and the kernel's lanes, scan and search agree"""
    n_fft, hop, F, sr = 2048, 512, 9, 22050
    T = (F - 1) * hop + n_fft
    rng = np.random.default_rng(77)
    rows = np.zeros((1, T + 4), dtype=np.float32)
    rows[0, :T] = tonal(rng, 1, T, n_fft)[0]
    for roll in (0.85, 0.5, 0.99):
        got, _ = _emul_run(n_fft, hop, n_fft, None, 1, F, rows, T, T + 4, 0, sr, roll=roll)
        res = spref.spectral(rows[:, :T], 0, n_fft // 2, F, n_fft, hop, sr, roll_percent=roll)
        spref.check_rolloff(got[:, 4], res, sr, n_fft)
        x, _ = sref.stft(rows[:, :T], 0, n_fft // 2, F, n_fft, hop, 1)
        stated = spref.rolloff_stated(np.moveaxis(x, 1, 2).astype(np.float32), roll, n_fft)
        decided = ~res["undecided"]
        assert np.array_equal(stated[decided], res["roll"][decided]) and decided.any(), roll


def test_the_undecided_share_of_the_rolloff_stays_within_the_cap():
    und = frames = 0
    for case in EMUL_CASES:
        got, tile, res = _case(case)
        u, f = spref.check_rolloff(got[:, 4], res, case[8], case[0])
        und, frames = und + u, frames + f
    print("roll-off: undecided in %d of %d frames of the host cases (%.1f %%; the cap is %.0f %%)" % (und, frames, 100.0 * und / frames, 100 * spref.UNDECIDED_CAP))
    assert und <= spref.UNDECIDED_CAP * frames


def test_the_emulator_refuses_parameters_that_leave_the_lds():
    lib = _emul()
    d = MelDesc()
    z = np.zeros(1, dtype=np.float32)
    span = 7 * 512 + 2048
    ok = dict(n_in=0, n_fft=2048, n2=32, hop=512, n_frames=0, tile=8, channels=1, bin_hz=10.0, roll_percent=0.85, amin=1e-10, zcr_threshold=1e-10,
              span_floats=span, lds_bytes=(span + 8 * 32 * 32 + 8 * 1025 + 64) * 4)
    assert lib.emul_clip_spectral(C.byref(d), 1, z.ctypes.data, C.byref(SpectralParams(**ok))) == 0
    for bad in (dict(span_floats=span - 4), dict(lds_bytes=ok["lds_bytes"] - 4), dict(tile=4), dict(tile=16), dict(n2=64), dict(hop=513),
                dict(roll_percent=1.0), dict(amin=0.0), dict(zcr_threshold=-1.0), dict(lds_bytes=160 * 1024)):
        assert lib.emul_clip_spectral(C.byref(d), 1, z.ctypes.data, C.byref(SpectralParams(**dict(ok, **bad)))) == -1, bad


def test_the_sanitizer_program_of_the_planning_calls(tmp_path):
    """tools/sanitize/spectral_plan.c: pdmp3_amd/host/clip_spectral.c's check and plan over the refusals, the windows' ends and
    every hop under AddressSanitizer and UBSan, a stand-alone program on the CPU"""
    run_sanitizer_program(tmp_path, "spectral_plan", ("clip_spectral.c", "clip_stft_long.c"))
