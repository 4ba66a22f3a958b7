"""MFCC, deltas and dB mel of clips at n_fft 2048 / 4096 without a GPU: the planning calls of
pdmp3_amd/host/clip_mfcc_long.c (check, DCT table, delta taps, plan) against the definition and against scipy, and the kernels'
own values, LDS planes and stencil (pdmp3_amd/csrc/mfcc_long_core.h, compiled here with g++ into
tests/host_emul/mfcc_long_emul.cpp's loops) on random log-mel input: the dB values bit for bit, the cepstra and the deltas within
the derived bounds of tests/clip_mfcc_long_ref.py."""
import ctypes as C

import numpy as np
import pytest

import clip_mfcc_long_ref as ref
from clip_host import MelDesc, build_emul, run_sanitizer_program

GUARD_VALUE = np.float32(-3e9)
LDS_MAX = 160 * 1024 - 64              # include/pdmp3_hip.h PDMP3_MEL_LDS_MAX


class MfccLongParams(C.Structure):     # include/pdmp3_hip.h pdmp3_mfcc_long_params
    _fields_ = [(n, C.c_int32) for n in ("n_mels", "mels16", "n_mfcc", "ceps16", "n_frames", "n_stage", "halo", "deltas", "tile", "channels",
                                         "d_pitch", "c_pitch", "out_mode", "use_top")] + \
               [("top_db", C.c_float), ("lds_bytes", C.c_uint32), ("taps", (C.c_double * 17) * 2)]


def _emul():
    lib = build_emul("mfcc_long")
    lib.emul_clip_mfcc_long.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    for name in ("lds_floats", "d_at", "c_at", "b_at", "result_at"):
        getattr(lib, "emul_mfcc_long_" + name).restype = C.c_uint
    assert lib.emul_mfcc_long_desc_bytes() == C.sizeof(MelDesc) and lib.emul_mfcc_long_params_bytes() == C.sizeof(MfccLongParams)
    return lib


def _emul_run(stage, f, n_mfcc=20, lifter=0.0, top_db=80.0, deltas=0, w=9, mode="mfcc"):
    """stage: float32 [C, n_mels, F + 2 h] log10 mel -> the emulator's [C, rows, F]"""
    from pdmp3_amd import api
    lib = _emul()
    channels, nm = stage.shape[0], stage.shape[1]
    front, back, tile, dp, cp, lds = api.mfcc_long_plan(nm, n_mfcc, deltas, w, mode)
    assert stage.shape[2] == f + 2 * front and stage.dtype == np.float32 and front == back
    rows = nm if mode == "db" else (1 + deltas) * n_mfcc
    p = MfccLongParams(n_mels=nm, mels16=(nm + 15) & ~15, n_frames=f, n_stage=f + 2 * front, halo=front, tile=tile, channels=channels, d_pitch=dp,
                       c_pitch=cp, out_mode=ref.MODES.index(mode), use_top=top_db is not None, top_db=0.0 if top_db is None else top_db, lds_bytes=lds)
    table = None
    if mode == "mfcc":
        p.n_mfcc, p.ceps16, p.deltas = n_mfcc, (n_mfcc + 15) & ~15, deltas
        table = np.ascontiguousarray(api.mfcc_long_dct_table(nm, n_mfcc, lifter))
        if deltas:
            t = api.mfcc_long_delta_taps(w)
            for o in range(2):
                for j in range(w):
                    p.taps[o][j] = t[o, j]
    mel_floats = nm * (f + 2 * front)
    buf = np.full(channels * mel_floats + channels, np.nan, dtype=np.float32)         # (the log-mel, then the planes' thresholds)
    buf[:channels * mel_floats] = stage.reshape(-1)
    per = rows * f
    out = np.full((channels, per + 8), GUARD_VALUE, dtype=np.float32)
    d = MelDesc(buf.ctypes.data, out.ctypes.data, mel_floats, per + 8, 0, 0)
    assert lib.emul_clip_mfcc_long(C.byref(d), 1, table.ctypes.data if table is not None else None, C.byref(p)) == 0
    assert (out[:, per:] == GUARD_VALUE).all()
    return out[:, :per].reshape(channels, rows, f).copy()


def _log_mel(channels, nm, cols, seed):
    """random log10 mel values between the floor (-10) and +3, with runs at the floor, a loud column and equal maxima"""
    rng = np.random.default_rng(seed)
    l = (rng.random((channels, nm, cols), dtype=np.float32) * np.float32(8.0) - np.float32(6.0)).astype(np.float32)
    l[:, :, cols // 3] = np.float32(-10.0)
    l[:, nm // 2, :] = np.float32(-10.0)
    l[:, :, 0] += np.float32(3.0)                          # (the loudest column is the first: a halo column where there is a halo)
    l[:, 3, cols // 2] = l[:, 5, cols // 2 + 1] = np.float32(2.5)
    return l


def test_check_refusals_one_by_one():
    from pdmp3_amd import api
    assert api.MFCC_LONG_MODES == {m: i for i, m in enumerate(ref.MODES)}
    ok = api.mfcc_long_check
    assert ok(22050) and ok(44100, n_fft=4096, hop=1024, n_mels=256, n_mfcc=128, deltas=2, delta_width=17, lifter=22.0, top_db=None)
    assert ok(22050, out_mode="db", n_mfcc=0, deltas=7, delta_width=4, lifter=-1.0) and ok(22050, out_mode="db", n_mfcc=2.5, deltas=0.5) and ok(22050, top_db=0.0) and ok(22050, deltas=0, delta_width=4)
    assert ok(22050, n_mels=20, n_mfcc=20) and ok(22050, deltas=1, delta_width=3) and ok(16000, win_length=400, window=np.ones(400, dtype=np.float32))
    for bad in (dict(n_fft=1024), dict(n_fft=8192), dict(hop=0), dict(hop=2049), dict(n_mels=0), dict(n_mels=257), dict(amin=0.0), dict(amin=float("nan")),
                dict(f_max=12000.0), dict(n_frames=-1), dict(win_length=2049), dict(top_db=float("nan")), dict(top_db=float("inf")), dict(top_db=-1.0),
                dict(n_mfcc=0), dict(n_mfcc=129, n_mels=256), dict(n_mfcc=21, n_mels=20), dict(lifter=-1.0), dict(lifter=float("nan")),
                dict(lifter=float("inf")), dict(deltas=-1), dict(deltas=3), dict(deltas=1, delta_width=2), dict(deltas=2, delta_width=19),
                dict(deltas=1, delta_width=1), dict(out_mode="ceps"), dict(out_mode=2), dict(n_mfcc=1, n_frames=(2 ** 31 - 1) // 128 + 1),
                dict(n_mfcc=1, deltas=2, n_frames=(2 ** 31 - 1) // 128 - 7), dict(out_mode="db", n_frames=(2 ** 31 - 1) // 128 + 1)):
        assert not ok(22050, **bad), bad
    assert ok(22050, n_mfcc=1, n_frames=(2 ** 31 - 1) // 128) and ok(22050, n_mfcc=1, deltas=2, n_frames=(2 ** 31 - 1) // 128 - 8)
    assert not ok(0) and not ok(-1)


@pytest.mark.parametrize("n_mels", [20, 40, 128, 256])
def test_dct_table_against_the_definition_and_scipy(n_mels):
    import scipy.fft
    from pdmp3_amd import api
    full = scipy.fft.dct(np.eye(n_mels), type=2, norm="ortho", axis=0)
    for n_mfcc in sorted({1, 13, 20, min(n_mels, 128)}):
        for lifter in (0.0, 22.0):
            want = ref.dct(n_mels, n_mfcc, lifter)
            lift = 1.0 + (lifter / 2.0) * np.sin(np.pi * np.arange(1, n_mfcc + 1) / lifter) if lifter else np.ones(n_mfcc)
            assert np.abs(want - full[:n_mfcc] * lift[:, None]).max() <= 1e-12
            t = api.mfcc_long_dct_table(n_mels, n_mfcc, lifter)
            assert t.shape == ((n_mfcc + 15) // 16 * 16, (n_mels + 15) // 16 * 16) and t.dtype == np.float32
            assert (np.abs(t[:n_mfcc, :n_mels].astype(np.float64) - want) <= ref.U * np.abs(want)).all()
            assert (t[n_mfcc:] == 0).all() and (t[:, n_mels:] == 0).all()
    for bad in ((0, 1, 0.0), (257, 1, 0.0), (20, 21, 0.0), (256, 129, 0.0), (128, 20, -1.0), (128, 20, float("nan"))):
        with pytest.raises(ValueError):
            api.mfcc_long_dct_table(*bad)


def test_delta_taps_against_savgol_and_the_literal_rows():
    import scipy.signal
    from pdmp3_amd import api
    for w in range(3, 18, 2):
        t = api.mfcc_long_delta_taps(w)
        assert t.shape == (2, w) and t.dtype == np.float64
        for order in (1, 2):
            sg = scipy.signal.savgol_coeffs(w, order, deriv=order, use="dot")
            assert np.abs(t[order - 1] - sg).max() <= 1e-14, (w, order)
        assert np.array_equal(t, ref.taps(w))
    j = np.arange(-4, 5, dtype=np.float64)
    t = api.mfcc_long_delta_taps(9)
    assert np.abs(t[0] - j / 60.0).max() <= 1e-16 and np.abs(t[1] - (3.0 * j * j - 20.0) / 462.0).max() <= 1e-16
    for w in (0, 1, 2, 4, 16, 18, 19, -3):
        with pytest.raises(ValueError):
            api.mfcc_long_delta_taps(w)


def test_the_references_delta_is_the_interior_of_savgol_filter():
    """validates the reference (tests/clip_mfcc_long_ref.py delta) that the other tests hold the library against, not the
    library itself: it passes without the feature"""
    import scipy.signal
    rng = np.random.default_rng(3)
    c = rng.standard_normal((7, 60))
    for w in (3, 9, 17):
        h = w // 2
        for order in (1, 2):
            sg = scipy.signal.savgol_filter(c, w, polyorder=order, deriv=order, axis=-1, mode="interp")
            assert np.abs(ref.delta(c, w, order)[0] - sg[:, h:60 - h]).max() <= 1e-12, (w, order)


def test_plan_fits_the_lds_at_every_shape():
    from pdmp3_amd import api
    lib = _emul()
    assert lib.emul_mfcc_long_d_pitch() == 80 and lib.emul_mfcc_long_c_pitch() == 84
    for nm in (1, 16, 17, 20, 40, 128, 255, 256):
        for nc in sorted({1, min(nm, 13), min(nm, 16), min(nm, 17), min(nm, 128)}):
            for deltas in (0, 1, 2):
                for w in (3, 9, 17):
                    got = api.mfcc_long_plan(nm, nc, deltas, w)
                    assert got == ref.plan(nm, nc, deltas, w), (nm, nc, deltas, w)
                    # the arithmetic, restated: a plane [mels16][64 + 16] and a plane [ceps16][64 + 16 + 4] of floats
                    m16, c16 = (nm + 15) // 16 * 16, (nc + 15) // 16 * 16
                    assert got[5] == 4 * (m16 * (64 + 16) + c16 * (64 + 16 + 4)) == 4 * lib.emul_mfcc_long_lds_floats(m16, c16) <= LDS_MAX
                    assert lib.emul_mfcc_long_cols16(got[0]) == (64 if not got[0] else 80) >= 64 + 2 * got[0]
    assert api.mfcc_long_plan(256, 128, 2, 17)[5] == 124928 and api.mfcc_long_plan(128, 20, 2, 9)[5] == 51712 <= 64 * 1024
    assert api.mfcc_long_plan(128, 0, 5, 4, "db") == ref.plan(128, 0, 5, 4, "db")
    for bad in ((0, 1, 0, 9), (257, 1, 0, 9), (128, 129, 0, 9), (20, 21, 0, 9), (128, 20, 3, 9), (128, 20, 1, 8), (128, 20, 1, 19)):
        with pytest.raises(ValueError):
            api.mfcc_long_plan(*bad)


def test_the_planes_addresses_are_a_bijection_and_every_access_meets_32_banks_once():
    lib = _emul()
    for m16, c16 in ((16, 16), (48, 16), (128, 32), (256, 128)):
        total = lib.emul_mfcc_long_lds_floats(m16, c16)
        seen = np.zeros(total, dtype=np.int32)
        for m in range(m16):
            for c in range(80):
                seen[lib.emul_mfcc_long_d_at(m, c)] += 1
        for q in range(c16):
            for c in range(84):
                seen[lib.emul_mfcc_long_c_at(m16, q, c)] += 1
        assert (seen == 1).all()
        # a 4-byte access is served 32 lanes at a time (lanes 0 .. 31, then 32 .. 63) over 32 banks
        def once(addr):
            a = np.array(addr, dtype=np.int64)
            assert a.size == 64
            for half in (a[:32], a[32:]):
                assert np.unique(half % 32).size == 32, addr
        for col0 in range(0, 80, 16):
            for k in (0, 4, m16 - 4):
                once([lib.emul_mfcc_long_b_at(k, lane >> 4, col0, lane & 15) for lane in range(64)])
            for q0 in range(0, c16, 16):
                for r in range(4):
                    once([lib.emul_mfcc_long_result_at(m16, q0, lane >> 4, r, col0, lane & 15) for lane in range(64)])
        for m in (0, m16 - 1):
            once([lib.emul_mfcc_long_d_at(m, lane) for lane in range(64)])
        for q in (0, 1, c16 - 1):
            for j in range(17):
                once([lib.emul_mfcc_long_c_at(m16, q, lane + j) for lane in range(64)])


@pytest.mark.parametrize("nm,nc,f", [(40, 13, 69), (128, 20, 133), (20, 20, 5), (256, 128, 64)])
def test_the_emulated_course_db_bit_for_bit_cepstra_and_deltas_within_the_bounds(nm, nc, f):
    worst_c, worst_d, worst_full = 0.0, 0.0, 0.0
    for top in (80.0, 6.0, None):
        l = _log_mel(2, nm, f, nm + f)
        got = _emul_run(l, f, top_db=top, mode="db")
        for ch in range(2):
            assert np.array_equal(got[ch].view(np.uint32), ref.db(l[ch], top).view(np.uint32)), (top, ch)
        if top == 6.0:
            assert (got[0] == got[0].max() - np.float32(6.0)).any() and got[0].max() != got[1].max()
        for lifter in (0.0, 22.0):
            c = _emul_run(l, f, nc, lifter, top)
            for ch in range(2):
                want, bound = ref.cepstra(ref.db(l[ch], top), nc, lifter)
                err = np.abs(c[ch].astype(np.float64) - want)
                assert (err <= bound).all(), (top, lifter, ch, float((err / bound).max()))
                worst_c = max(worst_c, float((err / bound).max()))
        for w in (3, 9, 17):
            h = w // 2
            lw = _log_mel(2, nm, f + 2 * h, nm + f + w)
            wide = _emul_run(lw, f + 2 * h, nc, 22.0, None)
            for deltas in (1, 2):
                got = _emul_run(lw, f, nc, 22.0, top, deltas, w)
                if top is None:
                    assert np.array_equal(got[:, :nc].view(np.uint32), np.ascontiguousarray(wide[:, :, h:h + f]).view(np.uint32))
                for ch in range(2):
                    full, fb = ref.mfcc(lw[ch], nc, 22.0, top, deltas, w, f)
                    err = np.abs(got[ch].astype(np.float64) - full)
                    assert (err <= fb).all(), (top, w, deltas, ch, float((err / fb).max()))
                    worst_full = max(worst_full, float((err / fb).max()))
                    if top is None:
                        for order in range(1, deltas + 1):
                            want, mass = ref.delta(wide[ch], w, order)
                            bound = ref.delta_bound(want, mass, w)
                            err = np.abs(got[ch, order * nc:(order + 1) * nc].astype(np.float64) - want)
                            assert (err <= bound).all(), (w, deltas, order, ch, float((err / bound).max()))
                            worst_d = max(worst_d, float((err / bound).max()))
                    else:
                        # the loudest column is a halo column: it does not set the threshold
                        own = (np.float32(10.0) * lw[ch][:, h:h + f]).max()
                        assert (np.float32(10.0) * lw[ch]).max() > own
    print("%d bands, %d cepstra, %d frames: worst error / bound %.4f (cepstra), %.4f (deltas on the cepstra), %.4f (the full chain)"
          % (nm, nc, f, worst_c, worst_d, worst_full))
    assert 0.0 < worst_c <= 1.0 and 0.0 < worst_d <= 1.0 and 0.0 < worst_full <= 1.0


def test_the_emulator_refuses_what_the_engine_refuses():
    lib = _emul()
    l = _log_mel(1, 40, 20, 1)
    buf = np.concatenate([l.reshape(-1), np.zeros(1, dtype=np.float32)])
    out = np.zeros(13 * 20, dtype=np.float32)
    d = MelDesc(buf.ctypes.data, out.ctypes.data, 800, 260, 0, 0)
    table = np.zeros((16, 48), dtype=np.float32)
    good = dict(n_mels=40, mels16=48, n_mfcc=13, ceps16=16, n_frames=20, n_stage=20, tile=64, channels=1, d_pitch=80, c_pitch=84, lds_bytes=4 * (48 * 80 + 16 * 84))
    assert lib.emul_clip_mfcc_long(C.byref(d), 1, table.ctypes.data, C.byref(MfccLongParams(**good))) == 0
    for bad in (dict(mels16=40), dict(ceps16=32), dict(tile=32), dict(d_pitch=64), dict(c_pitch=80), dict(lds_bytes=4 * 48 * 80), dict(n_stage=28),
                dict(halo=4), dict(halo=9, n_stage=38, deltas=1), dict(deltas=1), dict(deltas=3), dict(n_mfcc=41), dict(n_mels=257), dict(out_mode=2)):
        assert lib.emul_clip_mfcc_long(C.byref(d), 1, table.ctypes.data, C.byref(MfccLongParams(**dict(good, **bad)))) == -1, bad


def test_the_sanitizer_program_of_the_planning_calls(tmp_path):
    """tools/sanitize/mfcc_long_plan.c: pdmp3_amd/host/clip_mfcc_long.c's check, table, taps and plan over the refusals, buffers that
    are too small and every edge of the shapes under AddressSanitizer and UBSan, a stand-alone program on the CPU"""
    run_sanitizer_program(tmp_path, "mfcc_long_plan", ("clip_mfcc_long.c", "clip_mel_long.c", "clip_mel.c", "clip_stft_long.c", "clip_stft.c"))
