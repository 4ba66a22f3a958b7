"""The short-time Fourier transform of clips at n_fft 2048 and 4096, the part that needs no GPU: the
planning calls of pdmp3_amd/host/clip_stft_long.c against the binary64 restatement tests/clip_stft_long_ref.py, the
factorisation against the definition (tests/clip_stft_ref.py) and that against torch.stft in float64 at these lengths, the
derived constant of the bound, and k_clip_stft_long's own index maps, LDS layouts, twiddle step and Nyquist chain
(pdmp3_amd/csrc/stft_long_core.h, compiled here with g++ into tests/host_emul/stft_long_emul.cpp's loops) on random float32
rows against the definition, within the derived binary32 bound -- no value left out."""
import ctypes as C

import numpy as np
import pytest

import clip_stft_long_ref as lref
import clip_stft_ref as ref
from clip_host import MelDesc, build_emul

U = ref.U


class StftLongParams(C.Structure):                 # include/pdmp3_hip.h pdmp3_stft_long_params
    _fields_ = [("n_in", C.c_int64), ("n_fft", C.c_int32), ("n2", C.c_int32), ("hop", C.c_int32), ("bins", C.c_int32),
                ("n_frames", C.c_int32), ("tile", C.c_int32), ("channels", C.c_int32), ("out_mode", C.c_int32), ("floor", C.c_float),
                ("span_floats", C.c_uint32), ("lds_bytes", C.c_uint32)]


def _emul():
    lib = build_emul("stft_long")
    lib.emul_clip_stft_long.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    assert lib.emul_stft_long_desc_bytes() == C.sizeof(MelDesc) and lib.emul_stft_long_params_bytes() == C.sizeof(StftLongParams)
    return lib


def _window(nw, seed):
    """a caller's window: random binary32 values of both signs"""
    return (np.random.default_rng(seed).random(nw, dtype=np.float32) * np.float32(1.5) - np.float32(0.25)).astype(np.float32)


@pytest.mark.parametrize("nw", [None, 1764, 1], ids=["Nw-N", "Nw-1764", "Nw-1"])
@pytest.mark.parametrize("own_window", [False, True], ids=["hann", "own-window"])
@pytest.mark.parametrize("normalized", [False, True], ids=["plain", "normalized"])
@pytest.mark.parametrize("n_fft", lref.SIZES)
def test_tables_are_their_definitions_in_binary64_rounded_once(n_fft, normalized, own_window, nw):
    from pdmp3_amd import api
    nw = nw or n_fft
    win = _window(nw, 1000 + nw) if own_window else None
    got = api.stft_long_tables(n_fft, nw, win, normalized)
    want = lref.tables(n_fft, nw, win, normalized)
    n2 = n_fft // 64
    assert [t.shape for t in got] == [(n_fft,), (64, 128), (2 * n2, n2), (n2, 128)]
    for name, t, w in zip(("wt", "D64", "H2", "TW"), got, want):
        assert t.dtype == np.float32 and t.shape == w.shape and np.isfinite(t).all()
        # one rounding to binary32 of a binary64 value whose own error is a few 2^-53 of a magnitude of at most 1.25
        err = np.abs(t.astype(np.float64) - w)
        assert (err <= U * np.abs(w) + 2.0 ** -50).all(), (name, err.max())
        big = np.abs(w) > 1e-6
        print("N %d Nw %d normalized %d own window %d: %s %s, worst |table - binary64| / (u |value|) = %.3f"
              % (n_fft, nw, normalized, own_window, name, t.shape, (err[big] / (U * np.abs(w[big]))).max(initial=0.0)))
    wt, d64, h2, tw = got
    # wt: exactly 0 outside the window's support (there is no padding in these tables)
    left = (n_fft - nw) // 2
    assert (wt[:left] == 0.0).all() and (wt[left + nw:] == 0.0).all() and (nw == n_fft or left > 0)
    assert (np.abs(wt).sum() > 0) == (own_window or nw > 1)
    # the sine coefficients of k1 = 0 and k2 = 0 -- what bins 0 and N / 2 take their Im from -- are exact zeros
    k2n = n2 // 2
    assert (d64[:, 64] == 0.0).all() and (tw[:, 64] == 0.0).all() and (h2[0::2, k2n] == 0.0).all() and (h2[1::2, 0] == 0.0).all()
    assert (d64[:, 0] == 1.0).all() and (tw[:, 0] == 1.0).all() and (h2[0::2, 0] == 1.0).all() and (h2[1::2, k2n] == 1.0).all()


def test_constant_tables_do_not_depend_on_the_window():
    from pdmp3_amd import api
    for n_fft in lref.SIZES:
        a, b = api.stft_long_tables(n_fft), api.stft_long_tables(n_fft, 1764, _window(1764, 3), True)
        assert not np.array_equal(a[0], b[0])
        for x, y in zip(a[1:], b[1:]):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    a, b = api.stft_long_tables(2048), api.stft_long_tables(4096)
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))          # (the 64-point DFT is shared by both N)


def _frames_case(n_fft, nw, own, normalized, seed):
    hop = n_fft // 3
    F = 5
    win = _window(nw, 2000 + nw) if own else None
    rng = np.random.default_rng(seed)
    start = 3 * n_fft + 5
    T = (F - 1) * hop + n_fft
    y = ((rng.random(start + T) * 2 - 1) * 0.7).astype(np.float32)
    pos0 = start - n_fft // 2
    w = ref.scale(n_fft, normalized) * ref.frame_window(n_fft, nw, win)
    fr = ref.frames_of(y[pos0:pos0 + T].astype(np.float64), pos0, start, F, n_fft, hop)
    A = np.abs(fr * w[None, :]).sum(axis=1)[None, :]
    got, _ = ref.stft(y[pos0:pos0 + T], pos0, start, F, n_fft, hop, 0, win_length=nw, window=win, normalized=normalized)
    return y[pos0:pos0 + T], hop, F, win, fr, A, got[0, :, :, 0] + 1j * got[0, :, :, 1]


CASES64 = [(2048, 2048, False, False), (2048, 1764, True, True), (4096, 4096, False, True), (4096, 1920, True, False)]


@pytest.mark.parametrize("case", CASES64, ids=lambda c: "N%d-Nw%d" % c[:2])
def test_factorisation_in_binary64_is_the_definition(case):
    """the two-stage identity -- index maps, table layouts, the Nyquist bin's chain -- evaluated in binary64 from the binary64
    tables, against clip_stft_ref.stft: within 1e-12 A"""
    n_fft, nw, own, normalized = case
    y, hop, F, win, fr, A, want = _frames_case(n_fft, nw, own, normalized, n_fft * 7 + nw)
    got = lref.two_stage(fr, lref.tables(n_fft, nw, win, normalized))
    assert got.shape == want.shape == (n_fft // 2 + 1, F)
    err = np.abs(got - want)
    assert (A > 0).all() and (err <= 1e-12 * A).all(), float((err / A).max())
    print("N %d Nw %d: worst |two-stage - definition| / A = %.3g" % (n_fft, nw, (err / A).max()))


@pytest.mark.parametrize("case", CASES64, ids=lambda c: "N%d-Nw%d" % c[:2])
def test_restatement_against_torch_stft_in_float64(case):
    """tests/clip_stft_ref.py against torch.stft(center=False, onesided=True) in float64 at N = 2048 and 4096 (section 13's
    pin stopped at 1024)"""
    torch = pytest.importorskip("torch")
    n_fft, nw, own, normalized = case
    y, hop, F, win, fr, A, got = _frames_case(n_fft, nw, own, normalized, n_fft * 11 + nw)
    w = torch.from_numpy(ref.frame_window(nw, nw, win))
    want = torch.stft(torch.from_numpy(np.asarray(y, dtype=np.float64)), n_fft, hop_length=hop, win_length=nw, window=w, normalized=normalized,
                      onesided=True, return_complex=True, center=False).numpy()
    assert want.shape == got.shape == (n_fft // 2 + 1, F)
    err = np.maximum(np.abs(got.real - want.real), np.abs(got.imag - want.imag))
    assert (err <= 1e-12 * A).all(), float((err / A).max())
    assert np.abs(want.imag).max() > 1e-3 * A.max() / n_fft
    print("N %d Nw %d: worst |ref - torch.stft| / A = %.3g" % (n_fft, nw, (err / A).max()))


def test_refusals_of_the_planning_calls():
    from pdmp3_amd import api
    lib = api.load_library()
    assert api.stft_long_check(44100) and api.stft_long_check(48000, n_fft=4096, hop=1024)
    assert api.stft_long_check(44100, n_fft=2048, hop=1, win_length=1, normalized=True) and api.stft_long_check(22050, n_fft=4096, hop=4096, win_length=0)
    assert api.stft_long_check(44100, win_length=1764, window=_window(1764, 1)) and api.stft_long_check(48000, win_length=1920)
    for mode in ("complex", "magnitude", "power"):                          # (the floor is read in the logarithms' modes only)
        assert api.stft_long_check(44100, mode=mode, floor=0.0) and api.stft_long_check(44100, mode=mode, floor=float("nan"))
    # every n_fft other than 2048 / 4096
    for n_fft in (0, 16, 400, 512, 1024, 1026, 1536, 2046, 2047, 2049, 2050, 3072, 4094, 4098, 8192, 16384, -2048):
        assert not api.stft_long_check(44100, n_fft=n_fft, hop=1), n_fft
        with pytest.raises(ValueError):
            api.stft_long_plan(n_fft, 1)
        with pytest.raises(ValueError):
            api.stft_long_tables(n_fft)
    bad_window = _window(2048, 2)
    refused = [dict(hop=0), dict(hop=2049), dict(hop=-1), dict(n_fft=4096, hop=4097), dict(win_length=2049), dict(win_length=-1),
               dict(n_fft=4096, hop=512, win_length=4097), dict(n_frames=-1), dict(mode=5), dict(mode=-1), dict(mode="log", floor=0.0),
               dict(mode="log10", floor=0.0), dict(mode="log10", floor=-1e-10), dict(mode="log", floor=float("nan")), dict(mode="log10", floor=1e-46),
               dict(mode="log10", floor=float("inf")), dict(normalized=2)]
    for value in (np.nan, np.inf, -np.inf):
        for at in (0, 1023, 2047):
            w = bad_window.copy()
            w[at] = value
            refused.append(dict(window=w))
    for bad in refused:
        if "normalized" in bad:                                              # (the Python wrapper makes a bool of it: the C call)
            spec, keep = api._stft_spec(n_fft=2048, hop=512)
            spec.normalized = 2
            assert lib.pdmp3_amd_stft_long_check(C.byref(spec), 44100) != 0
            continue
        assert not api.stft_long_check(44100, **bad), bad
    assert not api.stft_long_check(0) and not api.stft_long_check(-1)
    for kw in (dict(n_fft=2048, win_length=2049), dict(n_fft=2048, win_length=-1), dict(n_fft=2048, window=np.array([1.0, np.nan], dtype=np.float32))):
        with pytest.raises(ValueError):
            api.stft_long_tables(**kw)
    with pytest.raises(ValueError):                                         # (a window of another length than win_length)
        api.stft_long_tables(2048, 1764, _window(1765, 1))
    for n_fft, hop, mode in ((2048, 0, 0), (2048, 2049, 0), (4096, 4097, 0), (2048, 512, 5), (2048, 512, -1)):
        with pytest.raises(ValueError):
            api.stft_long_plan(n_fft, hop, mode)
    # NULL pointers
    spec, keep = api._stft_spec(n_fft=2048, hop=512)
    assert lib.pdmp3_amd_stft_long_check(None, 44100) == -1
    assert lib.pdmp3_amd_stft_long_tables(None, None, 0, None) == -1
    assert lib.pdmp3_amd_stft_long_tables(C.byref(spec), None, 0, None) == 2048 + 8192 + 2048 + 4096
    assert lib.pdmp3_amd_stft_long_plan(2048, 512, 0, None, None, None) == 0
    assert lib.pdmp3_amd_bulk_decode_clips_stft_long(None, None, 0, C.byref(spec), None) == -1
    # a cap below the whole: only that many floats are written
    buf = np.full(3000, np.float32(-7.0), dtype=np.float32)
    assert lib.pdmp3_amd_stft_long_tables(C.byref(spec), buf.ctypes.data_as(C.c_void_p), 2100, None) == 16384
    assert (buf[2100:] == -7.0).all() and (buf[2048:2100] != -7.0).all()
    # the calls of section 13 keep refusing these lengths
    assert not api.stft_check(44100, n_fft=2048, hop=512) and not api.stft_check(44100, n_fft=4096, hop=1024)


def test_the_plan_is_the_restated_one_and_keeps_the_kernels_preconditions():
    """a grid of hops, both N, every mode: the call's plan is the restated one, the span, the staging tile and Z fit the LDS
    asked for, at most PDMP3_MEL_LDS_MAX; every launch path is hit in both mode classes"""
    from pdmp3_amd import api
    paths = {(p, c): 0 for p in lref.PATHS for c in ("complex", "real")}
    for n_fft in lref.SIZES:
        n2 = n_fft // 64
        edge = 1500 if n_fft == 2048 else 2923                               # (the last hop of the larger tile: section 14's arithmetic)
        for hop in (1, 2, 441, 512, 1024, n_fft // 2 + 1, edge, edge + 1, n_fft - 1, n_fft):
            for mode in range(5):
                tile, pad, lds = api.stft_long_plan(n_fft, hop, mode)
                want = lref.plan(n_fft, hop, mode)
                assert (tile, pad, lds) == want[:3], (n_fft, hop, mode)
                assert pad == 0 and lds <= lref.LDS_MAX and want[3] == "N%d-tile%d" % (n_fft, tile) and want[3] in lref.PATHS
                first = lds // 4 - tile * n2 * 32
                assert first % 4 == 0 and first >= (tile - 1) * hop + n_fft and first >= (2 if mode == 0 else 1) * 16 * (n2 // 2) * (tile + 1)
                assert lds > 64 * 1024                                       # (every plan runs on the static array)
                paths[want[3], "complex" if mode == 0 else "real"] += 1
        assert api.stft_long_plan(n_fft, edge)[0] == 2 * api.stft_long_plan(n_fft, edge + 1)[0]
    assert all(paths.values()), paths
    assert api.stft_long_plan(2048, 512)[0] == 16 and api.stft_long_plan(2048, 2048)[::2] == (8, 96 * 1024)
    assert api.stft_long_plan(4096, 1024)[0] == 8 and api.stft_long_plan(4096, 4096)[::2] == (4, 96 * 1024)
    print("launch paths over the grid: %s" % paths)


def test_the_two_stage_bound_is_tighter_than_the_direct_chains():
    for n_fft in lref.SIZES:
        c = lref.c_of(n_fft)
        n2 = n_fft // 64
        print("c(%d) = %.4f (N + 2 = %d)" % (n_fft, c, n_fft + 2))
        assert 64 + 2 * n2 < c < 64 + 3 * n2 + 12 < n_fft + 2


EMUL_CASES = [
    # n_fft, hop, win_length, own window, normalized, channels, start, n_frames, J - start (None: the row is all signal)
    (2048, 512, 2048, False, False, 2, 0, 21, None),              # leading zeros: N / 2 of them; a full tile of 16 and a partial one
    (2048, 441, 1764, True, True, 1, 57, 19, 6000),               # start inside the first N / 2 samples; valid = 14 ends inside a tile
    (2048, 2048, 2048, False, False, 1, 5000, 11, 9000),          # H = N: the tile of 8; valid = 5
    (4096, 1024, 4096, False, True, 1, 300, 18, 12000),           # N2 = 64, tile of 8; valid = 12
    (4096, 4096, 1920, True, False, 2, 100, 5, None),             # the tile of 4
    (2048, 1, 1, True, False, 1, 3, 40, None),                    # H = 1, a window of one tap
    (4096, 3000, 4096, False, False, 1, 100000, 6, -7),           # wholly behind J: silent frames only
]


@pytest.mark.parametrize("case", EMUL_CASES, ids=lambda c: "N%d-H%d-Nw%d-C%d-s%d" % (c[0], c[1], c[2], c[5], c[6]))
def test_kernel_arithmetic_on_the_host_against_binary64(case):
    from pdmp3_amd import api
    lib = _emul()
    n_fft, hop, nw, own, normalized, channels, start, F, left = case
    rng = np.random.default_rng((n_fft * 131 + hop * 17 + start) & 0xffffffff)
    win = _window(nw, 3000 + nw) if own else None
    K = n_fft // 2 + 1
    n2 = n_fft // 64
    tab = np.concatenate([t.ravel() for t in api.stft_long_tables(n_fft, nw, win, normalized)])
    # the row as the call stages it: from max(0, start - N / 2) on, zeros from J on
    s0 = max(0, start - n_fft // 2)
    lead = s0 - (start - n_fft // 2)
    T = (F - 1) * hop + n_fft
    Ts = (T + 3) // 4 * 4
    stage = np.full(channels * Ts + 16, np.float32(7e8), dtype=np.float32)        # (guards: nothing outside [0, T) may be read)
    rows = stage[8:8 + channels * Ts].reshape(channels, Ts)
    rows[:, :T] = (rng.random((channels, T), dtype=np.float32) * 2 - 1) * np.float32(0.7)
    if left is not None:
        rows[:, max(0, start + left - s0):T] = 0.0
    y = rows[:, :T].copy()
    w = ref.scale(n_fft, normalized) * ref.frame_window(n_fft, nw, win)
    signal = np.abs(ref.frames_of(y[0], s0, start, F, n_fft, hop) * w[None, :]).sum(axis=1) > 0
    nv = ref.valid(start + left if left is not None else 2 ** 62, start, hop, F)
    floors = {3: 1e-6, 4: 1e-10}
    wants = lref.stft_all(y, s0, start, F, n_fft, hop, floors, nw, win, normalized)
    outs = {}
    for mode in range(5):
        tile, row_pad, lds_bytes = api.stft_long_plan(n_fft, hop, mode)
        per = K * F * (2 if mode == 0 else 1)
        out = np.full((channels, per + 8), np.float32(-3e9), dtype=np.float32)
        d = MelDesc(src=rows.ctypes.data, dst=out.ctypes.data, src_chan_stride=Ts, dst_chan_stride=per + 8, lead=lead)
        P = StftLongParams(n_in=T, n_fft=n_fft, n2=n2, hop=hop, bins=K, n_frames=F, tile=tile, channels=channels, out_mode=mode,
                           floor=floors.get(mode, 0.0), span_floats=lds_bytes // 4 - tile * n2 * 32, lds_bytes=lds_bytes)
        assert lib.emul_clip_stft_long(C.byref(d), 1, tab.ctypes.data, C.byref(P)) == 0
        assert (out[:, per:] == np.float32(-3e9)).all() and (out[:, :per] != np.float32(-3e9)).all()
        got32 = out[:, :per].reshape((channels, K, F, 2) if mode == 0 else (channels, K, F))
        outs[mode] = got32
        got = got32.astype(np.float64)
        want, bound = wants[mode]
        assert want.shape == got.shape
        err = np.abs(got - want)
        assert (err <= bound).all(), (mode, float((err - bound).max()))
        ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
        print("N %d H %d Nw %d C %d start %d mode %d tile %d (%s): worst error / bound %.4f (%d of %d frames hold signal, valid %d)"
              % (n_fft, hop, nw, channels, start, mode, tile, lref.plan(n_fft, hop, mode)[3], ratio, signal.sum(), F, nv))
        if signal.any():
            assert 0.0 < ratio <= 1.0
        if mode <= 2:
            # silence: the bound is 0 there and the value exactly 0.0
            assert (bound[:, :, ~signal] == 0.0).all() and (got[:, :, ~signal] == 0.0).all()
    # Im of bins 0 and N / 2 is exactly zero
    assert (outs[0][:, 0, :, 1] == 0.0).all() and (outs[0][:, K - 1, :, 1] == 0.0).all()
    if signal.any():
        assert np.abs(outs[0][:, 0, :, 0]).max() > 0 and np.abs(outs[0][:, K - 1, :, 0]).max() > 0
    # modes 1 and 2 are mode 0's pair through the product's own arithmetic, bit for bit
    p = ref.power_as_the_product(outs[0][..., 0], outs[0][..., 1])
    assert np.array_equal(p.view(np.uint32), outs[2].view(np.uint32))
    assert np.array_equal(np.sqrt(p).view(np.uint32), outs[1].view(np.uint32))
    if left is not None:
        assert nv < F and not signal[nv + (n_fft // 2 + hop - 1) // hop:].any()


def test_the_cases_cover_every_launch_path_silent_frames_and_a_valid_inside_a_tile():
    from pdmp3_amd import api
    inside, silent, paths = 0, 0, set()
    for n_fft, hop, nw, own, normalized, channels, start, F, left in EMUL_CASES:
        paths.add(lref.plan(n_fft, hop, 0)[3])
        if left is None:
            continue
        nv = ref.valid(start + left, start, hop, F)
        tile = api.stft_long_plan(n_fft, hop, 0)[0]
        inside += 0 < nv < F and nv % tile != 0
        silent += nv + (n_fft // 2 + hop - 1) // hop < F
    assert paths == set(lref.PATHS) and inside >= 3 and silent >= 3


def test_the_emulator_refuses_parameters_that_leave_the_lds():
    lib = _emul()
    d = MelDesc()
    tab = np.zeros(1, dtype=np.float32)
    ok = dict(n_in=0, n_fft=2048, n2=32, hop=512, bins=1025, n_frames=0, tile=16, channels=1, out_mode=0, floor=0.0,
              span_floats=(15 * 512 + 2048), lds_bytes=(15 * 512 + 2048 + 16 * 32 * 32) * 4)
    assert lib.emul_clip_stft_long(C.byref(d), 1, tab.ctypes.data, C.byref(StftLongParams(**ok))) == 0
    for bad in (dict(span_floats=ok["span_floats"] - 4), dict(lds_bytes=ok["lds_bytes"] - 4), dict(tile=4), dict(n2=64), dict(hop=513),
                dict(lds_bytes=160 * 1024, span_floats=160 * 256 - 16 * 32 * 32)):
        assert lib.emul_clip_stft_long(C.byref(d), 1, tab.ctypes.data, C.byref(StftLongParams(**dict(ok, **bad)))) == -1, bad
