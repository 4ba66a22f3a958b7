"""The short-time Fourier transform of clips, the part that needs no GPU: the planning calls of
pdmp3_amd/host/clip_stft.c against the binary64 restatement tests/clip_stft_ref.py, that restatement against torch.stft in
float64 (an implementation from outside), and k_clip_stft's own indexing, pointwise arithmetic and staging layout
(pdmp3_amd/csrc/stft_core.h, compiled here with g++ into tests/host_emul/stft_emul.cpp's loops) on random float32 rows against
the definition, within the derived binary32 bound -- no value left out."""
import ctypes as C

import numpy as np
import pytest

import clip_stft_ref as ref
from clip_host import MelDesc, build_emul

U = ref.U

SHAPES = [(16, 16), (400, 400), (400, 301), (512, 1), (1024, 1024)]          # (N, Nw)


class StftParams(C.Structure):                     # include/pdmp3_hip.h pdmp3_stft_params
    _fields_ = [("n_in", C.c_int64), ("n_fft", C.c_int32), ("rows", C.c_int32), ("hop", C.c_int32), ("row_pad", C.c_int32),
                ("bins", C.c_int32), ("bins16", C.c_int32), ("n_frames", C.c_int32), ("tile", C.c_int32), ("channels", C.c_int32),
                ("out_mode", C.c_int32), ("floor", C.c_float), ("span_floats", C.c_uint32), ("lds_bytes", C.c_uint32)]


def _emul():
    lib = build_emul("stft")
    lib.emul_clip_stft.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    assert lib.emul_stft_desc_bytes() == C.sizeof(MelDesc) and lib.emul_stft_params_bytes() == C.sizeof(StftParams)
    return lib


def _window(nw, seed):
    """a caller's window: random binary32 values of both signs"""
    return (np.random.default_rng(seed).random(nw, dtype=np.float32) * np.float32(1.5) - np.float32(0.25)).astype(np.float32)


@pytest.mark.parametrize("own_window", [False, True], ids=["hann", "own-window"])
@pytest.mark.parametrize("normalized", [False, True], ids=["plain", "normalized"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "N%d-Nw%d" % s)
def test_table_is_the_definition_in_binary64_rounded_once(shape, normalized, own_window):
    from pdmp3_amd import api
    n_fft, nw = shape
    win = _window(nw, 1000 + nw) if own_window else None
    t = api.stft_table(n_fft, nw, win, normalized)
    want = ref.table(n_fft, nw, win, normalized)
    assert t.shape == want.shape and t.dtype == np.float32
    K = n_fft // 2 + 1
    Kp = want.shape[1] // 2
    # one rounding to binary32 of a binary64 value whose own error is a few 2^-53 of the row's |s w[n]| (<= 1.25)
    err = np.abs(t.astype(np.float64) - want)
    assert (err <= U * np.abs(want) + 2.0 ** -50).all(), err.max()
    # the padding and the rows outside the window's support: exactly 0
    left = (n_fft - nw) // 2
    zero = np.ones(want.shape, dtype=bool)
    zero[left:left + nw, :K] = False
    zero[left:left + nw, Kp:Kp + K] = False
    assert (t[zero] == 0.0).all() and zero.sum() > 0 and np.isfinite(t).all()
    # (the periodic Hann window of one tap is its formula's value, 0: the transform of that frame is 0)
    assert (np.abs(t[left:left + nw]).sum() > 0) == (own_window or nw > 1)
    big = np.abs(want) > 1e-6
    print("N %d Nw %d normalized %d own window %d: table %s, worst |table - binary64| / (u |value|) = %.3f"
          % (n_fft, nw, normalized, own_window, t.shape, (err[big] / (U * np.abs(want[big]))).max(initial=0.0)))


@pytest.mark.parametrize("n_fft", [16, 400, 512, 1024])
def test_default_table_is_the_log_mel_calls_bit_for_bit(n_fft):
    from pdmp3_amd import api
    a, b = api.stft_table(n_fft), api.mel_dft_table(n_fft)
    assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(api.stft_table(n_fft, n_fft).view(np.uint32), b.view(np.uint32))
    assert not np.array_equal(api.stft_table(n_fft, normalized=True).view(np.uint32), b.view(np.uint32))


def _torch_stft(y, n_fft, hop, nw, win, normalized, **kw):
    import torch
    w = torch.from_numpy(ref.frame_window(nw, nw, win))            # (the Nw values in binary64; torch centres them itself)
    x = torch.stft(torch.from_numpy(np.asarray(y, dtype=np.float64)), n_fft, hop_length=hop, win_length=nw, window=w, normalized=normalized,
                   onesided=True, return_complex=True, **kw)
    return x.numpy()                                               # [K, F]


@pytest.mark.parametrize("own_window", [False, True], ids=["hann", "own-window"])
@pytest.mark.parametrize("normalized", [False, True], ids=["plain", "normalized"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "N%d-Nw%d" % s)
def test_restatement_against_torch_stft_in_float64(shape, normalized, own_window):
    """tests/clip_stft_ref.py against an implementation from outside: torch.stft, float64, center=False on the span from
    start - N / 2 on.  Agreement within 1e-12 A of the frame (observed: below 1e-15 A)."""
    torch = pytest.importorskip("torch")
    assert hasattr(torch, "stft")
    n_fft, nw = shape
    hop = max(1, n_fft // 3)
    F = 9
    win = _window(nw, 2000 + nw) if own_window else None
    rng = np.random.default_rng(n_fft * 7 + nw)
    start = 3 * n_fft + 5
    T = (F - 1) * hop + n_fft
    y = ((rng.random(start + T) * 2 - 1) * 0.7).astype(np.float32)
    pos0 = start - n_fft // 2
    got, _ = ref.stft(y[pos0:pos0 + T], pos0, start, F, n_fft, hop, 0, win_length=nw, window=win, normalized=normalized)
    want = _torch_stft(y[pos0:pos0 + T], n_fft, hop, nw, win, normalized, center=False)
    assert want.shape == (n_fft // 2 + 1, F)
    w = ref.scale(n_fft, normalized) * ref.frame_window(n_fft, nw, win)
    A = np.abs(ref.frames_of(y[pos0:pos0 + T], pos0, start, F, n_fft, hop) * w[None, :]).sum(axis=1)[None, :]
    err = np.maximum(np.abs(got[0, :, :, 0] - want.real), np.abs(got[0, :, :, 1] - want.imag))
    if nw == 1 and not own_window:                                          # (the Hann window of one tap is 0: both are exactly 0)
        assert (A == 0).all() and (err == 0).all()
        return
    assert (A > 0).all() and (err <= 1e-12 * A).all(), float((err / A).max())
    assert np.abs(want.imag).max() > 1e-3 * A.max() / n_fft                 # (Im is there to be compared, sign included)
    print("N %d Nw %d normalized %d own window %d: worst |ref - torch.stft| / A = %.3g" % (n_fft, nw, normalized, own_window, (err / A).max()))


def test_stream_start_frames_are_center_true_with_constant_padding():
    """a clip at start 0: the frames that reach in front of the stream read zeros, which is torch.stft(center=True,
    pad_mode="constant") on the stream's first samples (hop divides N / 2, so the frame grids coincide)"""
    torch = pytest.importorskip("torch")
    n_fft, hop, nw, F = 400, 50, 301, 12
    assert (n_fft // 2) % hop == 0
    win = _window(nw, 77)
    rng = np.random.default_rng(5)
    L = (F - 1) * hop                                                       # center=True gives 1 + L // hop = F frames
    y = ((rng.random(L) * 2 - 1) * 0.7).astype(np.float32)
    for normalized in (False, True):
        got, _ = ref.stft(y, 0, 0, F, n_fft, hop, 0, win_length=nw, window=win, normalized=normalized)
        want = _torch_stft(y, n_fft, hop, nw, win, normalized, center=True, pad_mode="constant")
        assert want.shape == (n_fft // 2 + 1, F)
        w = ref.scale(n_fft, normalized) * ref.frame_window(n_fft, nw, win)
        A = np.abs(ref.frames_of(y, 0, 0, F, n_fft, hop) * w[None, :]).sum(axis=1)[None, :]
        err = np.maximum(np.abs(got[0, :, :, 0] - want.real), np.abs(got[0, :, :, 1] - want.imag))
        assert (err <= 1e-12 * A).all(), float((err / A).max())
        print("center=True, constant padding, normalized %d: worst |ref - torch.stft| / A = %.3g" % (normalized, (err / A).max()))


def test_refusals_of_the_planning_calls():
    from pdmp3_amd import api
    assert api.stft_check(16000)
    assert api.stft_check(16000, n_fft=16, hop=16, win_length=1) and api.stft_check(48000, n_fft=1024, hop=1, win_length=1024, normalized=True)
    assert api.stft_check(16000, win_length=301, window=_window(301, 1)) and api.stft_check(16000, win_length=0)
    for mode in ("complex", "magnitude", "power"):                          # (the floor is read in the logarithms' modes only)
        assert api.stft_check(16000, mode=mode, floor=0.0) and api.stft_check(16000, mode=mode, floor=float("nan"))
    bad_window = _window(400, 2)
    refused = [dict(n_fft=401), dict(n_fft=14), dict(n_fft=1026), dict(n_fft=2048), dict(hop=0), dict(hop=401), dict(hop=-1), dict(win_length=401),
               dict(win_length=-1), dict(n_frames=-1), dict(mode=5), dict(mode=-1), dict(mode="log", floor=0.0), dict(mode="log10", floor=0.0),
               dict(mode="log10", floor=-1e-10), dict(mode="log", floor=float("nan")), dict(mode="log10", floor=1e-46),
               dict(mode="log10", floor=float("inf"))]
    for value in (np.nan, np.inf, -np.inf):
        for at in (0, 199, 399):
            w = bad_window.copy()
            w[at] = value
            refused.append(dict(window=w))
    for bad in refused:
        assert not api.stft_check(16000, **bad), bad
    assert not api.stft_check(0) and not api.stft_check(-1)
    for kw in (dict(n_fft=401), dict(n_fft=14), dict(n_fft=1026), dict(n_fft=400, win_length=401), dict(n_fft=400, win_length=-1),
               dict(n_fft=400, window=np.array([1.0, np.nan], dtype=np.float32))):
        with pytest.raises(ValueError):
            api.stft_table(**kw)
    with pytest.raises(ValueError):                                         # (a window of another length than win_length)
        api.stft_table(400, 300, _window(301, 1))
    for n_fft, hop, mode in ((401, 1, 0), (14, 1, 0), (1026, 1, 0), (400, 0, 0), (400, 401, 0), (400, 160, 5), (400, 160, -1)):
        with pytest.raises(ValueError):
            api.stft_tile(n_fft, hop, mode)


def tile_sweep():
    """(n_fft, hop, mode) of the grid the plan is walked over (tests/test_clip_forms_host.py walks it too)"""
    for n_fft in (16, 18, 398, 400, 512, 1022, 1024):
        for hop in sorted(set([1, 2, 3, 4, 5, 31, 32, 33, 64, 128, 160, 450, 512, 900, n_fft // 2, n_fft - 1, n_fft]) & set(range(1, n_fft + 1))):
            for mode in range(5):
                yield n_fft, hop, mode


def test_the_tile_is_the_plan_restated_and_keeps_the_kernels_preconditions():
    """every (N, H, mode) of a grid: the call's plan is the restated one, the span in its padded chunks and the four staging
    tiles fit the LDS asked for, at most 160 KB; every launch path is hit"""
    from pdmp3_amd import api
    paths = {"tile32": 0, "tile16": 0, "tile16-static": 0}
    for n_fft, hop, mode in tile_sweep():
        tile, pad, lds = api.stft_tile(n_fft, hop, mode)
        want = ref.tile_plan(n_fft, hop, mode)
        assert (tile, pad, lds) == want[:3], (n_fft, hop, mode)
        rows = (n_fft + 3) // 4 * 4
        assert tile in (16, 32) and 0 <= pad < 32 and (hop + pad) % 32 == 2 and lds <= 160 * 1024 - 64
        stage = 4 * (2 if mode == 0 else 1) * 16 * (tile + 4)
        first = lds // 4 - stage
        assert first % 4 == 0 and first >= -(-((tile - 1) * hop + rows) // hop) * (hop + pad)
        assert (want[3] == "tile32") == (tile == 32) and (want[3] == "tile16-static") == (lds > 64 * 1024)
        paths[want[3]] += 1
    assert all(paths.values()), paths
    assert api.stft_tile(400, 160)[0] == 32 and api.stft_tile(1024, 512)[0] == 16 and api.stft_tile(1024, 512)[2] <= 64 * 1024
    assert api.stft_tile(1024, 1024)[0] == 16 and api.stft_tile(1024, 1024)[2] > 64 * 1024
    print("launch paths over the grid: %s" % paths)


EMUL_CASES = [
    # n_fft, hop, win_length, own window, normalized, channels, start, n_frames, J - start (None: the row is all signal)
    (400, 160, 400, False, False, 1, 0, 35, None),                # leading zeros: N / 2 of them; valid ends the second tile early
    (400, 160, 301, True, True, 2, 57, 33, None),                 # start inside the first N / 2 samples
    (400, 160, 400, False, False, 1, 5000, 40, 3000),             # frames across and behind J: valid = 19 ends inside a tile
    (400, 160, 400, True, False, 2, 100000, 31, -7),              # wholly behind J: silent frames only
    (512, 128, 1, True, True, 2, 1000, 34, 4000),                 # a window of one tap
    (1024, 1024, 1024, False, False, 1, 300, 18, 9000),           # H = N: tile of 16 on the static array
    (1024, 512, 1024, False, True, 1, 300, 19, 5000),             # tile of 16 inside 64 KB
    (1024, 1, 1000, True, False, 1, 3, 37, None),                 # H = 1
    (16, 1, 16, False, False, 2, 2, 70, 40),
    (16, 16, 7, True, False, 1, 0, 33, 400),
    (398, 3, 398, False, True, 1, 50, 36, None),                  # N not a multiple of 4, a hop below 4
]


def _edge_case(e):
    """an entry of clip_stft_ref.EDGES as a case: one full tile of the mode with the larger tile and a partial one, the row all
    signal (a caller's window: one of this module's, of the entry's length)"""
    tile = max(ref.form(e["n_fft"], e["hop"], m)[0] for m in range(5))
    return (e["n_fft"], e["hop"], e.get("win_length") or e["n_fft"], "window" in e, e.get("normalized", False), e["channels"], 57, tile + 3, None)


EMUL_CASES += [_edge_case(e) for e in ref.EDGES.values()]


@pytest.mark.parametrize("case", EMUL_CASES, ids=lambda c: "N%d-H%d-Nw%d-C%d-s%d" % (c[0], c[1], c[2], c[5], c[6]))
def test_kernel_arithmetic_on_the_host_against_binary64(case):
    from pdmp3_amd import api
    lib = _emul()
    n_fft, hop, nw, own, normalized, channels, start, F, left = case
    rng = np.random.default_rng((n_fft * 131 + hop * 17 + start) & 0xffffffff)
    win = _window(nw, 3000 + nw) if own else None
    K = n_fft // 2 + 1
    Kp = (K + 15) // 16 * 16
    tab = api.stft_table(n_fft, nw, win, normalized)
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
    outs = {}
    for mode in range(5):
        floor = {3: 1e-6, 4: 1e-10}.get(mode, 0.0)
        tile, row_pad, lds_bytes = api.stft_tile(n_fft, hop, mode)
        per = K * F * (2 if mode == 0 else 1)
        out = np.full((channels, per + 8), np.float32(-3e9), dtype=np.float32)
        d = MelDesc(src=rows.ctypes.data, dst=out.ctypes.data, src_chan_stride=Ts, dst_chan_stride=per + 8, lead=lead)
        P = StftParams(n_in=T, n_fft=n_fft, rows=(n_fft + 3) // 4 * 4, hop=hop, row_pad=row_pad, bins=K, bins16=Kp, n_frames=F, tile=tile,
                       channels=channels, out_mode=mode, floor=floor, span_floats=lds_bytes // 4 - 4 * (2 if mode == 0 else 1) * 16 * (tile + 4),
                       lds_bytes=lds_bytes)
        assert lib.emul_clip_stft(C.byref(d), 1, tab.ctypes.data, C.byref(P)) == 0
        assert (out[:, per:] == np.float32(-3e9)).all()
        got32 = out[:, :per].reshape((channels, K, F, 2) if mode == 0 else (channels, K, F))
        outs[mode] = got32
        got = got32.astype(np.float64)
        want, bound = ref.stft(y, s0, start, F, n_fft, hop, mode, floor or 1e-10, nw, win, normalized)
        assert want.shape == got.shape
        err = np.abs(got - want)
        assert (err <= bound).all(), (mode, float((err - bound).max()))
        ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
        print("N %d H %d Nw %d C %d start %d mode %d tile %d (%s): worst error / bound %.4f (%d of %d frames hold signal, valid %d)"
              % (n_fft, hop, nw, channels, start, mode, tile, ref.tile_plan(n_fft, hop, mode)[3], ratio, signal.sum(), F, nv))
        if signal.any():
            assert 0.0 < ratio <= 1.0
        if mode <= 2:
            # silence: the bound is 0 there and the value exactly 0.0
            silent = (bound[:, :, ~signal] == 0.0).all() and (got[:, :, ~signal] == 0.0).all()
            assert silent
    # modes 1 and 2 are mode 0's pair through the product's own arithmetic, bit for bit
    p = ref.power_as_the_product(outs[0][..., 0], outs[0][..., 1])
    assert np.array_equal(p.view(np.uint32), outs[2].view(np.uint32))
    assert np.array_equal(np.sqrt(p).view(np.uint32), outs[1].view(np.uint32))
    if left is not None:
        assert nv < F and not signal[nv + (n_fft // 2 + hop - 1) // hop:].any()


def test_the_cases_hold_silent_frames_and_a_valid_inside_a_tile():
    from pdmp3_amd import api
    inside, silent = 0, 0
    for n_fft, hop, nw, own, normalized, channels, start, F, left in EMUL_CASES:
        if left is None:
            continue
        nv = ref.valid(start + left, start, hop, F)
        tile = api.stft_tile(n_fft, hop, 0)[0]
        inside += 0 < nv < F and nv % tile != 0
        silent += nv + (n_fft // 2 + hop - 1) // hop < F
    assert inside >= 3 and silent >= 3
