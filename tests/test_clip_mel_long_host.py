"""Log-mel features of clips at n_fft 2048 and 4096, the part that needs no GPU: the planning calls of
pdmp3_amd/host/clip_mel_long.c against the restatements (tests/clip_mel_ref.py's filterbank, tests/clip_mel_long_ref.py's plan
and order of the bins), their refusals, and k_clip_mel_long's own index maps and LDS layouts (pdmp3_amd/csrc/mel_long_core.h,
compiled here with g++ into tests/host_emul/mel_long_emul.cpp's loops) on random float32 rows against the definition in
binary64, within the derived binary32 bound -- no value left out."""
import ctypes as C
import itertools

import numpy as np
import pytest

import clip_mel_long_ref as mlref
import clip_mel_ref as mref
import clip_stft_ref as sref
from clip_host import MelDesc, build_emul

U = mref.U


class MelLongParams(C.Structure):                  # include/pdmp3_hip.h pdmp3_mel_long_params
    _fields_ = [("n_in", C.c_int64), ("n_fft", C.c_int32), ("n2", C.c_int32), ("hop", C.c_int32), ("n_mels", C.c_int32),
                ("mels16", C.c_int32), ("n_frames", C.c_int32), ("tile", C.c_int32), ("channels", C.c_int32), ("out_mode", C.c_int32),
                ("floor", C.c_float), ("span_floats", C.c_uint32), ("lds_bytes", C.c_uint32)]


def _emul():
    lib = build_emul("mel_long")
    lib.emul_clip_mel_long.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.emul_mel_long_lds_floats.restype = C.c_uint
    assert lib.emul_mel_long_desc_bytes() == C.sizeof(MelDesc) and lib.emul_mel_long_params_bytes() == C.sizeof(MelLongParams)
    return lib


def _window(nw, seed):
    return (np.random.default_rng(seed).random(nw, dtype=np.float32) * np.float32(1.5) - np.float32(0.25)).astype(np.float32)


def _ends(sr):
    """(f_min, f_max) inside and at the ends of what the check accepts"""
    return [(0.0, 0.0), (0.0, sr / 2.0), (20.0, sr / 2.0 - 100.0), (300.0, 3400.0), (0.0, sr / 4.0)]


@pytest.mark.parametrize("n_fft", mlref.SIZES)
@pytest.mark.parametrize("sr", [8000, 16000, 22050, 44100, 48000])
def test_filterbank_is_the_restatement_rounded_once_and_its_end_columns_are_zero(sr, n_fft):
    from pdmp3_amd import api
    K = n_fft // 2 + 1
    for n_mels, scale, norm, (f_min, f_max) in itertools.product((1, 17, 128, 256), ("slaney", "htk"), ("slaney", None), _ends(sr)):
        got = api.mel_long_filterbank(sr, n_fft, n_mels, f_min, f_max, scale, norm)
        want = mref.filterbank(sr, n_fft, n_mels, f_min, f_max, scale, norm)
        assert got.shape == want.shape == (n_mels, K) and got.dtype == np.float32 and np.isfinite(got).all()
        # one rounding to binary32 of a binary64 value whose own error is a few 2^-53 relative to the quotients it is made of
        err = np.abs(got.astype(np.float64) - want)
        assert (err <= U * np.abs(want) + 1e-13 * np.abs(want).max()).all(), (sr, n_fft, n_mels, scale, norm, f_min, f_max, err.max())
        assert (got >= 0.0).all()
        # the Nyquist bin's weight is exactly 0 (f_max <= sr / 2 and the last edge is f_max): what lets the kernel leave it out
        assert (got[:, K - 1] == 0.0).all() and (want[:, K - 1] == 0.0).all()
        if f_min == 0.0:
            assert (got[:, 0] == 0.0).all()
        empty = np.flatnonzero(~(got > 0).any(axis=1))
        assert np.array_equal(empty, np.flatnonzero(~(want > 0).any(axis=1)))
        if empty.size:
            print("sr %d N %d n_mels %d %s f %g..%g: all-zero rows %s" % (sr, n_fft, n_mels, scale, f_min, f_max, empty.tolist()))


@pytest.mark.parametrize("n_fft", mlref.SIZES)
def test_operand_is_a_permutation_of_the_dense_filterbank_at_the_core_headers_places(n_fft):
    from pdmp3_amd import api
    lib = _emul()
    n2 = n_fft // 64
    rows = [lib.emul_mel_long_operand_row(k, n2) for k in range(n_fft // 2)]
    assert sorted(rows) == list(range(n_fft // 2))                           # every bin 0 .. N / 2 - 1 exactly once
    assert rows == [mlref.operand_row(k, n_fft) for k in range(n_fft // 2)]
    for kt in range(4):                                                        # a tile of k1 fills its own 8 N2 rows
        own = [rows[k] for k in range(n_fft // 2) if (k % 64) // 16 == kt]
        assert sorted(own) == list(range(8 * n2 * kt, 8 * n2 * (kt + 1)))
    for sr, n_mels, scale, norm in ((22050, 128, "slaney", "slaney"), (48000, 17, "htk", None), (44100, 1, "slaney", "slaney"), (16000, 256, "htk", "slaney")):
        w = api.mel_long_filterbank(sr, n_fft, n_mels, 0.0, 0.0, scale, norm)
        op = api.mel_long_operand(sr, n_fft, n_mels, 0.0, 0.0, scale, norm)
        mp = (n_mels + 15) // 16 * 16
        assert op.shape == (n_fft // 2, mp) and op.dtype == np.float32
        assert np.array_equal(op[rows, :n_mels].view(np.uint32), w[:, :n_fft // 2].T.copy().view(np.uint32))
        assert (op[:, n_mels:].view(np.uint32) == 0).all()                     # the bands' padding: exactly +0


def test_refusals_write_nothing():
    from pdmp3_amd import api
    lib = api.load_library()
    assert api.mel_long_check(22050) and api.mel_long_check(48000, n_fft=4096, hop=1024) and api.mel_long_check(44100, hop=1, n_mels=256)
    assert api.mel_long_check(44100, win_length=1764, window=_window(1764, 1)) and api.mel_long_check(48000, win_length=1920, mode="power")
    assert api.mel_long_check(22050, n_fft=4096, hop=4096, n_mels=1, mode="log", f_min=20.0, f_max=11025.0)
    bad_window = _window(2048, 2)
    bad_window[77] = np.nan
    refused = [dict(n_fft=1024), dict(n_fft=8192), dict(n_fft=2047), dict(n_fft=2049), dict(n_fft=4095), dict(n_fft=400), dict(n_fft=0),
               dict(hop=0), dict(hop=2049), dict(n_fft=4096, hop=4097), dict(hop=-1), dict(n_mels=0), dict(n_mels=257),
               dict(f_max=22050 / 2 + 1.0), dict(f_min=4000.0, f_max=4000.0), dict(f_min=5000.0, f_max=4000.0), dict(f_min=-1.0),
               dict(mode=3), dict(mode="whisper"), dict(mode=4), dict(mode=-1), dict(floor=0.0), dict(floor=-1e-10), dict(floor=float("nan")),
               dict(floor=1e-46), dict(floor=float("inf")), dict(mode="power", floor=0.0), dict(win_length=2049), dict(win_length=-1),
               dict(window=bad_window), dict(window=np.array([1.0, np.inf], dtype=np.float32)), dict(n_frames=-1), dict(scale=2), dict(norm=2)]
    for bad in refused:
        assert not api.mel_long_check(22050, **bad), bad
    assert not api.mel_long_check(0) and not api.mel_long_check(-1)
    sent = np.float32(-7.0)
    for args in ((22050, 1024, 80), (22050, 8192, 80), (22050, 2047, 80), (22050, 2048, 0), (22050, 2048, 257), (0, 2048, 80)):
        for f_min, f_max in ((0.0, 0.0),):
            buf = np.full(4096, sent, dtype=np.float32)
            assert lib.pdmp3_amd_mel_long_filterbank(args[0], args[1], args[2], f_min, f_max, 0, 1, buf.ctypes.data_as(C.c_void_p), buf.size) == -1
            assert lib.pdmp3_amd_mel_long_operand(args[0], args[1], args[2], f_min, f_max, 0, 1, buf.ctypes.data_as(C.c_void_p), buf.size, None, None) == -1
            assert (buf == sent).all()
    for f_min, f_max in ((0.0, 11026.0), (4000.0, 4000.0), (-1.0, 0.0)):
        buf = np.full(4096, sent, dtype=np.float32)
        assert lib.pdmp3_amd_mel_long_filterbank(22050, 2048, 80, f_min, f_max, 0, 1, buf.ctypes.data_as(C.c_void_p), buf.size) == -1
        assert lib.pdmp3_amd_mel_long_operand(22050, 2048, 80, f_min, f_max, 0, 1, buf.ctypes.data_as(C.c_void_p), buf.size, None, None) == -1
        assert (buf == sent).all()
    for n_fft, hop, n_mels in ((1024, 256, 80), (8192, 512, 80), (2048, 0, 80), (2048, 2049, 80), (4096, 4097, 80), (2048, 512, 0), (2048, 512, 257)):
        with pytest.raises(ValueError):
            api.mel_long_plan(n_fft, hop, n_mels)
        t, b = C.c_int(-5), C.c_uint(77)
        assert lib.pdmp3_amd_mel_long_plan(n_fft, hop, n_mels, C.byref(t), None, C.byref(b)) == -1 and t.value == -5 and b.value == 77
    # NULL pointers
    spec, keep = api._mel_long_spec()
    assert lib.pdmp3_amd_mel_long_check(None, 22050) == -1
    assert lib.pdmp3_amd_mel_long_filterbank(22050, 2048, 128, 0.0, 0.0, 0, 1, None, 0) == 128 * 1025
    rows, cols = C.c_int(0), C.c_int(0)
    assert lib.pdmp3_amd_mel_long_operand(22050, 2048, 17, 0.0, 0.0, 0, 1, None, 0, C.byref(rows), C.byref(cols)) == 1024 * 32
    assert (rows.value, cols.value) == (1024, 32)
    assert lib.pdmp3_amd_mel_long_plan(2048, 512, 128, None, None, None) == 0
    assert lib.pdmp3_amd_bulk_decode_clips_mel_long(None, None, 0, C.byref(spec), None) == -1
    # a cap below the whole: only that many floats are written
    for call, extra in ((lib.pdmp3_amd_mel_long_filterbank, ()), (lib.pdmp3_amd_mel_long_operand, (None, None))):
        buf = np.full(3000, sent, dtype=np.float32)
        assert call(22050, 2048, 128, 0.0, 0.0, 0, 1, buf.ctypes.data_as(C.c_void_p), 2100, *extra) > 3000
        assert (buf[2100:] == sent).all() and (buf[:2100] != sent).all()
    # section 10's calls keep refusing these lengths
    assert not api.mel_check(22050, n_fft=2048, hop=512) and not api.mel_check(44100, n_fft=4096, hop=1024)
    with pytest.raises(ValueError):
        api.mel_filterbank(22050, 2048, 128)
    with pytest.raises(ValueError):
        api.mel_tile(2048, 512, 128)


def test_the_plan_is_the_restated_one_exists_everywhere_and_keeps_the_kernels_preconditions():
    from pdmp3_amd import api
    lib = _emul()
    paths = {p: 0 for p in mlref.PATHS}
    for n_fft in mlref.SIZES:
        n2 = n_fft // 64
        big = 16 if n_fft == 2048 else 8
        edge = mlref.last_hop(n_fft, big)
        assert edge is not None and 1 < edge < n_fft and mlref.last_hop(n_fft, big // 2) == n_fft
        assert mlref.last_hop(4096, 16) is None                               # (N = 4096 never takes 16 frames)
        for n_mels in (1, 128, 256):
            for hop in range(1, n_fft + 1):                                   # existence and identity over all hops
                tile, pad, lds = api.mel_long_plan(n_fft, hop, n_mels)
                want = mlref.plan(n_fft, hop, n_mels)
                assert (tile, pad, lds) == want[:3], (n_fft, hop, n_mels)
                assert tile == (big if hop <= edge else big // 2)
                if hop in (1, 2, 441, 512, 1024, n_fft // 2 + 1, edge, edge + 1, n_fft - 1, n_fft):
                    assert pad == 0 and 64 * 1024 < lds <= mlref.LDS_MAX and want[3] == "N%d-tile%d" % (n_fft, tile)
                    assert lds == 4 * lib.emul_mel_long_lds_floats(tile, hop, n_fft)
                    first = lds // 4 - tile * n2 * 32 - tile * (8 * n2 + 2)
                    assert first % 4 == 0 and (tile - 1) * hop + n_fft <= first < (tile - 1) * hop + n_fft + 4
                    paths[want[3]] += 1
            assert api.mel_long_plan(n_fft, edge, n_mels)[0] == 2 * api.mel_long_plan(n_fft, edge + 1, n_mels)[0]
        print("N %d: %d frames up to hop %d, %d beyond" % (n_fft, big, edge, big // 2))
    assert all(paths.values()), paths
    # the thresholds lie below section 14's: the span keeps its region to itself
    import clip_stft_long_ref as lref
    for n_fft, big in ((2048, 16), (4096, 8)):
        edge = mlref.last_hop(n_fft, big)
        assert lref.plan(n_fft, edge + 1, 2)[0] == big
    assert api.mel_long_plan(2048, 512, 128)[0] == 16 and api.mel_long_plan(2048, 2048, 128)[0] == 8
    assert api.mel_long_plan(4096, 1024, 128)[0] == 8 and api.mel_long_plan(4096, 4096, 128)[0] == 4


EMUL_CASES = [
    # n_fft, hop, win_length, own window, channels, start, n_frames, J - start (None: all signal), sr, n_mels, scale, norm
    (2048, 512, 2048, False, 2, 0, 21, None, 22050, 128, "slaney", "slaney"),     # tile 16: a full tile and a partial one; stereo
    (2048, 441, 1764, True, 1, 57, 19, 6000, 22050, 17, "htk", None),             # a caller's window of 1764; valid = 14 ends inside a tile
    (2048, 2048, 2048, False, 1, 5000, 11, 9000, 44100, 256, "slaney", "slaney"),  # tile 8; valid = 5; two band tiles a wave
    (4096, 1024, 4096, False, 1, 300, 11, 7000, 48000, 128, "slaney", "slaney"),  # N2 = 64, tile 8; valid = 7
    (4096, 4096, 1920, True, 2, 100, 5, None, 48000, 1, "htk", "slaney"),         # tile 4; one band
    (2048, 1, 2048, False, 1, 3, 19, None, 32000, 17, "slaney", None),            # H = 1
    (4096, 3000, 4096, False, 1, 100000, 6, -7, 44100, 17, "slaney", "slaney"),   # wholly behind J: silent frames only
]
FLOORS = {1: 1e-6, 2: 1e-10}


def _emul_run(lib, api, n_fft, hop, nw, win, channels, start, F, rows_in, T, Ts, lead, sr, n_mels, scale, norm, mode, tile_lds=None):
    n2 = n_fft // 64
    tab = np.concatenate([t.ravel() for t in api.stft_long_tables(n_fft, nw, win, False)])
    op = api.mel_long_operand(sr, n_fft, n_mels, 0.0, 0.0, scale, norm)
    tile, _, lds_bytes = tile_lds or api.mel_long_plan(n_fft, hop, n_mels)
    per = n_mels * F
    out = np.full((channels, per + 8), np.float32(-3e9), dtype=np.float32)
    d = MelDesc(src=rows_in.ctypes.data, dst=out.ctypes.data, src_chan_stride=Ts, dst_chan_stride=per + 8, lead=lead)
    P = MelLongParams(n_in=T, n_fft=n_fft, n2=n2, hop=hop, n_mels=n_mels, mels16=(n_mels + 15) // 16 * 16, n_frames=F, tile=tile,
                      channels=channels, out_mode=mode, floor=FLOORS.get(mode, 1e-10),
                      span_floats=lds_bytes // 4 - tile * n2 * 32 - tile * (8 * n2 + 2), lds_bytes=lds_bytes)
    assert lib.emul_clip_mel_long(C.byref(d), 1, tab.ctypes.data, op.ctypes.data, C.byref(P)) == 0
    assert (out[:, per:] == np.float32(-3e9)).all() and (out[:, :per] != np.float32(-3e9)).all()
    return out[:, :per].reshape(channels, n_mels, F), tile


@pytest.mark.parametrize("case", EMUL_CASES, ids=lambda c: "N%d-H%d-Nw%d-C%d-s%d-M%d" % (c[0], c[1], c[2], c[4], c[5], c[9]))
def test_kernel_arithmetic_on_the_host_against_binary64(case):
    from pdmp3_amd import api
    lib = _emul()
    n_fft, hop, nw, own, channels, start, F, left, sr, n_mels, scale, norm = case
    rng = np.random.default_rng((n_fft * 131 + hop * 17 + start) & 0xffffffff)
    win = _window(nw, 3000 + nw) if own else None
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
    wt = sref.frame_window(n_fft, nw, win)
    signal = np.abs(sref.frames_of(y[0], s0, start, F, n_fft, hop) * wt[None, :]).sum(axis=1) > 0
    nv = sref.valid(start + left if left is not None else 2 ** 62, start, hop, F)
    w = mref.filterbank(sr, n_fft, n_mels, 0.0, 0.0, scale, norm)
    outs = {}
    for mode in range(3):
        wants = mlref.mel_all(y, s0, start, F, n_fft, hop, w, FLOORS.get(mode, 1e-10), nw, win, modes=(mode,))
        got32, tile = _emul_run(lib, api, n_fft, hop, nw, win, channels, start, F, rows, T, Ts, lead, sr, n_mels, scale, norm, mode)
        outs[mode] = got32
        want, bound = wants[mode]
        assert want.shape == got32.shape
        err = np.abs(got32.astype(np.float64) - want)
        assert (err <= bound).all(), (mode, float((err - bound).max()))
        nz = bound[:, :, signal] > 0
        ratio = float((err[:, :, signal][nz] / bound[:, :, signal][nz]).max()) if nz.any() else 0.0
        print("N %d H %d Nw %d C %d start %d bands %d mode %d tile %d (%s): worst error / bound %.4f (%d of %d frames hold signal, valid %d)"
              % (n_fft, hop, nw, channels, start, n_mels, mode, tile, mlref.plan(n_fft, hop, n_mels)[3], ratio, signal.sum(), F, nv))
        if signal.any():
            assert 0.0 < ratio <= 1.0
        if mode == 0:
            # silence: the bound is 0 there and the value exactly 0.0
            assert (bound[:, :, ~signal] == 0.0).all() and (got32[:, :, ~signal] == 0.0).all() and (got32 >= 0.0).all()
    # the logarithms are mode 0's values through the product's own floor and logf / log10f: the same M in all modes
    m0 = outs[0].astype(np.float64)
    assert (np.abs(outs[2] - np.log10(np.maximum(m0, float(np.float32(FLOORS[2]))))) <= mref.LOG_C * U * np.maximum(1.0, np.abs(outs[2]))).all()
    if left is not None:
        assert nv < F and not signal[nv + (n_fft // 2 + hop - 1) // hop:].any()


@pytest.mark.parametrize("n_fft,hop,n_mels", [(2048, 512, 128), (2048, 2048, 17), (4096, 1024, 17), (4096, 4096, 17)])
def test_a_frame_is_the_same_chains_wherever_it_lies_in_a_tile(n_fft, hop, n_mels):
    """frame f of a row is bit-equal to frame 0 of the row shifted by f H: both sides of the tile's edge"""
    from pdmp3_amd import api
    lib = _emul()
    tile = api.mel_long_plan(n_fft, hop, n_mels)[0]
    F = tile + 2
    T = (F - 1) * hop + n_fft
    Ts = (T + 3) // 4 * 4
    rng = np.random.default_rng(n_fft + hop)
    rows = np.zeros((1, Ts + 4), dtype=np.float32)
    rows[0, :T] = (rng.random(T, dtype=np.float32) * 2 - 1) * np.float32(0.7)
    whole, _ = _emul_run(lib, api, n_fft, hop, n_fft, None, 1, 0, F, rows, T, Ts, 0, 44100, n_mels, "slaney", "slaney", 0)
    assert whole.sum() > 0
    for f in (1, tile - 1, tile, tile + 1):
        sh = np.zeros((1, n_fft + 4), dtype=np.float32)
        sh[0, :n_fft] = rows[0, f * hop:f * hop + n_fft]
        one, _ = _emul_run(lib, api, n_fft, hop, n_fft, None, 1, 0, 1, sh, n_fft, n_fft, 0, 44100, n_mels, "slaney", "slaney", 0)
        assert np.array_equal(one[0, :, 0].view(np.uint32), whole[0, :, f].view(np.uint32)), f


def test_the_cases_cover_every_launch_path_silent_frames_and_a_valid_inside_a_tile():
    from pdmp3_amd import api
    inside, silent, paths, bands, stereo, own1764, hop1 = 0, 0, set(), set(), 0, 0, 0
    for n_fft, hop, nw, own, channels, start, F, left, sr, n_mels, scale, norm in EMUL_CASES:
        paths.add(mlref.plan(n_fft, hop, n_mels)[3])
        bands.add(n_mels)
        stereo += channels == 2
        own1764 += own and nw == 1764
        hop1 += hop == 1
        if left is None:
            continue
        nv = sref.valid(start + left, start, hop, F)
        tile = api.mel_long_plan(n_fft, hop, n_mels)[0]
        inside += 0 < nv < F and nv % tile != 0
        silent += nv + (n_fft // 2 + hop - 1) // hop < F
    assert paths == set(mlref.PATHS) and inside >= 3 and silent >= 3 and {1, 17, 256} <= bands and stereo and own1764 and hop1


def test_the_emulator_refuses_parameters_that_leave_the_lds():
    lib = _emul()
    d = MelDesc()
    z = np.zeros(1, dtype=np.float32)
    span = 15 * 512 + 2048
    ok = dict(n_in=0, n_fft=2048, n2=32, hop=512, n_mels=128, mels16=128, n_frames=0, tile=16, channels=1, out_mode=0, floor=1e-10,
              span_floats=span, lds_bytes=(span + 16 * 32 * 32 + 16 * 258) * 4)
    assert lib.emul_clip_mel_long(C.byref(d), 1, z.ctypes.data, z.ctypes.data, C.byref(MelLongParams(**ok))) == 0
    for bad in (dict(span_floats=span - 4), dict(lds_bytes=ok["lds_bytes"] - 4), dict(tile=4), dict(n2=64), dict(hop=513), dict(mels16=112),
                dict(n_mels=257, mels16=272), dict(lds_bytes=160 * 1024, span_floats=160 * 256 - 16 * 32 * 32 - 16 * 258)):
        assert lib.emul_clip_mel_long(C.byref(d), 1, z.ctypes.data, z.ctypes.data, C.byref(MelLongParams(**dict(ok, **bad)))) == -1, bad
