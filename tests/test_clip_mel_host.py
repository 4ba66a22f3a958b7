"""Log-mel features of clips, the part that needs no GPU: the planning calls of
pdmp3_amd/host/clip_mel.c against the binary64 restatement tests/clip_mel_ref.py, and k_clip_mel's own indexing and pointwise
arithmetic (pdmp3_amd/csrc/mel_core.h, compiled here with g++ into tests/host_emul/mel_emul.cpp's loops) on random float32
rows against the definition, within the derived binary32 bound -- no value left out."""
import ctypes as C
import itertools

import numpy as np
import pytest

import clip_mel_ref as ref
from clip_host import MelDesc, build_emul

U = ref.U


class MelParams(C.Structure):                      # include/pdmp3_hip.h pdmp3_mel_params
    _fields_ = [("n_in", C.c_int64), ("n_fft", C.c_int32), ("rows", C.c_int32), ("hop", C.c_int32), ("row_pad", C.c_int32),
                ("bins16", C.c_int32), ("n_mels", C.c_int32), ("mels16", C.c_int32), ("n_frames", C.c_int32), ("tile", C.c_int32),
                ("channels", C.c_int32), ("out_mode", C.c_int32), ("floor", C.c_float), ("span_floats", C.c_uint32), ("lds_bytes", C.c_uint32)]


def _emul():
    lib = build_emul("mel")
    lib.emul_clip_mel.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    assert lib.emul_mel_desc_bytes() == C.sizeof(MelDesc) and lib.emul_mel_params_bytes() == C.sizeof(MelParams)
    return lib


@pytest.mark.parametrize("n_fft", [16, 400, 512, 1024])
def test_dft_table_is_the_definition_in_binary64_rounded_once(n_fft):
    from pdmp3_amd import api
    t = api.mel_dft_table(n_fft)
    want = ref.dft_table(n_fft)
    assert t.shape == want.shape and t.dtype == np.float32
    K = n_fft // 2 + 1
    Kp = want.shape[1] // 2
    # one rounding to binary32 of a binary64 value whose own error is a few 2^-53 (|value| <= 1)
    err = np.abs(t.astype(np.float64) - want)
    assert (err <= U * np.abs(want) + 2.0 ** -50).all(), err.max()
    pad = np.ones(want.shape, dtype=bool)
    pad[:n_fft, :K] = False
    pad[:n_fft, Kp:Kp + K] = False
    assert (t[pad] == 0.0).all() and pad.sum() > 0
    assert (t[0] == 0.0).all()                     # (w[0] = 0: the periodic window)
    print("n_fft %d: table %s, worst |table - binary64| / (u |value|) = %.3f" % (n_fft, t.shape, (err / np.maximum(U * np.abs(want), 1e-300))[np.abs(want) > 1e-6].max()))


FB_CASES = [(n_fft, sr, n_mels) for n_fft in (16, 400, 512, 1024) for sr in (8000, 16000, 22050, 44100, 48000) for n_mels in (1, 40, 80, 128, 256)]


def test_filterbank_is_the_definition_in_binary64_rounded_once():
    from pdmp3_amd import api
    empty = []
    worst = 0.0
    for (n_fft, sr, n_mels), scale, norm in itertools.product(FB_CASES, ("slaney", "htk"), ("slaney", None)):
        for f_min, f_max in ((0.0, 0.0), (0.0, sr / 2.0), (20.0, sr / 2.0 - 100.0), (sr / 8.0, sr / 4.0)):
            w = api.mel_filterbank(sr, n_fft, n_mels, f_min, f_max, scale, norm)
            want = ref.filterbank(sr, n_fft, n_mels, f_min, f_max, scale, norm)
            assert w.shape == want.shape == (n_mels, n_fft // 2 + 1) and w.dtype == np.float32
            assert (w >= 0.0).all() and np.isfinite(w).all()
            # one rounding; the binary64 values themselves may differ in their last bits where the two libraries' log / exp
            # do, amplified by f / (f_(m+1) - f_m) < 2^20 here: 2^-32 of a row's largest weight
            tol = U * np.abs(want) + 2.0 ** -32 * want.max(axis=1, keepdims=True)
            err = np.abs(w.astype(np.float64) - want)
            assert (err <= tol).all(), (n_fft, sr, n_mels, scale, norm, f_min, f_max, (err - tol).max())
            worst = max(worst, float((err / np.maximum(tol, 1e-300)).max()))
            rows = np.flatnonzero((w == 0.0).all(axis=1))
            assert np.array_equal(rows, np.flatnonzero((want == 0.0).all(axis=1)))
            if rows.size:
                empty.append((n_fft, sr, n_mels, scale, f_min, f_max, rows.size))
    print("filterbank: worst error / tolerance %.3f over %d shapes" % (worst, len(FB_CASES) * 16))
    # rows without a bin inside their band: all zero, and said so
    print("filterbanks with all-zero rows (no bin inside the band): %d, e.g. %s" % (len(empty), empty[:6]))
    assert any(e[0] == 16 and e[2] == 256 for e in empty)
    assert not any(e[0] == 400 and e[1] == 16000 and e[2] == 80 and e[4] == 0.0 and e[5] in (0.0, 8000.0) for e in empty)


def test_span_against_brute_force_around_both_ends():
    from pdmp3_amd import api
    for n_fft, hop in ((16, 1), (16, 16), (400, 160), (512, 128), (1024, 1024), (1024, 1)):
        w = ref.window(n_fft)
        J = 5 * n_fft + 3
        for start in list(range(0, n_fft + 2, max(1, n_fft // 7))) + [J - n_fft, J - n_fft // 2, J - 1, J, J + 5, 2 ** 40]:
            for F in (0, 1, 2, 3, 33):
                first, count = api.mel_span(n_fft, hop, start, F)
                assert (first, count) == ref.span(n_fft, hop, start, F)
                # brute force over the definition: every position some frame reads
                pos = set()
                for f in range(F):
                    for n in range(n_fft):
                        pos.add(start + f * hop - n_fft // 2 + n)
                if F:
                    assert min(pos) == first and max(pos) == first + count - 1
                    # (w[0] = 0, so the first position has weight 0: one sample more than is needed, never one less)
                    assert w[0] == 0.0
                else:
                    assert count == 0
                assert ref.valid(J, start, hop, F) == sum(1 for f in range(F) if start + f * hop < J)


EMUL_CASES = [
    # n_fft, hop, n_mels, sr, scale, norm, channels, start, n_frames, J - start (None: the row is all signal)
    (400, 160, 80, 16000, "slaney", "slaney", 1, 0, 35, None),            # leading zeros: N / 2 of them
    (400, 160, 80, 16000, "slaney", "slaney", 2, 57, 33, None),           # start inside the first N / 2 samples
    (400, 160, 80, 16000, "slaney", "slaney", 1, 5000, 40, 3000),         # frames across and behind J
    (400, 160, 80, 16000, "slaney", "slaney", 2, 100000, 31, -7),         # wholly behind J
    (512, 128, 128, 24000, "htk", None, 2, 1000, 34, 4000),
    (1024, 1024, 40, 44100, "slaney", "slaney", 1, 300, 18, 9000),        # H = N: tile of 16
    (1024, 1, 40, 44100, "slaney", "slaney", 1, 3, 37, None),             # H = 1
    (16, 1, 5, 8000, "htk", "slaney", 2, 2, 70, 40),
    (16, 16, 9, 8000, "slaney", None, 1, 0, 33, 400),
    (400, 400, 80, 16000, "slaney", "slaney", 1, 123, 17, None),
    (398, 3, 20, 16000, "htk", None, 1, 50, 36, None),                    # N not a multiple of 4, a hop below 4
]


def _edge_case(e):
    """an entry of clip_mel_ref.EDGES as a case: one full tile and a partial one, the row all signal; the own rate: 44.1 kHz"""
    tile = ref.form(e["n_fft"], e["hop"], e["n_mels"])[0]
    return (e["n_fft"], e["hop"], e["n_mels"], e["sample_rate"] or 44100, e["scale"], e["norm"], e["channels"], 57, tile + 3, None)


EMUL_CASES += [_edge_case(e) for e in ref.EDGES.values()]


@pytest.mark.parametrize("case", EMUL_CASES, ids=lambda c: "N%d-H%d-m%d-C%d-s%d" % (c[0], c[1], c[2], c[6], c[7]))
def test_kernel_arithmetic_on_the_host_against_binary64(case):
    from pdmp3_amd import api
    lib = _emul()
    n_fft, hop, n_mels, sr, scale, norm, channels, start, F, left = case
    rng = np.random.default_rng(hash(case[:4] + (start,)) & 0xffffffff)
    tile, row_pad, lds_bytes = api.mel_tile(n_fft, hop, n_mels)
    K = n_fft // 2 + 1
    Kp, Mp = (K + 15) // 16 * 16, (n_mels + 15) // 16 * 16
    dft = api.mel_dft_table(n_fft)
    w32 = api.mel_filterbank(sr, n_fft, n_mels, 0.0, 0.0, scale, norm)
    fbt = np.zeros((Kp, Mp), dtype=np.float32)
    fbt[:K, :n_mels] = w32.T
    w64 = ref.filterbank(sr, n_fft, n_mels, 0.0, 0.0, scale, norm)
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
    for mode in (0, 1, 2, 3):
        floor = 1e-10 if mode != 1 else 1e-6
        out = np.full((channels, n_mels * F + 8), np.float32(-3e9), dtype=np.float32)
        d = MelDesc(src=rows.ctypes.data, dst=out.ctypes.data, src_chan_stride=Ts, dst_chan_stride=n_mels * F + 8, lead=lead)
        P = MelParams(n_in=T, n_fft=n_fft, rows=(n_fft + 3) // 4 * 4, hop=hop, row_pad=row_pad, bins16=Kp, n_mels=n_mels, mels16=Mp, n_frames=F,
                      tile=tile, channels=channels, out_mode=mode, floor=floor, span_floats=lds_bytes // 4 - tile * (Kp + 2), lds_bytes=lds_bytes)
        assert lib.emul_clip_mel(C.byref(d), 1, dft.ctypes.data, fbt.ctypes.data, C.byref(P)) == 0
        assert (out[:, n_mels * F:] == np.float32(-3e9)).all()
        got = out[:, :n_mels * F].reshape(channels, n_mels, F).astype(np.float64)
        want, bound = ref.mel(y, s0, start, F, n_fft, hop, w64, mode, floor)
        err = np.abs(got - want)
        assert (err <= bound).all(), (mode, float((err - bound).max()))
        signal = np.abs(ref.frames_of(y[0], s0, start, F, n_fft, hop) * ref.window(n_fft)).sum(axis=1) > 0
        ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
        print("N %d H %d mels %d C %d start %d mode %d tile %d: worst error / bound %.4f (%d of %d frames hold signal)"
              % (n_fft, hop, n_mels, channels, start, mode, tile, ratio, signal.sum(), F))
        if signal.any():
            assert 0.0 < ratio <= 1.0
        if mode == 0:
            # silence: the bound is 0 there and the value exactly 0.0
            assert (bound[:, :, ~signal] == 0.0).all() and (got[:, :, ~signal] == 0.0).all()
            nv = ref.valid(start + left if left is not None else 2 ** 62, start, hop, F)
            assert not signal[nv + (n_fft // 2 + hop - 1) // hop:].any()


def test_refusals_of_the_planning_calls():
    from pdmp3_amd import api
    assert api.mel_check(16000)
    assert api.mel_check(16000, n_fft=16, hop=16, n_mels=1) and api.mel_check(48000, n_fft=1024, hop=1, n_mels=256, f_max=24000.0)
    for bad in (dict(n_fft=401), dict(n_fft=14), dict(n_fft=1026), dict(hop=0), dict(hop=401), dict(f_max=8000.5), dict(floor=0.0),
                dict(floor=-1e-10), dict(n_mels=0), dict(n_mels=257), dict(f_min=-1.0), dict(f_min=4000.0, f_max=4000.0), dict(n_frames=-1),
                dict(mode=4), dict(scale=2), dict(norm=2), dict(floor=float("nan")), dict(floor=1e-46)):
        assert not api.mel_check(16000, **bad), bad
    for n_fft in (401, 14, 1026, 0, -2):
        with pytest.raises(ValueError):
            api.mel_dft_table(n_fft)
        with pytest.raises(ValueError):
            api.mel_span(n_fft, 1, 0, 1)
        with pytest.raises(ValueError):
            api.mel_filterbank(16000, n_fft, 80)
    for hop in (0, -1, 401):
        with pytest.raises(ValueError):
            api.mel_span(400, hop, 0, 1)
        with pytest.raises(ValueError):
            api.mel_tile(400, hop, 80)
    with pytest.raises(ValueError):
        api.mel_span(400, 160, -1, 1)
    with pytest.raises(ValueError):
        api.mel_filterbank(16000, 400, 80, 0.0, 8000.5)
    with pytest.raises(ValueError):
        api.mel_filterbank(16000, 400, 80, 5000.0, 4000.0)


def tile_sweep():
    """(n_fft, hop, n_mels) of the grid the plan's preconditions are walked over (tests/test_clip_forms_host.py walks it too)"""
    for n_fft in (16, 18, 398, 400, 512, 1022, 1024):
        for hop in sorted(set([1, 2, 3, 4, 5, 31, 32, 33, 64, 128, 160, n_fft // 2, n_fft - 1, n_fft]) & set(range(1, n_fft + 1))):
            for n_mels in (1, 80, 256):
                yield n_fft, hop, n_mels


def test_the_tile_keeps_the_kernels_preconditions():
    """every (N, H): the span in its padded chunks, the mel tile over it and the powers behind it fit the LDS the product asks
    for, at most 160 KB, 32 frames wherever they fit 64 KB, and hop + row_pad = 2 mod 32"""
    from pdmp3_amd import api
    tiles = {16: 0, 32: 0}
    for n_fft, hop, n_mels in tile_sweep():
        tile, pad, lds = api.mel_tile(n_fft, hop, n_mels)
        Kp, Mp, rows = (n_fft // 2 + 1 + 15) // 16 * 16, (n_mels + 15) // 16 * 16, (n_fft + 3) // 4 * 4
        assert tile in (16, 32) and 0 <= pad < 32 and (hop + pad) % 32 == 2 and lds <= 160 * 1024
        first = lds // 4 - tile * (Kp + 2)
        sp = (tile - 1) * hop + rows
        assert first >= -(-sp // hop) * (hop + pad) and first >= Mp * (tile + 1)
        if tile == 16:
            assert (max(-(-(31 * hop + rows) // hop) * (hop + pad), Mp * 33) + 32 * (Kp + 2)) * 4 > 64 * 1024
        else:
            assert lds <= 64 * 1024
        tiles[tile] += 1
    assert tiles[16] and tiles[32]
    assert api.mel_tile(400, 160, 80)[0] == 32
