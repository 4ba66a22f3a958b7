"""Kaldi-style filterbank features of clips, the part that needs no GPU: the planning calls of
pdmp3_amd/host/clip_fbank.c against the step-by-step binary64 restatement tests/clip_fbank_ref.py, and k_clip_fbank's own
indexing and pointwise arithmetic (pdmp3_amd/csrc/mel_core.h and fbank_core.h, compiled here with g++ into
tests/host_emul/fbank_emul.cpp's loops) on random float32 rows against the definition, within the derived binary32 bound -- no
value left out.

torchaudio is not installed where these tests were written: nothing independent pins the restatement to Kaldi.  The last test
compares with torchaudio.compliance.kaldi.fbank where it is installed, and skips where it is not."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import clip_fbank_ref as ref
from clip_host import FbankDesc, build_emul

U = ref.U


class FbankParams(C.Structure):                    # include/pdmp3_hip.h pdmp3_fbank_params
    _fields_ = [("n_in", C.c_int64), ("win", C.c_int32), ("rows", C.c_int32), ("n_dft", C.c_int32), ("hop", C.c_int32), ("row_pad", C.c_int32),
                ("bins16", C.c_int32), ("n_mels", C.c_int32), ("mels16", C.c_int32), ("n_frames", C.c_int32), ("tile", C.c_int32),
                ("channels", C.c_int32), ("out_mode", C.c_int32), ("use_energy", C.c_int32), ("htk_compat", C.c_int32),
                ("subtract_mean", C.c_int32), ("remove_dc", C.c_int32), ("scale", C.c_float), ("eps", C.c_float),
                ("energy_log_floor", C.c_float), ("span_floats", C.c_uint32), ("lds_bytes", C.c_uint32)]


def _emul():
    lib = build_emul("fbank")
    lib.emul_clip_fbank.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    assert lib.emul_fbank_desc_bytes() == C.sizeof(FbankDesc) and lib.emul_fbank_params_bytes() == C.sizeof(FbankParams)
    return lib


FOLD_SHAPES = [(2, True), (2, False), (200, True), (200, False), (400, True), (400, False), (401, True), (1024, True), (1024, False)]


@pytest.mark.parametrize("nw,pow2", FOLD_SHAPES, ids=lambda v: str(v))
def test_the_folded_table_is_the_fold_rounded_once_and_the_fold_is_the_steps(nw, pow2):
    from pdmp3_amd import api
    n = ref.dft_length(nw, pow2)
    assert api.fbank_dft_length(nw, pow2) == n
    k2, kp, rows = n // 2, (n // 2 + 15) // 16 * 16, (nw + 3) // 4 * 4
    rng = np.random.default_rng(nw * 2 + pow2)
    y = rng.random((9, nw)) * 2 - 1
    y[0] = 0.25                                    # (a constant frame)
    y[1, : nw // 2] += 3.0                         # (a large offset in one half)
    worst_t = worst_f = 0.0
    for wt, rho, dc, scale in itertools.product(ref.WINDOWS, (0.0, 0.97, 1.0), (True, False), (1.0, 32768.0)):
        t = api.fbank_table(nw, pow2, dc, rho, wt, 0.42, scale)
        assert t.shape == (rows, 2 * kp) and t.dtype == np.float32
        win = ref.window(wt, nw)
        want = ref.folded(nw, n, rho, win, dc, scale)
        got = np.hstack([t[:nw, :k2], t[:nw, kp:kp + k2]]).astype(np.float64)
        # one rounding to binary32 of a binary64 value; the two binary64 evaluations (C's sequential sum of d, numpy's) may
        # differ by a few Nw 2^-53 of the largest entry: 2^-40 scale covers it
        tol = U * np.abs(want) + 2.0 ** -40 * scale
        err = np.abs(got - want)
        assert (err <= tol).all(), (wt, rho, dc, scale, float((err - tol).max()))
        worst_t = max(worst_t, float((err / tol).max()))
        pad = np.ones(t.shape, dtype=bool)
        pad[:nw, :k2] = False
        pad[:nw, kp:kp + k2] = False
        assert (t[pad] == 0.0).all()
        # the fold against the steps, in binary64, on random frames: relative 1e-12 of sum |T| |y| -- and, because the steps are
        # evaluated in binary64 themselves (the mean, the two subtractions, the window, a dot product of length Nw) on values
        # that do not cancel where the fold's coefficients do (Nw = N = 2 with DC removal: T = 0 exactly), that evaluation's own
        # rounding: (Nw + 8) 2^-53 of sum_n max|w| (1 + rho) (|s[n]| + |mean s|) <= 2 (1 + rho) max|w| scale sum |y|
        wp, _ = ref.frame_steps(scale * y, rho, win, dc)
        c, s = ref.dft_matrices(nw, n)
        steps = np.hstack([wp @ c, wp @ s])
        fold = y @ want
        own = (nw + 8) * 2.0 ** -53 * 2.0 * (1.0 + rho) * np.abs(win).max() * scale * np.abs(y).sum(axis=1, keepdims=True)
        lim = 1e-12 * (np.abs(y) @ np.abs(want)) + own
        assert (np.abs(fold - steps) <= lim).all(), (wt, rho, dc, scale)
        nz = lim > 0
        if nz.any():
            worst_f = max(worst_f, float((np.abs(fold - steps)[nz] / lim[nz]).max()))
    print("Nw %d N %d: worst table error / tolerance %.3f, worst |fold - steps| / (1e-12 sum |T| |y|) %.4f" % (nw, n, worst_t, worst_f))
    if (nw, pow2) == (400, True):
        t = api.fbank_table()
        assert 1.9 < float(np.abs(t).max()) < 2.0  # (the coefficients are no longer bounded by 1)


def test_filterbank_is_the_definition_in_binary64_rounded_once():
    from pdmp3_amd import api
    empty, worst, shapes = [], 0.0, 0
    for sr, n_mels, n in itertools.product((8000, 16000, 22050, 48000), (1, 23, 40, 80, 128, 256), (2, 256, 400, 512, 1024)):
        for lo, hi in ((20.0, 0.0), (0.0, sr / 2.0), (20.0, -400.0), (sr / 8.0, sr / 4.0), (100.0, -0.5)):
            w = api.fbank_filterbank(sr, n, n_mels, lo, hi)
            want = ref.filterbank(sr, n, n_mels, lo, hi)
            assert w.shape == want.shape == (n_mels, n // 2) and w.dtype == np.float32
            assert (w >= 0.0).all() and np.isfinite(w).all() and (w <= 1.0).all()
            # one rounding; the binary64 values themselves may differ in their last bits where the two libraries' log does,
            # amplified by mel / d < 2^12 here: 2^-38 absolute
            tol = U * np.abs(want) + 2.0 ** -38
            err = np.abs(w.astype(np.float64) - want)
            assert (err <= tol).all(), (sr, n_mels, n, lo, hi, float((err - tol).max()))
            worst = max(worst, float((err / tol).max()))
            shapes += 1
            rows = np.flatnonzero((w == 0.0).all(axis=1))
            assert np.array_equal(rows, np.flatnonzero((want == 0.0).all(axis=1)))
            if rows.size:
                empty.append((sr, n_mels, n, lo, hi, rows.size))
    print("filterbank: worst error / tolerance %.3f over %d shapes; %d with all-zero rows, e.g. %s" % (worst, shapes, len(empty), empty[:4]))
    assert any(e[1] == 256 and e[2] == 256 for e in empty)
    assert not any(e[0] == 16000 and e[1] in (23, 80) and e[2] == 512 and e[3] == 20.0 and e[4] == 0.0 for e in empty)
    # the Nyquist bin is not there, and a negative high_freq is an offset from it
    assert np.array_equal(api.fbank_filterbank(16000, 512, 40, 20.0, -400.0), api.fbank_filterbank(16000, 512, 40, 20.0, 7600.0))


def test_valid_against_brute_force_around_both_ends():
    from pdmp3_amd import api
    for nw, hop in ((2, 1), (2, 2), (200, 80), (400, 160), (400, 400), (1024, 480), (1024, 1)):
        J = 5 * nw + 3
        for start in [0, 1, hop - 1, hop, nw, J - 2 * nw - 1, J - nw - hop - 1, J - nw - hop, J - nw - 1, J - nw, J - nw + 1, J - 1, J, J + 5, 2 ** 40]:
            if start < 0:
                continue
            for F in (0, 1, 2, 3, 33):
                brute = 0
                for f in range(F):                 # (frames wholly inside [0, J): they are a prefix)
                    if start + f * hop + nw <= J:
                        assert brute == f
                        brute += 1
                assert api.fbank_valid(J, start, nw, hop, F) == brute == ref.valid(J, start, nw, hop, F), (nw, hop, start, F)
    assert api.fbank_valid(0, 0, 400, 160, 5) == 0
    for bad in ((-1, 0, 400, 160, 1), (10, -1, 400, 160, 1), (10, 0, 0, 160, 1), (10, 0, 400, 0, 1), (10, 0, 400, 160, -1)):
        with pytest.raises(ValueError):
            api.fbank_valid(*bad)



def tile_sweep():
    """(Nw, N, hop, n_mels) of the grid the plan's preconditions are walked over (tests/test_clip_forms_host.py walks it too)"""
    for nw, pow2 in ((2, True), (16, False), (200, True), (398, False), (400, True), (400, False), (401, True), (513, True), (1024, True)):
        n = ref.dft_length(nw, pow2)
        for hop in sorted(set([1, 2, 3, 4, 5, 31, 32, 33, 64, 80, 128, 160, 450, 480, nw // 2, nw - 1, nw]) & set(range(1, nw + 1))):
            for n_mels in (1, 23, 80, 256):
                yield nw, n, hop, n_mels


def test_the_tile_keeps_the_kernels_preconditions():
    """every (Nw, N, H, n_mels): the span in its padded chunks, the mel tile over it and the powers (with a spare float a row for
    the energy) behind it fit the LDS the product asks for -- 64 KB, or the static variant's array at a tile of 16 --, 32 frames
    wherever they fit 64 KB, and hop + row_pad = 2 mod 32"""
    from pdmp3_amd import api
    tiles = {16: 0, 32: 0}
    static = 0
    for nw, n, hop, n_mels in tile_sweep():
        tile, pad, lds = api.fbank_tile(nw, n, hop, n_mels)
        kp, mp, rows = (n // 2 + 15) // 16 * 16, (n_mels + 15) // 16 * 16, (nw + 3) // 4 * 4
        assert tile in (16, 32) and 0 <= pad < 32 and (hop + pad) % 32 == 2 and lds <= 160 * 1024 - 64
        first = lds // 4 - tile * (kp + 2)
        sp = (tile - 1) * hop + rows
        assert first >= -(-sp // hop) * (hop + pad) and first >= mp * (tile + 1)
        if tile == 16:
            assert (max(-(-(31 * hop + rows) // hop) * (hop + pad), mp * 33) + 32 * (kp + 2)) * 4 > 64 * 1024
            static += lds > 64 * 1024
        else:
            assert lds <= 64 * 1024
        tiles[tile] += 1
    assert tiles[16] and tiles[32] and static
    assert api.fbank_tile(400, 512, 160, 80) == (32, 2, 55056)
    t, _, lds = api.fbank_tile(1024, 1024, 480, 80)
    assert t == 16 and lds > 64 * 1024             # (the static-array kernel)


def test_refusals_of_the_planning_calls():
    from pdmp3_amd import api
    assert api.fbank_check(16000)
    assert api.fbank_check(8000, win_length=2, hop=1, num_mel_bins=1) and api.fbank_check(48000, win_length=1024, hop=1024, num_mel_bins=256, high_freq=24000.0)
    assert api.fbank_check(16000, win_length=401) and api.fbank_check(16000, preemphasis_coefficient=0.0) and api.fbank_check(16000, preemphasis_coefficient=1.0)
    assert api.fbank_check(16000, vtln_warp=1.0) and api.fbank_check(16000, energy_floor=0.0, use_energy=True, htk_compat=True, subtract_mean=True)
    for wt in ref.WINDOWS:
        assert api.fbank_check(16000, window_type=wt)
    for bad in (dict(win_length=1), dict(win_length=1025), dict(win_length=401, round_to_power_of_two=False), dict(hop=0), dict(hop=401),
                dict(frame_shift=26.0), dict(num_mel_bins=0), dict(num_mel_bins=257), dict(preemphasis_coefficient=-0.1),
                dict(preemphasis_coefficient=1.01), dict(preemphasis_coefficient=float("nan")), dict(window_type="kaiser"), dict(window_type=5),
                dict(blackman_coeff=float("inf")), dict(low_freq=-1.0), dict(high_freq=8000.5), dict(low_freq=4000.0, high_freq=4000.0),
                dict(low_freq=7900.0, high_freq=-200.0), dict(high_freq=-8000.0), dict(use_log_fbank=2), dict(energy_floor=-1.0),
                dict(energy_floor=float("inf")), dict(scale=0.0), dict(scale=-1.0), dict(scale=float("inf")), dict(scale=float("nan")),
                dict(scale=1e-46), dict(scale=1e38), dict(n_frames=-1),
                # what is not offered
                dict(dither=1.0), dict(dither=1e-9), dict(use_power=False), dict(raw_energy=False), dict(snip_edges=False), dict(vtln_warp=1.1),
                dict(vtln_warp=0.9)):
        assert not api.fbank_check(16000, **bad), bad
    assert not api.fbank_check(0) and not api.fbank_check(-16000, win_length=400, hop=160)
    for nw, pow2 in ((1, True), (1025, True), (401, False), (0, True)):
        with pytest.raises(ValueError):
            api.fbank_dft_length(nw, pow2)
        with pytest.raises(ValueError):
            api.fbank_table(nw, pow2)
    for kw in (dict(preemphasis_coefficient=1.5), dict(window_type="kaiser"), dict(scale=0.0), dict(scale=float("nan")), dict(blackman_coeff=float("nan"))):
        with pytest.raises(ValueError):
            api.fbank_table(400, **kw)
    for args in ((16000, 401, 23), (16000, 0, 23), (16000, 1026, 23), (16000, 512, 0), (16000, 512, 257), (0, 512, 23), (16000, 512, 23, -1.0),
                 (16000, 512, 23, 20.0, 8000.5), (16000, 512, 23, 5000.0, 4000.0), (16000, 512, 23, 20.0, -8000.0)):
        with pytest.raises(ValueError):
            api.fbank_filterbank(*args)
    for args in ((1, 2, 1, 23), (400, 512, 0, 23), (400, 512, 401, 23), (400, 256, 160, 23), (400, 600, 160, 23), (400, 512, 160, 0),
                 (400, 512, 160, 257), (1025, 2048, 160, 23), (401, 401, 160, 23)):
        with pytest.raises(ValueError):
            api.fbank_tile(*args)


EMUL_CASES = [
    # Nw, H, power of two, n_mels, sr, channels, start, n_frames, J - start (None: the row is all signal), options
    (400, 160, True, 80, 16000, 1, 0, 35, None, {}),
    (400, 160, True, 80, 16000, 2, 5000, 40, 3000, {}),                                  # frames across and behind J
    (400, 160, True, 23, 16000, 2, 100000, 31, -7, {}),                                  # wholly behind J
    (200, 80, True, 23, 8000, 1, 77, 34, 2500, dict(scale=32768.0)),
    (400, 160, False, 40, 16000, 1, 3, 33, None, dict(window_type="hamming", rho=0.0)),  # N = Nw
    (400, 200, True, 40, 16000, 2, 3, 17, 2000, dict(window_type="hanning", remove_dc=False)),
    (401, 3, True, 20, 16000, 1, 50, 36, 300, dict(window_type="rectangular", rho=1.0)),  # Nw odd, a hop below 4
    (1024, 480, True, 80, 48000, 2, 300, 18, 6000, dict(window_type="blackman")),        # tile of 16, more than 64 KB
    (1024, 1024, False, 256, 44100, 1, 0, 17, None, {}),
    (18, 1, True, 5, 8000, 2, 2, 70, 40, dict(window_type="hamming", low=0.0)),             # H = 1
    (16, 16, False, 5, 8000, 1, 0, 33, 400, dict(window_type="hamming")),
]


def edge_options(e):
    """decode_clips_fbank's argument names of an entry of EDGES -> the options of a case"""
    names = dict(window_type="window_type", preemphasis_coefficient="rho", low_freq="low", remove_dc_offset="remove_dc", scale="scale")
    return {names[k]: v for k, v in e.items() if k in names}


def _edge_case(e):
    """an entry of clip_fbank_ref.EDGES as a case: one full tile and a partial one, the row all signal; the own rate: 44.1 kHz"""
    pow2 = e.get("round_to_power_of_two", True)
    tile = ref.form(e["win_length"], ref.dft_length(e["win_length"], pow2), e["hop"], e["num_mel_bins"])[0]
    return (e["win_length"], e["hop"], pow2, e["num_mel_bins"], e["sample_rate"] or 44100, e["channels"], 57, tile + 3, None, edge_options(e))


EMUL_CASES += [_edge_case(e) for e in ref.EDGES.values()]


def _run_emul(lib, y_rows, Ts, T, channels, F, nv, nw, hop, pow2, n_mels, sr, o, mode, energy, sub):
    from pdmp3_amd import api
    n = ref.dft_length(nw, pow2)
    tile, row_pad, lds_bytes = api.fbank_tile(nw, n, hop, n_mels)
    k2 = n // 2
    kp, mp = (k2 + 15) // 16 * 16, (n_mels + 15) // 16 * 16
    dft = api.fbank_table(nw, pow2, o.get("remove_dc", True), o.get("rho", 0.97), o.get("window_type", "povey"), 0.42, o.get("scale", 1.0))
    w32 = api.fbank_filterbank(sr, n, n_mels, o.get("low", 20.0), 0.0)
    fbt = np.zeros((kp, mp), dtype=np.float32)
    fbt[:k2, :n_mels] = w32.T
    use_e, htk, floor = energy
    D = n_mels + use_e
    out = np.full((channels, F * D + 8), np.float32(-3e9), dtype=np.float32)
    d = FbankDesc(src=y_rows.ctypes.data, dst=out.ctypes.data, src_chan_stride=Ts, dst_chan_stride=F * D + 8, valid=nv)
    P = FbankParams(n_in=T, win=nw, rows=(nw + 3) // 4 * 4, n_dft=n, hop=hop, row_pad=row_pad, bins16=kp, n_mels=n_mels, mels16=mp, n_frames=F,
                    tile=tile, channels=channels, out_mode=mode, use_energy=use_e, htk_compat=htk, subtract_mean=int(sub),
                    remove_dc=int(o.get("remove_dc", True)), scale=o.get("scale", 1.0), eps=2.0 ** -23,
                    energy_log_floor=math.log(floor) if floor > 0 else -math.inf, span_floats=lds_bytes // 4 - tile * (kp + 2), lds_bytes=lds_bytes)
    assert lib.emul_clip_fbank(C.byref(d), 1, dft.ctypes.data, fbt.ctypes.data, C.byref(P)) == 0
    assert (out[:, F * D:] == np.float32(-3e9)).all()
    return out[:, :F * D].reshape(channels, F, D).astype(np.float64), tile


ENERGIES = [(0, 0, 0.0), (1, 0, 0.0), (1, 1, 100.0)]


@pytest.mark.parametrize("case", EMUL_CASES, ids=lambda c: "Nw%d-H%d-%s-m%d-C%d-s%d" % (c[0], c[1], "p2" if c[2] else "eq", c[3], c[5], c[6]))
def test_kernel_arithmetic_on_the_host_against_binary64(case):
    lib = _emul()
    nw, hop, pow2, n_mels, sr, channels, start, F, left, o = case
    n = ref.dft_length(nw, pow2)
    rng = np.random.default_rng((nw * 131 + hop * 7 + start) & 0xffffffff)
    T = (F - 1) * hop + nw
    Ts = (T + 3) // 4 * 4
    stage = np.full(channels * Ts + 16, np.float32(7e8), dtype=np.float32)        # (guards: nothing outside [0, T) may be read)
    rows = stage[8:8 + channels * Ts].reshape(channels, Ts)
    rows[:, :T] = (rng.random((channels, T), dtype=np.float32) * 2 - 1) * np.float32(0.7) + np.float32(0.05)
    if left is not None:
        rows[:, max(0, left):T] = 0.0
    y = rows[:, :T].copy()
    nv = ref.valid(start + left if left is not None else 2 ** 62, start, nw, hop, F)
    w64 = ref.filterbank(sr, n, n_mels, o.get("low", 20.0), 0.0)
    signal = np.abs(ref.frames_of(y[0], start, start, F, nw, hop)).sum(axis=1) > 0
    for mode, energy, sub in itertools.product((0, 1), ENERGIES, (False, True)):
        got, tile = _run_emul(lib, rows, Ts, T, channels, F, nv, nw, hop, pow2, n_mels, sr, o, mode, energy, sub)
        want, bound = ref.fbank(y, start, start, F, nw, hop, w64, nv, pow2, o.get("remove_dc", True), o.get("rho", 0.97),
                                o.get("window_type", "povey"), 0.42, mode, bool(energy[0]), bool(energy[1]), energy[2], sub, o.get("scale", 1.0))
        err = np.abs(got - want)
        assert (err <= bound).all(), (mode, energy, sub, float((err - bound).max()), np.unravel_index(np.argmax(err - bound), err.shape))
        ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
        print("Nw %d N %d H %d mels %d C %d start %d mode %d energy %s mean %d tile %d: worst error / bound %.4f (%d of %d frames hold signal, valid %d)"
              % (nw, n, hop, n_mels, channels, start, mode, energy, sub, tile, ratio, signal.sum(), F, nv))
        if signal.any():
            assert 0.0 < ratio <= 1.0
        if not sub:
            sil = ~signal
            mel_cols = slice(1, None) if (energy[0] and not energy[1]) else slice(0, n_mels)
            if mode == 0:
                # silence: the bound is 0 there and the value exactly 0.0
                assert (bound[:, sil] == 0.0).all() and (got[:, sil] == 0.0).all()
            else:
                assert np.allclose(want[:, sil][:, :, mel_cols], math.log(ref.EPS), rtol=1e-15, atol=0)
        if sub and nv == 0:
            # nothing is subtracted: the same as without
            plain, _ = _run_emul(lib, rows, Ts, T, channels, F, nv, nw, hop, pow2, n_mels, sr, o, mode, energy, False)
            assert np.array_equal(got, plain)


def test_a_constant_signal_with_dc_removal_gives_the_floor():
    """every sample of every frame the same: DC removal leaves nothing, every mel column is ln eps in the definition, and the
    binary32 evaluation stays within the bound (which is loose here: the cancellation is the table's, not the bound's)"""
    lib = _emul()
    nw, hop, n_mels, sr, F = 400, 160, 80, 16000, 34
    T = (F - 1) * hop + nw
    Ts = (T + 3) // 4 * 4
    rows = np.full((1, Ts), np.float32(0.37), dtype=np.float32)
    w64 = ref.filterbank(sr, 512, n_mels)
    for scale in (1.0, 32768.0):
        o = dict(scale=scale)
        got, _ = _run_emul(lib, rows, Ts, T, 1, F, F, nw, hop, True, n_mels, sr, o, 1, (1, 0, 0.0), False)
        want, bound = ref.fbank(rows[:, :T], 0, 0, F, nw, hop, w64, F, mode=1, use_energy=True, scale=scale)
        assert np.allclose(want[:, :, 1:], math.log(ref.EPS), rtol=1e-12, atol=0)
        err = np.abs(got - want)
        assert (err <= bound).all(), float((err - bound).max())
        print("constant 0.37, scale %g: mel columns %.4f .. %.4f (ln eps = %.4f), worst error / bound %.3g, energy column %.4f .. %.4f"
              % (scale, got[:, :, 1:].min(), got[:, :, 1:].max(), math.log(ref.EPS), float((err / bound).max()), got[:, :, 0].min(), got[:, :, 0].max()))


def test_against_torchaudio_where_it_is_installed():
    """float64 input, M well above the floor only: torchaudio's eps follows the dtype"""
    pytest.importorskip("torchaudio")
    import torch
    import torchaudio
    rng = np.random.default_rng(5)
    y = (rng.random(16000) * 2 - 1) * 0.5
    for kw in (dict(), dict(use_energy=True), dict(window_type="hamming", preemphasis_coefficient=0.0), dict(remove_dc_offset=False, htk_compat=True, use_energy=True),
               dict(num_mel_bins=80, round_to_power_of_two=False)):
        want = torchaudio.compliance.kaldi.fbank(torch.from_numpy(y)[None], dither=0.0, energy_floor=0.0, **kw).numpy()
        nw, hop, n_mels = 400, 160, kw.get("num_mel_bins", 23)
        n = ref.dft_length(nw, kw.get("round_to_power_of_two", True))
        F = want.shape[0]
        got, _ = ref.fbank(y[None], 0, 0, F, nw, hop, ref.filterbank(16000, n, n_mels), F, kw.get("round_to_power_of_two", True),
                           kw.get("remove_dc_offset", True), kw.get("preemphasis_coefficient", 0.97), kw.get("window_type", "povey"), 0.42, 1,
                           kw.get("use_energy", False), kw.get("htk_compat", False))
        big = want > math.log(1e-6)
        assert np.allclose(got[0][big], want[big], rtol=0, atol=1e-9), kw
