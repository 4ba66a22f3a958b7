"""Kaldi-style MFCC features of clips, the part that needs no GPU: the planning calls of
pdmp3_amd/host/clip_mfcc.c against the step-by-step binary64 restatement tests/clip_mfcc_ref.py, and k_clip_mfcc's own indexing
and pointwise arithmetic (pdmp3_amd/csrc/mel_core.h, fbank_core.h and mfcc_core.h, compiled here with g++ into
tests/host_emul/mfcc_emul.cpp's loops) on random float32 rows against the definition, within the derived binary32 bound -- no
value left out.

torchaudio is not installed where these tests were written: nothing independent pins the restatement to Kaldi."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import clip_fbank_ref as fref
import clip_mfcc_ref as ref
from clip_host import FbankDesc, build_emul

U = ref.U
LN_EPS = math.log(ref.EPS)


class FbankParams(C.Structure):                    # include/pdmp3_hip.h pdmp3_fbank_params
    _fields_ = [("n_in", C.c_int64), ("win", C.c_int32), ("rows", C.c_int32), ("n_dft", C.c_int32), ("hop", C.c_int32), ("row_pad", C.c_int32),
                ("bins16", C.c_int32), ("n_mels", C.c_int32), ("mels16", C.c_int32), ("n_frames", C.c_int32), ("tile", C.c_int32),
                ("channels", C.c_int32), ("out_mode", C.c_int32), ("use_energy", C.c_int32), ("htk_compat", C.c_int32),
                ("subtract_mean", C.c_int32), ("remove_dc", C.c_int32), ("scale", C.c_float), ("eps", C.c_float),
                ("energy_log_floor", C.c_float), ("span_floats", C.c_uint32), ("lds_bytes", C.c_uint32)]


class MfccParams(C.Structure):                     # include/pdmp3_hip.h pdmp3_mfcc_params
    _fields_ = [("fb", FbankParams), ("n_ceps", C.c_int32), ("ceps16", C.c_int32)]


def _emul():
    lib = build_emul("mfcc")
    lib.emul_clip_mfcc.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    assert lib.emul_mfcc_desc_bytes() == C.sizeof(FbankDesc) and lib.emul_mfcc_params_bytes() == C.sizeof(MfccParams)
    return lib


TABLE_SHAPES = [(23, 13), (80, 80), (40, 1), (23, 17)]


@pytest.mark.parametrize("nm,nc", TABLE_SHAPES, ids=lambda v: str(v))
def test_the_dct_table_is_the_steps_rounded_once(nm, nc):
    from pdmp3_amd import api
    mp, cp = (nm + 15) // 16 * 16, (nc + 15) // 16 * 16
    worst = 0.0
    for q, htk, energy in itertools.product((0.0, 22.0, 0.5), (False, True), (False, True)):
        t = api.mfcc_dct_table(nm, nc, q, htk, energy)
        assert t.shape == (mp, cp) and t.dtype == np.float32
        # the definition step by step: the DCT rows, the lifter, the energy's row, the sqrt 2, then the column order
        want = ref.dct_rows(nm, nc) * ref.lifter(nc, q)[:, None]
        if energy:
            want[0] = 0.0
        elif htk:
            want[0] = want[0] * math.sqrt(2.0)
        order = ref.column_order(nc, htk)
        want = want[order].T                                                      # [Nm, num_ceps]: Bt[m][col]
        got = t[:nm, :nc].astype(np.float64)
        # one rounding to binary32 of a binary64 value; the two binary64 evaluations (C's libm, numpy's) may differ in the last
        # bits of cos / sin of arguments up to pi Nm and of the products: 2^-40 of the largest coefficient covers it
        tol = U * np.abs(want) + 2.0 ** -40 * max(1.0, 1.0 + 0.5 * q) * math.sqrt(2.0)
        err = np.abs(got - want)
        assert (err <= tol).all(), (q, htk, energy, float((err - tol).max()))
        worst = max(worst, float((err / tol).max()))
        pad = np.ones(t.shape, dtype=bool)
        pad[:nm, :nc] = False
        assert (t[pad] == 0.0).all()                                              # (exactly: +0.0 or -0.0 alike)
        assert not np.signbit(t[pad]).any()
        if energy:
            ecol = nc - 1 if htk else 0
            assert (t[:, ecol] == 0.0).all() and order[ecol] == 0
            if nc > 1:
                assert (np.abs(t[:nm, [c for c in range(nc) if c != ecol]]).sum(axis=0) > 0).all()
        if q == 0.0 and nc == nm and not htk and not energy:
            # orthonormal: Bt^T Bt = I to the rounding of the entries -- each entry off by at most u |Bt|, so an entry of the
            # product by at most sum_m (2 u |Bt||Bt'| + u^2 |Bt||Bt'|) <= (2 u + u^2) (Cauchy-Schwarz: rows of norm 1) plus
            # binary64's own evaluation
            g = t[:nm, :nc].astype(np.float64)
            assert np.abs(g.T @ g - np.eye(nc)).max() <= (2.0 * U + U * U) * (1.0 + 1e-6) + nm * 2.0 ** -52
    print("Nm %d num_ceps %d: worst table error / tolerance %.3f" % (nm, nc, worst))


def test_refusals_of_the_planning_calls():
    from pdmp3_amd import api
    assert api.mfcc_check(16000)
    assert api.mfcc_check(16000, num_ceps=1) and api.mfcc_check(16000, num_ceps=23) and api.mfcc_check(16000, num_mel_bins=80, num_ceps=80)
    assert api.mfcc_check(16000, cepstral_lifter=0.0) and api.mfcc_check(16000, cepstral_lifter=0.5)
    assert api.mfcc_check(16000, use_energy=True, htk_compat=True, subtract_mean=True, energy_floor=0.0, scale=32768.0)
    assert api.mfcc_check(16000, use_log_fbank=True) and api.mfcc_check(16000, vtln_warp=1.0)
    assert api.mfcc_check(8000, win_length=200, hop=80) and api.mfcc_check(8000, win_length=16, hop=16, round_to_power_of_two=False, num_mel_bins=40, num_ceps=40)
    for bad in (dict(num_ceps=0), dict(num_ceps=24), dict(num_ceps=-1), dict(num_mel_bins=40, num_ceps=41),
                dict(cepstral_lifter=-1.0), dict(cepstral_lifter=-1e-300), dict(cepstral_lifter=float("nan")), dict(cepstral_lifter=float("inf")),
                dict(use_log_fbank=False),                                        # the power mode
                dict(use_log_fbank=2),
                # everything the filterbank check refuses
                dict(win_length=1), dict(win_length=1025), dict(win_length=401, round_to_power_of_two=False), dict(hop=0), dict(hop=401),
                dict(frame_shift=26.0), dict(num_mel_bins=0), dict(num_mel_bins=257, num_ceps=13), dict(preemphasis_coefficient=-0.1),
                dict(preemphasis_coefficient=1.01), dict(preemphasis_coefficient=float("nan")), dict(window_type="kaiser"), dict(window_type=5),
                dict(blackman_coeff=float("inf")), dict(low_freq=-1.0), dict(high_freq=8000.5), dict(low_freq=4000.0, high_freq=4000.0),
                dict(low_freq=7900.0, high_freq=-200.0), dict(high_freq=-8000.0), dict(energy_floor=-1.0), dict(energy_floor=float("inf")),
                dict(scale=0.0), dict(scale=-1.0), dict(scale=float("inf")), dict(scale=float("nan")), dict(scale=1e-46), dict(scale=1e38),
                dict(n_frames=-1),
                dict(dither=1.0), dict(dither=1e-9), dict(use_power=False), dict(raw_energy=False), dict(snip_edges=False), dict(vtln_warp=1.1),
                dict(vtln_warp=0.9)):
        assert not api.mfcc_check(16000, **bad), bad
        assert bad.keys() & {"num_ceps", "cepstral_lifter", "use_log_fbank"} or not api.fbank_check(16000, **bad), bad
    assert not api.mfcc_check(0) and not api.mfcc_check(-16000, win_length=400, hop=160)
    for args in ((23, 0), (23, 24), (0, 1), (257, 13), (23, 13, -1.0), (23, 13, float("nan")), (23, 13, float("inf"))):
        with pytest.raises(ValueError):
            api.mfcc_dct_table(*args)
    for args in ((400, 512, 160, 23, 0), (400, 512, 160, 23, 24), (1, 2, 1, 23, 13), (400, 512, 0, 23, 13), (400, 512, 401, 23, 13), (400, 256, 160, 23, 13),
                 (400, 600, 160, 23, 13), (400, 512, 160, 0, 1), (400, 512, 160, 257, 13), (1025, 2048, 160, 23, 13), (401, 401, 160, 23, 13)):
        with pytest.raises(ValueError):
            api.mfcc_tile(*args)


def _expected_tile(nw, n, hop, nm, nc):
    """the plan restated: the first region as the filterbank kernel's, then max(Kp + 2, ceps16 + 1) floats a frame; 32 frames
    where they fit 64 KB, else 16"""
    kp, mp, cp, rows = (n // 2 + 15) // 16 * 16, (nm + 15) // 16 * 16, (nc + 15) // 16 * 16, (nw + 3) // 4 * 4
    pad = (2 - hop) % 32
    res = {}
    for tile in (32, 16):
        first = max(-(-((tile - 1) * hop + rows) // hop) * (hop + pad), mp * (tile + 1))
        first = (first + 3) // 4 * 4
        res[tile] = (first + tile * max(kp + 2, cp + 1)) * 4
    tile = 32 if res[32] <= 64 * 1024 else 16
    return tile, pad, res[tile]


def tile_sweep():
    """(Nw, N, hop, n_mels, num_ceps) of the grid the plan is walked over (tests/test_clip_forms_host.py walks it too)"""
    for nw, pow2 in ((2, True), (16, False), (200, True), (400, True), (400, False), (401, True), (1024, True)):
        n = fref.dft_length(nw, pow2)
        for hop in sorted(set([1, 3, 4, 33, 80, 160, 450, 480, nw]) & set(range(1, nw + 1))):
            for nm, nc in ((1, 1), (23, 13), (80, 80), (256, 256), (256, 1)):
                yield nw, n, hop, nm, nc


def test_the_tile_takes_the_larger_of_the_powers_and_the_cepstra():
    from pdmp3_amd import api
    # torchaudio's defaults at 16 kHz: the powers are the larger (258 floats a frame against 17); the same bytes as the
    # filterbank kernel's
    assert api.mfcc_tile(400, 512, 160, 23, 13) == _expected_tile(400, 512, 160, 23, 13) == api.fbank_tile(400, 512, 160, 23)
    assert api.mfcc_tile(400, 512, 160, 23, 13) == (32, 2, (34 * 162 + 32 * 258) * 4)   # (34 chunks of 160 + 2 floats hold the 5360 samples)
    # the cepstra outgrow the powers: 49 floats a frame against 18
    t, pad, lds = api.mfcc_tile(16, 16, 16, 40, 40)
    assert (t, pad, lds) == _expected_tile(16, 16, 16, 40, 40) and t == 32
    first = max(32 * (16 + pad), 48 * 33)
    assert lds == (first + 32 * 49) * 4 and lds == api.fbank_tile(16, 16, 16, 40)[2] + 32 * (49 - 18) * 4
    # the static-array kernel
    t, pad, lds = api.mfcc_tile(1024, 1024, 480, 80, 40)
    assert (t, pad, lds) == _expected_tile(1024, 1024, 480, 80, 40) and t == 16 and 64 * 1024 < lds <= 160 * 1024 - 64
    tiles = {16: 0, 32: 0}
    for nw, n, hop, nm, nc in tile_sweep():
        t, pad, lds = api.mfcc_tile(nw, n, hop, nm, nc)
        assert (t, pad, lds) == _expected_tile(nw, n, hop, nm, nc), (nw, n, hop, nm, nc)
        assert lds <= 160 * 1024 - 64 and (hop + pad) % 32 == 2
        tiles[t] += 1
    assert tiles[16] and tiles[32]
    # a tile of 32 for the filterbank kernel, 16 here: 257 floats of cepstra a frame against 18 of powers push it over 64 KB
    assert api.fbank_tile(16, 16, 1, 256)[0] == 32 and api.mfcc_tile(16, 16, 1, 256, 256)[0] == 16


EMUL_CASES = [
    # Nw, H, power of two, n_mels, num_ceps, Q, sr, channels, start, n_frames, J - start (None: the row is all signal), options
    (400, 160, True, 23, 13, 22.0, 16000, 1, 0, 70, None, {}),
    (400, 160, True, 80, 80, 22.0, 16000, 2, 5000, 40, 3000, {}),                       # frames across and behind J: silent frames, valid inside a tile
    (400, 160, True, 23, 17, 0.5, 16000, 2, 100000, 31, -7, {}),                        # wholly behind J: every frame silent
    (200, 80, True, 23, 1, 22.0, 8000, 1, 77, 34, 2500, dict(scale=32768.0)),
    (400, 160, False, 40, 40, 0.0, 16000, 1, 3, 33, None, dict(window_type="hamming", rho=0.0)),
    (1024, 480, True, 80, 40, 22.0, 48000, 2, 300, 18, 6000, dict(window_type="blackman")),   # tile of 16, more than 64 KB
    (16, 16, False, 40, 40, 22.0, 8000, 1, 0, 33, 400, dict(window_type="hamming", low=0.0)),  # the cepstra outgrow the powers
]


def _edge_case(e):
    """an entry of clip_mfcc_ref.EDGES as a case: one full tile and a partial one, the row all signal; the own rate: 44.1 kHz"""
    import test_clip_fbank_host as tfh
    pow2 = e.get("round_to_power_of_two", True)
    tile = ref.form(e["win_length"], fref.dft_length(e["win_length"], pow2), e["hop"], e["num_mel_bins"], e["num_ceps"])[0]
    return (e["win_length"], e["hop"], pow2, e["num_mel_bins"], e["num_ceps"], 22.0, e["sample_rate"] or 44100, e["channels"], 57, tile + 3, None,
            tfh.edge_options(e))


EMUL_CASES += [_edge_case(e) for e in ref.EDGES.values()]
ENERGIES = [(0, 0, 0.0), (0, 1, 0.0), (1, 0, 0.0), (1, 1, 100.0)]


def _run_emul(lib, y_rows, Ts, T, channels, F, nv, nw, hop, pow2, n_mels, nc, q, sr, o, energy, sub):
    from pdmp3_amd import api
    n = fref.dft_length(nw, pow2)
    tile, row_pad, lds_bytes = api.mfcc_tile(nw, n, hop, n_mels, nc)
    k2 = n // 2
    kp, mp, cp = (k2 + 15) // 16 * 16, (n_mels + 15) // 16 * 16, (nc + 15) // 16 * 16
    dft = api.fbank_table(nw, pow2, o.get("remove_dc", True), o.get("rho", 0.97), o.get("window_type", "povey"), 0.42, o.get("scale", 1.0))
    w32 = api.fbank_filterbank(sr, n, n_mels, o.get("low", 20.0), 0.0)
    fbt = np.zeros((kp, mp), dtype=np.float32)
    fbt[:k2, :n_mels] = w32.T
    use_e, htk, floor = energy
    dct = api.mfcc_dct_table(n_mels, nc, q, bool(htk), bool(use_e))
    assert dct.shape == (mp, cp)
    out = np.full((channels, F * nc + 8), np.float32(-3e9), dtype=np.float32)
    d = FbankDesc(src=y_rows.ctypes.data, dst=out.ctypes.data, src_chan_stride=Ts, dst_chan_stride=F * nc + 8, valid=nv)
    P = FbankParams(n_in=T, win=nw, rows=(nw + 3) // 4 * 4, n_dft=n, hop=hop, row_pad=row_pad, bins16=kp, n_mels=n_mels, mels16=mp, n_frames=F,
                    tile=tile, channels=channels, out_mode=1, use_energy=use_e, htk_compat=htk, subtract_mean=int(sub),
                    remove_dc=int(o.get("remove_dc", True)), scale=o.get("scale", 1.0), eps=2.0 ** -23,
                    energy_log_floor=math.log(floor) if floor > 0 else -math.inf,
                    span_floats=lds_bytes // 4 - tile * max(kp + 2, cp + 1), lds_bytes=lds_bytes)
    Q = MfccParams(fb=P, n_ceps=nc, ceps16=cp)
    assert lib.emul_clip_mfcc(C.byref(d), 1, dft.ctypes.data, fbt.ctypes.data, dct.ctypes.data, C.byref(Q)) == 0
    assert (out[:, F * nc:] == np.float32(-3e9)).all()
    return out[:, :F * nc].reshape(channels, F, nc).astype(np.float64), tile


@pytest.mark.parametrize("case", EMUL_CASES, ids=lambda c: "Nw%d-H%d-%s-m%d-c%d-C%d-s%d" % (c[0], c[1], "p2" if c[2] else "eq", c[3], c[4], c[7], c[8]))
def test_kernel_arithmetic_on_the_host_against_binary64(case):
    lib = _emul()
    nw, hop, pow2, n_mels, nc, q, sr, channels, start, F, left, o = case
    n = fref.dft_length(nw, pow2)
    rng = np.random.default_rng((nw * 131 + hop * 7 + start + nc) & 0xffffffff)
    T = (F - 1) * hop + nw
    Ts = (T + 3) // 4 * 4
    stage = np.full(channels * Ts + 16, np.float32(7e8), dtype=np.float32)        # (guards: nothing outside [0, T) may be read)
    rows = stage[8:8 + channels * Ts].reshape(channels, Ts)
    rows[:, :T] = (rng.random((channels, T), dtype=np.float32) * 2 - 1) * np.float32(0.7) + np.float32(0.05)
    if left is not None:
        rows[:, max(0, left):T] = 0.0
    y = rows[:, :T].copy()
    nv = fref.valid(start + left if left is not None else 2 ** 62, start, nw, hop, F)
    tile0 = _expected_tile(nw, n, hop, n_mels, nc)[0]
    if case[10] == 3000:
        assert 0 < nv < tile0                      # valid ends inside the first tile, and silent frames follow
    w64 = fref.filterbank(sr, n, n_mels, o.get("low", 20.0), 0.0)
    signal = np.abs(fref.frames_of(y[0], start, start, F, nw, hop)).sum(axis=1) > 0
    for energy, sub in itertools.product(ENERGIES, (False, True)):
        got, tile = _run_emul(lib, rows, Ts, T, channels, F, nv, nw, hop, pow2, n_mels, nc, q, sr, o, energy, sub)
        want, bound = ref.mfcc(y, start, start, F, nw, hop, w64, nv, nc, q, pow2, o.get("remove_dc", True), o.get("rho", 0.97),
                               o.get("window_type", "povey"), 0.42, bool(energy[0]), bool(energy[1]), energy[2], sub, o.get("scale", 1.0))
        assert np.isfinite(got).all()
        err = np.abs(got - want)
        assert (err <= bound).all(), (energy, sub, float((err - bound).max()), np.unravel_index(np.argmax(err - bound), err.shape))
        ratio = float((err[:, signal] / bound[:, signal]).max()) if signal.any() else 0.0
        print("Nw %d N %d H %d mels %d ceps %d Q %g C %d start %d energy %s mean %d tile %d: worst error / bound %.4f (%d of %d frames hold signal, valid %d)"
              % (nw, n, hop, n_mels, nc, q, channels, start, energy, sub, tile, ratio, signal.sum(), F, nv))
        if signal.any():
            assert 0.0 < ratio <= 1.0
        if not sub and (~signal).any():
            # a silent frame: L = ln eps in every band; C0 is sqrt(Nm) ln eps (times l[0] = 1, and sqrt 2 with htk_compat), the
            # others vanish in the definition
            sil = want[:, ~signal]
            order = ref.column_order(nc, bool(energy[1]))
            c0 = order.index(0)
            if not energy[0]:
                assert np.allclose(sil[:, :, c0], math.sqrt(n_mels) * LN_EPS * (math.sqrt(2.0) if energy[1] else 1.0), rtol=1e-12, atol=0)
            others = [c for c in range(nc) if c != c0]
            assert (np.abs(sil[:, :, others]) <= 1e-9).all()
        if sub and nv == 0:
            plain, _ = _run_emul(lib, rows, Ts, T, channels, F, nv, nw, hop, pow2, n_mels, nc, q, sr, o, energy, False)
            assert np.array_equal(got, plain)
