"""Kaldi-style MFCC features of clips (include/pdmp3_bulk.h) restated step by step in binary64 with numpy
alone: the log filterbank and the energy column come from tests/clip_fbank_ref.py (its fbank(), mode 1, which is itself the
definition step by step), then the orthonormal DCT-II rows, the lifter, the energy in C0's place, htk_compat's sqrt 2 and column
order and the mean subtraction as separate steps -- never through the folded table -- and the binary32 error bound the tests
hold the product to.  Nothing here is the product's code.

torchaudio is not installed where this was written, so nothing independent pins this restatement to Kaldi: it was written from
the published definitions of torchaudio.compliance.kaldi.mfcc, and a reader should compare it with them."""
import math

import numpy as np

import clip_fbank_ref as fref

U = fref.U
EPS = fref.EPS


def dct_rows(n_mels, num_ceps):
    """B[c, m], [num_ceps, n_mels]: sqrt(1 / Nm) for c = 0, sqrt(2 / Nm) cos(pi (m + 1/2) c / Nm) below it"""
    m = np.arange(n_mels, dtype=np.float64)[None, :]
    c = np.arange(num_ceps, dtype=np.float64)[:, None]
    b = math.sqrt(2.0 / n_mels) * np.cos(np.pi * (m + 0.5) * c / n_mels)
    b[0] = math.sqrt(1.0 / n_mels)
    return b


def lifter(num_ceps, q):
    """l[c] = 1 + (Q / 2) sin(pi c / Q); Q = 0: ones"""
    if q == 0.0:
        return np.ones(num_ceps)
    return 1.0 + 0.5 * q * np.sin(np.pi * np.arange(num_ceps, dtype=np.float64) / q)


def column_order(num_ceps, htk_compat):
    """the cepstral index every output column holds"""
    return list(range(1, num_ceps)) + [0] if htk_compat else list(range(num_ceps))


def coefficients(n_mels, num_ceps, q, htk_compat, use_energy):
    """[num_ceps (by cepstral index, not yet reordered), n_mels]: what multiplies L[m] in C[c], built from the steps (for the
    bound's |Bt|, and for the table's test); the energy's row is zeros"""
    b = dct_rows(n_mels, num_ceps) * lifter(num_ceps, q)[:, None]
    if use_energy:
        b[0] = 0.0
    elif htk_compat:
        b[0] = b[0] * math.sqrt(2.0)
    return b


def mfcc(y, pos0, start, n_frames, nw, hop, w, n_valid, num_ceps=13, q=22.0, round_pow2=True, remove_dc=True, rho=0.97, window_type="povey",
         blackman_coeff=0.42, use_energy=False, htk_compat=False, energy_floor=0.0, subtract_mean=False, scale=1.0):
    """y: [C, T] binary32 values of the signal from position pos0 on; w: clip_fbank_ref.filterbank(...).  -> (out, bound),
    binary64 [C, n_frames, num_ceps]: the definition on those values, and what a binary32 evaluation may differ from it by
    (DESIGN.md section 12), u = 2^-24.  With L, b the log filterbank and its bound (clip_fbank_ref.fbank, mode 1), Bt the
    coefficient of L[m] in a column -- l[c] s B[c, m], rounded once to binary32 in the product -- and mels16 = Nm rounded up to 16:
      dC = sum_m |Bt| b_m + (mels16 + 2) u sum_m |Bt| (|L_m| + b_m)
    -- a binary32 dot product of length mels16 with once-rounded coefficients in any order (g_mels16 (1 + u) + u <=
    (mels16 + 2) u for mels16 <= 256; the padded bands meet zero coefficients and add nothing).  The energy column and its bound
    are clip_fbank_ref's.  The mean subtraction's bound is clip_fbank_ref's, applied to these columns:
      dmu = (sum b + g_(nv-1) sum (|v| + b)) / nv + DIV_C u (|mu| + the former);  final = b + dmu + u (|v - mu| + b + dmu)"""
    n_mels = w.shape[0]
    both, both_b = fref.fbank(y, pos0, start, n_frames, nw, hop, w, 0, round_pow2, remove_dc, rho, window_type, blackman_coeff, 1, True, False,
                              energy_floor, False, scale)
    en, den = both[:, :, 0], both_b[:, :, 0]
    lg, dlg = both[:, :, 1:], both_b[:, :, 1:]
    assert lg.shape[2] == n_mels
    b = dct_rows(n_mels, num_ceps)
    lift = lifter(num_ceps, q)
    out = (lg @ b.T) * lift[None, None, :]                                        # the DCT, then the lifter
    babs = np.abs(coefficients(n_mels, num_ceps, q, htk_compat, use_energy))
    mels16 = (n_mels + 15) // 16 * 16
    bound = dlg @ babs.T + (mels16 + 2) * U * ((np.abs(lg) + dlg) @ babs.T)
    if use_energy:                                                                # the energy replaces C0
        out[:, :, 0] = en
        bound[:, :, 0] = den
    if htk_compat:
        if not use_energy:
            out[:, :, 0] = out[:, :, 0] * math.sqrt(2.0)
        order = column_order(num_ceps, True)                                      # C0 moves behind the others
        out, bound = out[:, :, order], bound[:, :, order]
    if subtract_mean and n_valid > 0:
        nv = int(n_valid)
        mu = out[:, :nv].mean(axis=1, keepdims=True)
        dsum = bound[:, :nv].sum(axis=1, keepdims=True) + fref.gamma(max(nv - 1, 0)) * (np.abs(out[:, :nv]) + bound[:, :nv]).sum(axis=1, keepdims=True)
        dmu = dsum / nv
        dmu = dmu + fref.DIV_C * U * (np.abs(mu) + dmu)
        v = out - mu
        bound = bound + dmu + U * (np.abs(v) + bound + dmu)
        out = v
    return out, bound


# ---- the plan of a workgroup of k_clip_mfcc restated, and the classes of a geometry ("launch forms") ----
def form(nw, n, hop, n_mels, num_ceps):
    """-> (tile, row_pad, lds_bytes, classes): clip_fbank_ref.form with the second region the larger of the powers
    [tile][bins16 + 2] and the cepstra [tile][ceps16 + 1]"""
    import clip_mel_ref as mref
    rows, kp, mp, cp = (nw + 3) // 4 * 4, (n // 2 + 15) // 16 * 16, (n_mels + 15) // 16 * 16, (num_ceps + 15) // 16 * 16
    for tile in (32, 16):
        first, what = mref.plan_first(rows, hop, mp, tile)
        lds = (first + tile * max(kp + 2, cp + 1)) * 4
        if lds <= mref.LDS_SOFT:
            break
    assert lds <= mref.LDS_MAX
    c = {mref.launch_of(tile, lds), what, "cepstra" if cp + 1 > kp + 2 else "powers"} | mref.shape_classes(nw, rows, hop, kp, n_mels)
    if mref.LDS_SOFT - 64 < lds <= mref.LDS_SOFT:
        c.add("edge-64k")
    return tile, (2 - hop) % 32, lds, c


def _e(win, hop, n_mels, num_ceps, rate, stream, channels=1, **options):
    return dict(dict(win_length=win, hop=hop, num_mel_bins=n_mels, num_ceps=num_ceps, sample_rate=rate, channels=channels, **options), stream=stream)


# the shapes whose launch forms no speech front end reaches; `stream` names one of test_gpu_clip_audio's, the rest are
# decode_clips_mfcc's arguments
EDGES = {
    "taco-1024-256-80-40-stereo": _e(1024, 256, 80, 40, 22050, "22k", 2),
    "551-220-80-13": _e(551, 220, 80, 13, 22050, "22k"),
    "900-hop4-exactly-64k": _e(900, 4, 80, 13, 16000, "16k-mono"),
    "960-hop4-n-equals-nw-exactly-64k": _e(960, 4, 80, 13, 16000, "16k-mono", round_to_power_of_two=False),
    "401-hop3-20-20-mean-energy": _e(401, 3, 20, 20, 16000, "32k", subtract_mean=True, use_energy=True),
    "512-hop2-256-256": _e(512, 2, 256, 256, 16000, "32k", round_to_power_of_two=False),
    "16-hop4-1-band-1-cepstrum": _e(16, 4, 1, 1, 8000, "8k", low_freq=0.0, scale=32768.0),
    "64-hop5-15-bands": _e(64, 5, 15, 15, 8000, "8k", low_freq=0.0, scale=32768.0),
    "64-hop5-17-bands-13-cepstra-stereo": _e(64, 5, 17, 13, 8000, "8k", 2, low_freq=0.0, scale=32768.0),
    # first region the mel tile, second region the cepstra, 16 column tiles over four waves
    "64-hop64-256-256": _e(64, 64, 256, 256, 16000, "16k-mono", round_to_power_of_two=False, low_freq=0.0),
}
EXACT_EDGE = ("900-hop4-exactly-64k", "960-hop4-n-equals-nw-exactly-64k")
