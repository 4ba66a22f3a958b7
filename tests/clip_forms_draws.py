"""The seeded geometries of tests/test_gpu_clip_forms.py's sweeps: twelve a call, drawn with a fixed seed from the sizes at which
the feature kernels change course, each kept only where the plan restated in tests/clip_*_ref.py (`form`) puts it in a class
the speech front ends do not reach.  tests/test_clip_forms_host.py holds the draws to that without a GPU."""
import numpy as np

import clip_fbank_ref as fref
import clip_mel_ref as mref
import clip_mfcc_ref as cref
import clip_stft_ref as sref

SIZES = (16, 18, 64, 254, 398, 400, 512, 766, 958, 1022, 1024)
BANDS = (1, 15, 16, 17, 80, 255, 256)
RATES = ((8000, "8k"), (16000, "32k"), (22050, "48k"), (0, "44k-mono"))    # (rate, the stream it is drawn with); 0: the stream's own
INTERESTING = {"tile16-dyn", "tile16-static", "mel-tile", "cepstra", "hop<4", "rows-padded", "idle-waves", "edge-64k", "bands-1", "bands-15",
               "bands-17", "bands-256"}
SEEDS = {"mel": 1001, "fbank": 1002, "mfcc": 1013, "stft": 1004}
N_DRAWS = 12
MEL_MODES = ("power", "log", "log10", "whisper")


def _hops(n):
    return sorted(set(h for h in (1, 2, 3, 4, 5, 31, 33, n // 4, n // 2, n - 1, n) if 1 <= h <= n))


def _pick(rng, seq):
    return seq[int(rng.integers(len(seq)))]


def _one(call, rng):
    """one draw: decode_clips_<call>'s arguments, and "stream"; the classes of its form.  fbank and mfcc take int16-scaled
    samples, as Kaldi does: a quiet stretch stays above the floors (eps, and energy_floor = 1), below which every value of a
    row is the same constant and the definition has nothing to compare"""
    n = _pick(rng, SIZES)
    hop = _pick(rng, _hops(n))
    rate, stream = _pick(rng, RATES)
    channels = int(rng.integers(1, 3))
    if call == "stft":
        p = dict(n_fft=n, hop=hop, sample_rate=rate, channels=channels, normalized=bool(rng.integers(2)), stream=stream,
                 mode=_pick(rng, tuple(sref.MODES)))
        if rng.integers(2):
            p["win_length"] = max(1, n - int(rng.integers(0, n // 2)))
        return p, sref.form(n, hop, sref.MODES[p["mode"]])[3]
    bands = _pick(rng, BANDS)
    if call == "mel":
        p = dict(n_fft=n, hop=hop, n_mels=bands, sample_rate=rate, channels=channels, scale=_pick(rng, ("slaney", "htk")),
                 norm=_pick(rng, ("slaney", None)), stream=stream, mode=_pick(rng, MEL_MODES))
        return p, mref.form(n, hop, bands)[3]
    pow2 = bool(rng.integers(2))
    p = dict(win_length=n, hop=hop, num_mel_bins=bands, sample_rate=rate, channels=channels, round_to_power_of_two=pow2,
             low_freq=_pick(rng, (0.0, 20.0)), use_energy=bool(rng.integers(2)), subtract_mean=bool(rng.integers(2)), scale=32768.0, stream=stream)
    nd = fref.dft_length(n, pow2)
    if call == "fbank":
        p["use_log_fbank"] = bool(rng.integers(2))
        return p, fref.form(n, nd, hop, bands)[3]
    p["num_ceps"] = min(bands, _pick(rng, (1, 13, 256)))
    return p, cref.form(n, nd, hop, bands, p["num_ceps"])[3]


def draw(call):
    """the call's twelve geometries, the same every time: draws outside INTERESTING are rejected"""
    rng = np.random.default_rng(SEEDS[call])
    out = []
    while len(out) < N_DRAWS:
        p, classes = _one(call, rng)
        if classes & INTERESTING:
            out.append(p)
    return out


def no_band_holds_a_bin(call, p, own_rate=44100):
    """True where the filterbank of a draw is all zeros: every band lies between two bins, and the definition has nothing to
    compare"""
    sr = p["sample_rate"] or own_rate
    if call == "mel":
        w = mref.filterbank(sr, p["n_fft"], p["n_mels"], 0.0, 0.0, p["scale"], p["norm"])
    else:
        w = fref.filterbank(sr, fref.dft_length(p["win_length"], p["round_to_power_of_two"]), p["num_mel_bins"], p["low_freq"], 0.0)
    return not (w > 0).any()
