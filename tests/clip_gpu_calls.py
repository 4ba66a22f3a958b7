"""What is particular to one clip feature call and used by more than one test module on the GPU: how the call is run into a
guarded destination (clip_gpu.run with the call's shapes) and how its rows are held to the definition of tests/clip_*_ref.py on
the product's own signal (clip_gpu.signal).  A helper that one test module alone uses stays in that module."""
import functools

import numpy as np

import clip_audio_ref as aref
import clip_beat_ref as bref
import clip_cqt_ref as qref
import clip_fbank_ref as fref
import clip_gpu as cg
import clip_loudness_ref as lref
import clip_mel_ref as mref
import clip_mfcc_ref as cref
import clip_pitch_ref as pref
import clip_pyin_ref as yref
import clip_r128_ref as rref
import clip_stft_long_ref as slref
import clip_stft_ref as sref
from clip_gpu import GUARD, SENT

MEL_MODES = ["power", "log", "log10", "whisper"]
STFT_MODES = ["complex", "magnitude", "power", "log", "log10"]
STFT_LONG_PA = dict(sample_rate=0, n_fft=2048, hop=512, channels=2)                  # the 48 kHz stream at its own rate, stereo
MEL_LONG_PA = dict(sample_rate=0, n_fft=2048, hop=512, n_mels=128, scale="slaney", norm="slaney", channels=2)     # the 48 kHz stream at its own rate
STFT_LONG_FLOORS = {3: 1e-10, 4: 1e-10}
LOUDNESS_CASES = {
    # streams, rate, channels
    "48k-32k-stereo-at-32000": (["48k", "32k"], 32000, 2),
    "44k-mono-own-rate": (["44k-mono"], 0, 1),
    "8k-own-rate": (["8k"], 0, 2),
    "22k-at-16000-mono": (["22k"], 16000, 1),
}


def centred_starts(name, p, f):
    """at 0, a small odd number, mid-stream, across the end and behind it"""
    j_all = cg.j_all(p, name)
    return [0, 57, j_all // 3 + 11, max(j_all - (f // 2) * p["hop"] - 3, 0), j_all + 3]


# ---- decode_clips_audio ----
def audio_run(dec, kind, clips, t, rate=0, channels=0, width=0, rolloff=0.0, c_out=None):
    """clips: (stream name, start) -> (host copy [k, c, t], valid)"""
    return cg.run(dec, "decode_clips_audio", kind, clips, t, c_out or channels, (t,), sample_rate=rate, channels=channels, width=width, rolloff=rolloff)


def audio_check(name, start, got, valid, t, rate, channels, width=6, rolloff=0.99):
    """one row against the definition; -> worst error / bound"""
    ix, lr = cg.ref(name)
    rate = rate or ix.rate
    x = aref.channels64(lr, ix.channels, channels)
    j_all = aref.out_length(ix.samples, ix.rate, rate)
    assert valid == min(max(j_all - start, 0), t), (name, start, valid)
    assert (got[:, valid:] == 0).all(), (name, start)
    y64, bound = aref.resample64(x, ix.rate, rate, width, rolloff, start, t)
    err = np.abs(got.astype(np.float64) - y64)
    if rate == ix.rate:
        assert np.array_equal(got.astype(np.float64), y64), "%s at %d: not the whole-stream decode bit for bit" % (name, start)
        return 0.0
    assert (err <= bound).all(), "%s at %d -> %d Hz: error beyond the bound by %g at %s" % (
        name, start, rate, float((err - bound).max()), np.unravel_index(np.argmax(err - bound), err.shape))
    nz = bound > 0
    return float((err[nz] / bound[nz]).max(initial=0.0))


def audio_rows(dec, clips, t, rate, channels, c):
    """the audio call's rows of the clips, through a guarded device destination -> ([k, c, t], valid)"""
    big, view = cg.destination("device", len(clips), c, (t,))
    out, valid = dec.decode_clips_audio(cg.src(clips), t, rate, channels, out=view)
    return cg.host(big)[:, :, :t].copy(), valid


# ---- decode_clips_mel, decode_clips_mel_long ----
def mel_filterbank(p, name):
    return mref.filterbank(cg.rate(p, name), p["n_fft"], p["n_mels"], p.get("f_min", 0.0), p.get("f_max", 0.0), p["scale"], p["norm"])


def mel_run(dec, kind, clips, f, p, mode, floor=1e-10, call="decode_clips_mel"):
    """clips: (stream name, start) -> (host copy [k, c, nm, f], valid)"""
    return cg.run(dec, call, kind, clips, f, p["channels"], (p["n_mels"], f), mode=mode, floor=floor, **p)


def mel_long_run(dec, kind, clips, f, p, mode, floor=1e-10):
    return mel_run(dec, kind, clips, f, p, mode, floor, "decode_clips_mel_long")


def mel_check(clips, sig, got, valid, f, p, mode, floor=1e-10):
    """every row against the definition on `sig`; -> worst error / bound over the rows that hold signal"""
    worst = 0.0
    m = MEL_MODES.index(mode)
    for i, (n, s) in enumerate(clips):
        assert int(valid[i]) == mref.valid(cg.j_all(p, n), s, p["hop"], f), (n, s, valid[i])
        s0, y = sig[i]
        want, bound = mref.mel(y, s0, s, f, p["n_fft"], p["hop"], mel_filterbank(p, n), m, floor)
        err = np.abs(got[i].astype(np.float64) - want)
        assert (err <= bound).all(), "%s at %d, mode %s: error beyond the bound by %g at %s" % (
            n, s, mode, float((err - bound).max()), np.unravel_index(np.argmax(err - bound), err.shape))
        nz = bound > 0
        if m == 0:
            assert (got[i][~nz] == 0.0).all()
        if np.abs(y).sum() > 0 and nz.any():        # (a start inside the first N / 2 samples: the span's last samples belong to no frame)
            r = float((err[nz] / bound[nz]).max())
            assert 0.0 < r <= 1.0, (n, s, mode, r)
            worst = max(worst, r)
    return worst


def mel_starts(name, p, f):
    """centred_starts and one far behind the end"""
    return centred_starts(name, p, f) + [cg.j_all(p, name) + 5 * p["n_fft"]]


# ---- decode_clips_fbank, decode_clips_mfcc ----
def fbank_n(p):
    return fref.dft_length(p["win_length"], p.get("round_to_power_of_two", True))


def fbank_d(p):
    """the floats of a frame: the bands, and the energy where it is asked for"""
    return p["num_mel_bins"] + int(p.get("use_energy", False))


def fbank_filterbank(p, name):
    return fref.filterbank(cg.rate(p, name), fbank_n(p), p["num_mel_bins"], p.get("low_freq", 20.0), p.get("high_freq", 0.0))


def fbank_definition(y, start, f, p, w, nv):
    return fref.fbank(y, start, start, f, p["win_length"], p["hop"], w, nv, p.get("round_to_power_of_two", True), p.get("remove_dc_offset", True),
                      p.get("preemphasis_coefficient", 0.97), p.get("window_type", "povey"), p.get("blackman_coeff", 0.42),
                      int(p.get("use_log_fbank", True)), p.get("use_energy", False), p.get("htk_compat", False), p.get("energy_floor", 1.0),
                      p.get("subtract_mean", False), p.get("scale", 1.0))


def mfcc_definition(y, start, f, p, w, nv):
    return cref.mfcc(y, start, start, f, p["win_length"], p["hop"], w, nv, p["num_ceps"], p.get("cepstral_lifter", 22.0),
                     p.get("round_to_power_of_two", True), p.get("remove_dc_offset", True), p.get("preemphasis_coefficient", 0.97),
                     p.get("window_type", "povey"), p.get("blackman_coeff", 0.42), p.get("use_energy", False), p.get("htk_compat", False),
                     p.get("energy_floor", 1.0), p.get("subtract_mean", False), p.get("scale", 1.0))


def fbank_signal(dec, clips, f, p):
    """clip_gpu.signal for the Kaldi-style calls: frames of win_length samples from `start` on"""
    return cg.signal(dec, clips, f, p, centred=False)


def fbank_run(dec, kind, clips, f, p):
    """clips: (stream name, start) -> (host copy [k, c, f, d], valid)"""
    return cg.run(dec, "decode_clips_fbank", kind, clips, f, p["channels"], (f, fbank_d(p)), **p)


def mfcc_run(dec, kind, clips, f, p):
    """clips: (stream name, start) -> (host copy [k, c, f, num_ceps], valid)"""
    return cg.run(dec, "decode_clips_mfcc", kind, clips, f, p["channels"], (f, p["num_ceps"]), **p)


def fbank_check(clips, sig, got, valid, f, p):
    """every row against the definition on `sig`; -> worst error / bound over the rows that hold signal"""
    worst = 0.0
    for i, (n, s) in enumerate(clips):
        nv = fref.valid(cg.j_all(p, n), s, p["win_length"], p["hop"], f)
        assert int(valid[i]) == nv, (n, s, valid[i], nv)
        y = sig[i][1]
        want, bound = fbank_definition(y, s, f, p, fbank_filterbank(p, n), nv)
        err = np.abs(got[i].astype(np.float64) - want)
        assert (err <= bound).all(), "%s at %d: error beyond the bound by %g at %s" % (
            n, s, float((err - bound).max()), np.unravel_index(np.argmax(err - bound), err.shape))
        nz = bound > 0
        if not p.get("use_log_fbank", True) and not p.get("subtract_mean", False):
            assert (got[i][~nz] == 0.0).all()
        if p.get("subtract_mean", False) and nv == 1 and f == 1:
            # the only frame minus the mean of that one frame: x - x / 1, exactly 0.0 in the definition and in binary32 alike,
            # so no error can show here; the row is held to that instead
            assert (want == 0.0).all() and (got[i] == 0.0).all(), (n, s)
        elif np.abs(y).sum() > 0:
            r = float((err[nz] / bound[nz]).max())
            assert 0.0 < r <= 1.0, (n, s, r)
            worst = max(worst, r)
    return worst


def mfcc_check(clips, sig, got, valid, f, p):
    """every row against the definition on `sig`; -> worst error / bound over the rows that hold signal"""
    worst = 0.0
    for i, (n, s) in enumerate(clips):
        nv = fref.valid(cg.j_all(p, n), s, p["win_length"], p["hop"], f)
        assert int(valid[i]) == nv, (n, s, valid[i], nv)
        y = sig[i][1]
        want, bound = mfcc_definition(y, s, f, p, fbank_filterbank(p, n), nv)
        assert np.isfinite(got[i]).all()
        err = np.abs(got[i].astype(np.float64) - want)
        assert (err <= bound).all(), "%s at %d: error beyond the bound by %g at %s" % (
            n, s, float((err - bound).max()), np.unravel_index(np.argmax(err - bound), err.shape))
        if p.get("subtract_mean", False) and nv == 1 and f == 1:
            # the only frame minus the mean of that one frame: x - x / 1, exactly 0.0 in the definition and in binary32 alike
            assert (want == 0.0).all() and (got[i] == 0.0).all(), (n, s)
        elif np.abs(y).sum() > 0:
            r = float((err / bound).max())
            assert 0.0 < r <= 1.0, (n, s, r)
            worst = max(worst, r)
    return worst


def fbank_starts(name, p, f):
    j_all = cg.j_all(p, name)
    return [0, 57, j_all // 3 + 11, max(j_all - (f // 2) * p["hop"] - 3, 0), j_all - p["win_length"] // 2, j_all + 3, j_all + 5 * p["win_length"]]


# ---- decode_clips_stft, decode_clips_stft_long ----
def stft_per(p, mode):
    """the floats of a frame"""
    return (p["n_fft"] // 2 + 1) * (2 if mode == "complex" else 1)


def stft_inner(nb, f, mode):
    return (nb, f, 2) if mode == "complex" else (nb, f)


def stft_run(dec, kind, clips, f, p, mode, floor=1e-10, offset=0, call="decode_clips_stft"):
    """clips: (stream name, start) -> (host copy [k, c, nb, f(, 2)], valid)"""
    return cg.run(dec, call, kind, clips, f, p["channels"], stft_inner(p["n_fft"] // 2 + 1, f, mode), offset, mode=mode, floor=floor, **p)


def stft_long_run(dec, kind, clips, f, p, mode, floor=1e-10, offset=0):
    return stft_run(dec, kind, clips, f, p, mode, floor, offset, "decode_clips_stft_long")


def _stft_row(n, s, got, want, bound, signal, mode):
    """one clip's rows within the bound, exactly 0 where it is 0 in modes 0 - 2 -> worst error / bound, or None without signal"""
    m = STFT_MODES.index(mode)
    assert want.shape == got.shape
    err = np.abs(got.astype(np.float64) - want)
    assert (err <= bound).all(), "%s at %d, mode %s: error beyond the bound by %g at %s" % (
        n, s, mode, float((err - bound).max()), np.unravel_index(np.argmax(err - bound), err.shape))
    nz = bound > 0
    if m <= 2:
        assert (got[~nz] == 0.0).all()
    if not (signal and nz.any()):               # (a start inside the first N / 2 samples: the span's last samples belong to no frame)
        return None
    r = float((err[nz] / bound[nz]).max())
    assert 0.0 < r <= 1.0, (n, s, mode, r)
    if m == 0:
        # the signal is no even function of n about any frame's centre: Im is far above the bound somewhere, so its sign (and a
        # swap with Re) shows in the comparison above
        assert (np.abs(want[..., 1]) > 100.0 * bound[..., 1])[nz[..., 1]].any()
        assert (np.abs(want[..., 0] - want[..., 1]) > 100.0 * bound[..., 0])[nz[..., 0]].any()
    return r


def stft_check(clips, sig, got, valid, f, p, mode, floor=1e-10):
    """every row against the definition on `sig`; -> worst error / bound over the rows that hold signal"""
    worst = 0.0
    for i, (n, s) in enumerate(clips):
        assert int(valid[i]) == sref.valid(cg.j_all(p, n), s, p["hop"], f), (n, s, valid[i])
        s0, y = sig[i]
        want, bound = sref.stft(y, s0, s, f, p["n_fft"], p["hop"], STFT_MODES.index(mode), floor, p.get("win_length"), p.get("window"),
                                p.get("normalized", False))
        worst = max(worst, _stft_row(n, s, got[i], want, bound, np.abs(y).sum() > 0, mode) or 0.0)
    return worst


def stft_long_wants(clips, sig, f, p):
    """per clip {mode: (out, bound)}: the definition on the product's own signal, once for all modes"""
    return [slref.stft_all(y, s0, s, f, p["n_fft"], p["hop"], STFT_LONG_FLOORS, p.get("win_length"), p.get("window"), p.get("normalized", False))
            for (n, s), (s0, y) in zip(clips, sig)]


def stft_long_check(clips, sig, wants, got, valid, f, p, mode):
    """every row against the definition; -> worst error / bound over the rows that hold signal"""
    worst = 0.0
    m = STFT_MODES.index(mode)
    K = p["n_fft"] // 2 + 1
    for i, (n, s) in enumerate(clips):
        assert int(valid[i]) == sref.valid(cg.j_all(p, n), s, p["hop"], f), (n, s, valid[i])
        want, bound = wants[i][m]
        if m == 0:
            assert (got[i][:, 0, :, 1] == 0.0).all() and (got[i][:, K - 1, :, 1] == 0.0).all()     # Im of bins 0 and N / 2
        worst = max(worst, _stft_row(n, s, got[i], want, bound, np.abs(sig[i][1]).sum() > 0, mode) or 0.0)
    return worst


# ---- decode_clips_cqt (and decode_clips_chroma, which folds it) ----
def cqt_geo(p):
    return {k: p[k] for k in ("fmin", "n_bins", "bins_per_octave", "filter_scale", "norm", "scale") if k in p}


def cqt_shape(p):
    return {k: p[k] for k in ("fmin", "n_bins", "bins_per_octave", "filter_scale") if k in p}


def cqt_run(dec, kind, clips, f, p, mode, floor=1e-10, offset=0):
    """clips: (stream name, start) -> (host copy [k, c, n_bins, f(, 2)], valid)"""
    return cg.run(dec, "decode_clips_cqt", kind, clips, f, p["channels"], stft_inner(p["n_bins"], f, mode), offset, mode=mode, floor=floor, **p)


def cqt_signal(dec, clips, f, p):
    """clip_gpu.signal with the longest filter's length N_0 for n_fft: its half is h_0, the lead of the first frame"""
    h0 = int(qref.lengths(cg.rate(p, clips[0][0]), **cqt_shape(p))[2][0])
    return cg.signal(dec, clips, f, dict(p, n_fft=2 * h0 + 1))


# ---- decode_clips_loudness, decode_clips_r128 ----
def loud_rate(clips, rate):
    """the rate the loudness calls work at: `rate`, or the first clip's stream's own"""
    return rate or cg.source(clips[0][0])[1].rate


def _loud_run(dec, call, n_stats, kind, clips, t, rate, channels, c, curves, given, **kw):
    """the loudness or the r128 call into a guarded audio destination and, for every curve (keyword -> length of a row), an array
    of one row more than the clips; `given` False: the call gets None for each, and none may be written ->
    (audio [k, c, t], stats, {keyword: the whole array}, valid), host copies"""
    k = len(clips)
    big, view = cg.destination(kind, k, c or channels, (t,))
    arrays = {name: cg.filled(kind, (k + 1, n)) for name, n in curves.items()}
    audio, stats, valid = getattr(dec, call)(cg.src(clips), t, rate, channels, out=view, **{name: a if given else None for name, a in arrays.items()}, **kw)
    assert audio is view and tuple(stats.shape) == (k, n_stats) and hasattr(stats, "data_ptr") == (kind == "device")
    host = cg.host(big)
    assert (host[:, :, t:] == SENT).all(), "written behind a row's samples"
    rows = {name: cg.host(a) for name, a in arrays.items()}
    for r in rows.values():
        assert (r[k] == SENT).all() and (given or (r == SENT).all()), "written behind the curves' rows"
    return host[:, :, :t].copy(), np.array(cg.host(stats)), rows, valid


def loudness_run(dec, kind, clips, t, rate=0, channels=0, c=None, momentary=True, **kw):
    """clips: (stream name, start) -> (audio [k, c, t], stats [k, 8], momentary [k, J] or None, valid), host copies"""
    J = lref.plan(loud_rate(clips, rate), t)["J"]
    audio, stats, rows, valid = _loud_run(dec, "decode_clips_loudness", 8, kind, clips, t, rate, channels, c, {"momentary": J}, momentary, **kw)
    return audio, stats, rows["momentary"][:len(clips)].copy() if momentary else None, valid


def r128_run(dec, kind, clips, t, rate=0, channels=0, c=None, curves=True, **kw):
    """clips: (stream name, start) -> (audio [k, c, t], stats [k, 16], momentary [k, J], short-term [k, Js], valid), host copies"""
    p = rref.plan(loud_rate(clips, rate), t)
    audio, stats, rows, valid = _loud_run(dec, "decode_clips_r128", 16, kind, clips, t, rate, channels, c,
                                          {"momentary": p["J"], "short_term": p["Jsmax"]}, curves, **kw)
    return audio, stats, rows["momentary"][:len(clips)].copy(), rows["short_term"][:len(clips)].copy(), valid


def loudness_check(x, want_valid, got, fs, **kw):
    """rows x [k, c, t] of the audio call against the loudness call's (audio, stats, momentary, valid) -> (the references, worst
    error / bound, smallest margin in dB, undecided clips)"""
    audio, stats, mom, valid = got
    assert np.array_equal(valid, want_valid)
    refs, worst, margin, undecided = [], 0.0, np.inf, 0
    for i in range(x.shape[0]):
        m = lref.measure(x[i], fs, **kw)
        refs.append(m)
        worst = max(worst, lref.check_stats(m, stats[i], None if mom is None else mom[i]))
        margin = min(margin, m.margin)
        undecided += m.undecided
        want = (x[i] * np.float32(stats[i, 3])).astype(np.float32)
        assert np.array_equal(audio[i].view(np.uint32), want.view(np.uint32)), "clip %d: audio is not x * g" % i
        assert np.float32(stats[i, 2]) == np.abs(x[i]).max()
    assert undecided * 10 <= x.shape[0], "%d of %d clips undecided" % (undecided, x.shape[0])
    print("worst error / bound %.3g, smallest gate margin %.3g dB, %d undecided of %d" % (worst, margin, undecided, x.shape[0]))
    return refs, worst, margin, undecided


def r128_check(x, want_valid, got, fs, curves=True, **kw):
    """rows x [k, c, t] of the audio call against the call's (audio, stats, momentary, short-term, valid) -> (the references,
    worst error / bound, smallest range-gate margin in bounds, undecided clips)"""
    audio, stats, mom, st, valid = got
    assert np.array_equal(valid, want_valid)
    refs, worst, margin, margin_db, undecided = [], 0.0, np.inf, np.inf, 0
    for i in range(x.shape[0]):
        m = rref.measure(x[i], fs, **kw)
        refs.append(m)
        worst = max(worst, rref.check_stats(m, stats[i], mom[i] if curves else None, st[i] if curves else None))
        margin, margin_db = min(margin, m.r_margin_bounds), min(margin_db, m.r_margin)
        undecided += m.undecided or m.r_undecided
        want = (x[i] * np.float32(stats[i, 3])).astype(np.float32)
        assert np.array_equal(audio[i].view(np.uint32), want.view(np.uint32)), "clip %d: audio is not x * g" % i
        assert np.float32(stats[i, 2]) == np.abs(x[i]).max() and stats[i, 8] >= stats[i, 2]
    assert undecided * 10 <= x.shape[0], "%d of %d clips undecided" % (undecided, x.shape[0])
    print("r128: worst error / bound %.3g, smallest range-gate margin %.3g dB = %.3g bounds, %d undecided of %d" %
          (worst, margin_db, margin, undecided, x.shape[0]))
    return refs, worst, margin, undecided


# ---- decode_clips_pyin ----
@functools.lru_cache(maxsize=None)
def _pyin_tables_cached(key):
    from pdmp3_amd import api
    a = dict(key)
    return api.pyin_tables(a["sample_rate"], **{k: v for k, v in a.items() if k != "sample_rate"})


def pyin_tables(a):
    """api.pyin_tables of the arguments a (clip_pyin_ref.args), once a process"""
    return _pyin_tables_cached(tuple(sorted((k, v) for k, v in a.items() if k != "channels")))


def pyin_pitch_args(a, channels):
    """what decode_clips_pitch takes for the curve that decode_clips_pyin works on"""
    n, w, hop = pref.defaults(a["frame_length"], a["win_length"], a["hop"])
    return dict(sample_rate=a["sample_rate"], frame_length=n, win_length=w, hop=hop, fmin=a["fmin"], fmax=a["fmax"], channels=channels)


def pyin_run(dec, kind, clips, f, a, channels, mode, **more):
    """clips: (stream name, start) -> (host copy [k, c, 4 or n_b + 1, f], valid)"""
    rows = 4 if mode == "pitch" else yref.numbers(a)["n_b"] + 1
    return cg.run(dec, "decode_clips_pyin", kind, clips, f, channels, (rows, f), out_mode=mode, channels=channels, **dict(a, **more))


def pyin_curve(dec, clips, f, a, channels):
    """decode_clips_pitch's own curve of the clips -> (host copy [k, c, tmax + 1, f], valid)"""
    k = yref.numbers(a)
    return cg.run(dec, "decode_clips_pitch", "device", clips, f, channels, (k["tmax"] + 1, f), out_mode="curve", **pyin_pitch_args(a, channels))


def pyin_check_both(clips, curve, obs, planes, a, channels):
    """-> (worst error / bound of the observation, the most troughs of a frame, frames without the margin, frames)"""
    k, t = yref.numbers(a), pyin_tables(a)
    worst, most, open_frames, frames = 0.0, 0, 0, 0
    for i in range(len(clips)):
        for c in range(channels):
            w, m = yref.check_observation(curve[i, c], obs[i, c], t, k["tmin"], k["tmax"], a["no_trough_prob"])
            o, _, _ = yref.check_path(obs[i, c], planes[i, c], t)
            worst, most, open_frames, frames = max(worst, w), max(most, m), open_frames + o, frames + obs.shape[-1]
    return worst, most, open_frames, frames


# ---- decode_clips_beats ----
BEAT_P0 = dict(sample_rate=22050, n_fft=2048, hop=512, n_mels=128, lag=1, max_size=1, win_length=384, channels=1)      # the defaults, spelled out
BEAT_TIGHTNESS = 100.0


@functools.lru_cache(maxsize=None)
def beat_tables(period, tightness=BEAT_TIGHTNESS):
    from pdmp3_amd import api
    return api.beat_tables(period, tightness=tightness)


def beat_bpm_of(period, sr, hop):
    """a bpm whose period is `period`: the middle of its rounding interval"""
    bpm = 60.0 * sr / (hop * period)
    assert bref.period_of(bpm, sr, hop) == period
    return bpm


def beat_run(dec, kind, clips, f, p, mode, **kw):
    """-> (host copy [k, c, f] or [k, c, 2, f], stats [k, c, 8], valid); the guard floats behind every row are looked at"""
    k, c = len(clips), p["channels"]
    rows = 1 if mode == "score" else 2
    big, view = cg.destination(kind, k, c, (rows, f))
    dst = view[:, :, 0] if mode == "score" else view
    stats = cg.filled(kind, (k, c, 8))
    out, st, valid = dec.decode_clips_beats(cg.src(clips), f, out_mode=mode, out=dst, stats=stats, **dict(p, **kw))
    assert out is dst and st is stats
    per = rows * f
    host = cg.host(big).reshape(k, c, per + GUARD)
    assert (host[:, :, per:] == SENT).all(), "written behind a row's floats"
    got = host[:, :, :per].copy()
    return (got if mode == "score" else got.reshape(k, c, 2, f)), cg.host(stats).copy(), valid


def beat_onset(dec, clips, f, p):
    """decode_clips_tempogram's onset envelope of the clips -> (host copy [k, c, f], valid)"""
    q = {a: p[a] for a in BEAT_P0}
    big, view = cg.destination("device", len(clips), p["channels"], (1, f))
    out, valid = dec.decode_clips_tempogram(cg.src(clips), f, out_mode="onset", out=view[:, :, 0], **q)
    return cg.host(big)[:, :, :f].copy(), valid


def beat_same(a, b, what):
    assert np.array_equal(cg.bits(np.asarray(a, dtype=np.float32)), cg.bits(np.asarray(b, dtype=np.float32))), what


def beat_check_chain(dec, clips, f, p, period, kind="device"):
    """every stage of the clips at this period against the restatement on the stage before; -> (beats rows, stats, valid)"""
    sr = cg.rate(p, clips[0][0])
    bpm = beat_bpm_of(period, sr, p["hop"])
    g, tx = beat_tables(period)
    env, valid = beat_onset(dec, clips, f, p)
    score, s0, v0 = beat_run(dec, kind, clips, f, p, "score", bpm=bpm)
    dp, s1, v1 = beat_run(dec, kind, clips, f, p, "dp", bpm=bpm)
    assert np.array_equal(valid, v0) and np.array_equal(valid, v1)
    beat_same(s0, s1, "stats of modes 0 and 1")
    res = {}
    for trim in (True, False):
        beats, s2, v2 = beat_run(dec, kind, clips, f, p, "beats", bpm=bpm, trim=trim)
        assert np.array_equal(valid, v2)
        for i in range(len(clips)):
            n = int(valid[i])
            for c in range(p["channels"]):
                what = (clips[i], period, trim, c)
                o = env[i, c, :n]
                run = bref.runs(o)
                # the score stage on the onset mode's own output
                want = bref.local_score(o, period, g)[1] if run else np.zeros(n, dtype=np.float32)
                beat_same(score[i, c, :n], want, what + ("score",))
                assert not score[i, c, n:].any()
                # the programme stage on mode "score"'s output
                cum, back = bref.programme(score[i, c, :n], period, tx) if run else (np.zeros(n), np.full(n, -1))
                with np.errstate(over="ignore"):
                    beat_same(dp[i, c, 0, :n], cum.astype(np.float32), what + ("cum",))
                beat_same(dp[i, c, 1, :n], back.astype(np.float32), what + ("back",))
                assert not dp[i, c, 0, n:].any() and (dp[i, c, 1, n:] == -1).all()
                # the beats stage on that programme; mode "beats" alone is the chain
                whole = bref.track(o, f, period, g, tx, trim)
                if run:
                    r = bref.pick(score[i, c, :n], cum, back, trim)
                    b = r["beats"]
                    assert np.array_equal(np.nonzero(beats[i, c, 0])[0], b) and np.array_equal(beats[i, c, 1, :b.size], b), what
                beat_same(beats[i, c], whole["beats"], what + ("beats",))
                beat_same(s2[i, c, 2:], whole["stats"], what + ("stats", s2[i, c], whole["stats"]))
                assert s2[i, c, 0] == np.float32(bpm) and s2[i, c, 1] == period
                beat_same(s0[i, c], [np.float32(bpm), period, 0, -1, -1, whole["stats"][3], -1, n], what + ("stats of mode 0",))
        res[trim] = (beats, s2)
    return res, valid
