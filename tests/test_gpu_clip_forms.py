"""Every launch form of the clip feature kernels on the GPU (k_clip_mel, k_clip_fbank, k_clip_mfcc, k_clip_stft and the second
grid launch of all five feature calls; DESIGN.md section 10, "launch forms").

The shapes are the EDGES tables of tests/clip_*_ref.py -- the geometries whose launch form, LDS layout or lane walk no speech
front end reaches; tests/test_clip_forms_host.py holds their classes without a GPU -- and twelve seeded draws a call
(tests/clip_forms_draws.py).  Every comparison is the one of test_gpu_clip_mel.py, _fbank.py, _mfcc.py and _stft.py, through
the same helpers: the binary64 definition on the product's own decode_clips_audio signal, every value within the derived
binary32 bound, sentinel-filled destinations with guards, `valid` compared, and the worst error / bound over the rows that
hold signal inside (0, 1].  No tolerance is introduced here.  Each device step runs once; the shapes at the plan's exact 64 KB
edge run last in the file."""
import functools
import time

import numpy as np
import pytest

import clip_audio_ref as aref
import clip_fbank_ref as fref
import clip_forms_draws as draws
import clip_gpu as cg
import clip_gpu_calls as calls
import clip_mel_ref as mref
import clip_mfcc_ref as cref
import clip_stft_ref as sref
from clip_gpu import GUARD, SENT

pytestmark = pytest.mark.gpu
NOT_ARGUMENTS = ("stream", "modes", "mode")


def _arguments(e):
    return {k: v for k, v in e.items() if k not in NOT_ARGUMENTS}


def _j(name, rate):
    ix = cg.ref(name)[0]
    return aref.out_length(ix.samples, ix.rate, rate or ix.rate)


def _centred_starts(name, p, f):
    """57, one inside the stream, one whose frames straddle the stream's end (valid is a partial count)"""
    j = _j(name, p["sample_rate"])
    return [57, j // 3 + 11, max(j - (f // 2) * p["hop"] - 3, 0)]


def _whole_frame_starts(name, p, f):
    """the same for the calls that count whole frames only: the straddling clip has f // 2 valid frames"""
    j = _j(name, p["sample_rate"])
    return [57, j // 3 + 11, max(j - p["win_length"] - (f // 2 - 1) * p["hop"] - 1, 0)]


# ---- one call's edge shape, all its modes: (name of the case, frames) -> {label: worst error / bound} ----
def _mel_case(dec, e, kinds=("device",), modes=calls.MEL_MODES, n_clips=3):
    from pdmp3_amd import api
    p, name = _arguments(e), e["stream"]
    tile, _, lds, classes = mref.form(p["n_fft"], p["hop"], p["n_mels"])
    assert api.mel_tile(p["n_fft"], p["hop"], p["n_mels"]) == (tile, (2 - p["hop"]) % 32, lds)
    f = tile + 3
    clips = [(name, s) for s in _centred_starts(name, p, f)[:n_clips]]
    sig = cg.signal(dec, clips, f, p)
    out = {}
    for mode in modes:
        for kind in kinds:
            got, valid = calls.mel_run(dec, kind, clips, f, p, mode)
            worst = calls.mel_check(clips, sig, got, valid, f, p, mode)
            print("mel N %d H %d mels %d C %d (tile %d, LDS %d, %s), mode %s, %s: worst error / bound %.4f over %d clips of %d frames"
                  % (p["n_fft"], p["hop"], p["n_mels"], p["channels"], tile, lds, " ".join(sorted(classes)), mode, kind, worst, len(clips), f))
            assert 0.0 < worst <= 1.0
            out[(mode, kind)] = worst
    if n_clips == 3:
        assert clips[-1][1] + (f - 1) * p["hop"] >= _j(name, p["sample_rate"]) > clips[-1][1]  # (the last clip straddles the end)
    return out


def _fbank_case(dec, e, kinds=("device",), variants=({}, fref.WITH_EVERYTHING), n_clips=3):
    from pdmp3_amd import api
    p0, name = _arguments(e), e["stream"]
    nw, n, hop, nm = p0["win_length"], calls.fbank_n(p0), p0["hop"], p0["num_mel_bins"]
    tile, _, lds, classes = fref.form(nw, n, hop, nm)
    assert api.fbank_tile(nw, n, hop, nm) == (tile, (2 - hop) % 32, lds)
    f = tile + 3
    clips = [(name, s) for s in _whole_frame_starts(name, p0, f)[:n_clips]]
    sig = calls.fbank_signal(dec, clips, f, p0)
    out = {}
    for extra in variants:
        p = dict(p0, **extra)
        for kind in kinds:
            got, valid = calls.fbank_run(dec, kind, clips, f, p)
            worst = calls.fbank_check(clips, sig, got, valid, f, p)
            print("fbank Nw %d N %d H %d mels %d C %d (tile %d, LDS %d, %s), %s, %s: worst error / bound %.4f over %d clips of %d frames"
                  % (nw, n, hop, nm, p["channels"], tile, lds, " ".join(sorted(classes)), "plain" if not extra else "energy mean htk", kind, worst,
                     len(clips), f))
            assert 0.0 < worst <= 1.0
            out[(bool(extra), kind)] = worst
            if n_clips == 3:
                assert 0 < int(valid[-1]) < f
    return out


def _mfcc_case(dec, e, kinds=("device",), n_clips=3):
    from pdmp3_amd import api
    p, name = _arguments(e), e["stream"]
    nw, n, hop, nm, nc = p["win_length"], calls.fbank_n(p), p["hop"], p["num_mel_bins"], p["num_ceps"]
    tile, _, lds, classes = cref.form(nw, n, hop, nm, nc)
    assert api.mfcc_tile(nw, n, hop, nm, nc) == (tile, (2 - hop) % 32, lds)
    f = tile + 3
    clips = [(name, s) for s in _whole_frame_starts(name, p, f)[:n_clips]]
    sig = calls.fbank_signal(dec, clips, f, p)
    out = {}
    for kind in kinds:
        got, valid = calls.mfcc_run(dec, kind, clips, f, p)
        worst = calls.mfcc_check(clips, sig, got, valid, f, p)
        print("mfcc Nw %d N %d H %d mels %d ceps %d C %d (tile %d, LDS %d, %s), %s: worst error / bound %.4f over %d clips of %d frames"
              % (nw, n, hop, nm, nc, p["channels"], tile, lds, " ".join(sorted(classes)), kind, worst, len(clips), f))
        assert 0.0 < worst <= 1.0
        out[kind] = worst
        if n_clips == 3:
            assert 0 < int(valid[-1]) < f
    return out


def _stft_case(dec, e, kinds=("device",), modes=calls.STFT_MODES, n_clips=3):
    from pdmp3_amd import api
    p, name = _arguments(e), e["stream"]
    forms = {m: sref.form(p["n_fft"], p["hop"], sref.MODES[m]) for m in modes}
    f = max(t for t, _, _, _ in forms.values()) + 3                        # (one signal for all modes: the larger tile's frames)
    clips = [(name, s) for s in _centred_starts(name, p, f)[:n_clips]]
    sig = cg.signal(dec, clips, f, p)
    out = {}
    for mode in modes:
        tile, pad, lds, classes = forms[mode]
        assert api.stft_tile(p["n_fft"], p["hop"], mode) == (tile, pad, lds)
        for kind in kinds:
            got, valid = calls.stft_run(dec, kind, clips, f, p, mode)
            worst = calls.stft_check(clips, sig, got, valid, f, p, mode)
            print("stft N %d H %d Nw %s C %d (tile %d, LDS %d, %s), mode %s, %s: worst error / bound %.4f over %d clips of %d frames"
                  % (p["n_fft"], p["hop"], p.get("win_length"), p["channels"], tile, lds, " ".join(sorted(classes)), mode, kind, worst, len(clips), f))
            assert 0.0 < worst <= 1.0
            out[(mode, kind)] = worst
            if n_clips == 3:
                assert 0 < int(valid[-1]) < f                              # (the last clip straddles the end)
    return out


RUNNERS = {"mel": (_mel_case, mref), "fbank": (_fbank_case, fref), "mfcc": (_mfcc_case, cref), "stft": (_stft_case, sref)}
# the case of each call that also runs into a numpy destination
NUMPY_TOO = {"mel": "512-hop2-256-bands", "fbank": "551-hop3-256-bands-hamming", "mfcc": "64-hop64-256-256", "stft": "1024-352-stereo-two-forms"}
EDGE_IDS = [(call, name) for call in ("mel", "fbank", "mfcc", "stft") for name in RUNNERS[call][1].EDGES if name not in RUNNERS[call][1].EXACT_EDGE]
EXACT_IDS = [(call, name) for call in ("mel", "fbank", "mfcc", "stft") for name in RUNNERS[call][1].EXACT_EDGE]


def test_the_tables_are_run_whole():
    for call, (_, module) in RUNNERS.items():
        assert set(n for c, n in EDGE_IDS + EXACT_IDS if c == call) == set(module.EDGES) and NUMPY_TOO[call] in module.EDGES
    assert set(EXACT_IDS) == {("mel", "958-hop4-exactly-64k"), ("fbank", "900-hop4-exactly-64k"), ("fbank", "960-hop4-n-equals-nw-exactly-64k"),
                              ("mfcc", "900-hop4-exactly-64k"), ("mfcc", "960-hop4-n-equals-nw-exactly-64k"), ("stft", "944-hop3-64k")}


@pytest.mark.parametrize("call,name", EDGE_IDS, ids=["%s-%s" % i for i in EDGE_IDS])
def test_edge_shapes_against_binary64_on_the_products_own_signal(call, name):
    run, module = RUNNERS[call]
    dec = cg.decoder()
    try:
        run(dec, module.EDGES[name], ("device", "numpy") if NUMPY_TOO[call] == name else ("device",))
    finally:
        dec.close()


# ---- frames are frames across the edges of a tile of 16 in dynamic LDS ----
def _frames(tile):
    return [0, 1, tile - 1, tile, tile + 1, 2 * tile - 1, 2 * tile]


@pytest.mark.parametrize("call", ["mel", "fbank", "mfcc", "stft"])
def test_frames_are_frames_across_the_edges_of_a_tile_of_16_in_dynamic_lds(call):
    """frame f of a clip at `start` is frame 0 of the clip at start + f H, bit for bit: a frame's values do not depend on its
    place in a tile of mel_tile<1> / fbank_tile<1> / mfcc_tile<1> / stft_tile<1> in dynamic LDS"""
    e = {"mel": mref.EDGES["taco-1024-256-80-stereo"], "fbank": fref.EDGES["taco-1024-256-80-stereo"],
         "mfcc": cref.EDGES["taco-1024-256-80-40-stereo"], "stft": sref.EDGES["1024-700-window-1000"]}[call]
    p, name, start = _arguments(e), e["stream"], 4321
    assert start % p["hop"] != 0
    classes = {"mel": lambda: mref.form(p["n_fft"], p["hop"], p["n_mels"]), "fbank": lambda: fref.form(1024, 1024, p["hop"], 80),
               "mfcc": lambda: cref.form(1024, 1024, p["hop"], 80, 40), "stft": lambda: sref.form(p["n_fft"], p["hop"], 0)}[call]()
    tile = classes[0]
    assert tile == 16 and "tile16-dyn" in classes[3]
    fs = _frames(tile)
    f_long = 2 * tile + 1
    shorts = [(name, start + f * p["hop"]) for f in fs]
    dec = cg.decoder()
    try:
        if call == "mel":
            pairs = [(calls.mel_run(dec, "device", [(name, start)], f_long, p, m)[0], calls.mel_run(dec, "device", shorts, 1, p, m)[0]) for m in calls.MEL_MODES[:3]]
            pick = lambda a, f: a[:, :, f]                                  # [c, n_mels, f]
        elif call == "stft":
            pairs = []
            for m in calls.STFT_MODES[:3]:
                assert sref.form(p["n_fft"], p["hop"], sref.MODES[m])[:1] == (16,)
                pairs.append((calls.stft_run(dec, "device", [(name, start)], f_long, p, m)[0], calls.stft_run(dec, "device", shorts, 1, p, m)[0]))
            pick = lambda a, f: a[:, :, f]                                  # [c, bins, f(, 2)]
        else:
            run = calls.fbank_run if call == "fbank" else calls.mfcc_run
            pairs = [(run(dec, "device", [(name, start)], f_long, p)[0], run(dec, "device", shorts, 1, p)[0])]
            pick = lambda a, f: a[:, f]                                     # [c, f, d]
        for long, short in pairs:
            for i, f in enumerate(fs):
                assert np.array_equal(np.ascontiguousarray(pick(long[0], f)).view(np.uint32), np.ascontiguousarray(pick(short[i], 0)).view(np.uint32)), (call, f)
            assert np.abs(long).sum() > 0 and np.isfinite(long).all()
    finally:
        dec.close()


def test_stft_mode_0_rederives_the_others_across_two_launch_forms():
    """(1024, 352): mode 0 runs stft_tile<1>, modes 1 and 2 stft_tile<2>; Re^2 + Im^2 through the product's own arithmetic on mode
    0's output is mode 2's and its correctly rounded square root mode 1's, bit for bit"""
    e = sref.EDGES["1024-352-stereo-two-forms"]
    p, name = _arguments(e), e["stream"]
    assert [sref.form(1024, 352, m)[0] for m in range(3)] == [16, 32, 32]
    f = 37
    clips = [(name, 4321), (name, 0)]
    dec = cg.decoder()
    try:
        z, _ = calls.stft_run(dec, "device", clips, f, p, "complex")
        power, _ = calls.stft_run(dec, "device", clips, f, p, "power")
        mag, _ = calls.stft_run(dec, "device", clips, f, p, "magnitude")
        want = sref.power_as_the_product(z[..., 0], z[..., 1])
        assert np.array_equal(want.view(np.uint32), power.view(np.uint32))
        assert np.array_equal(np.sqrt(want).view(np.uint32), mag.view(np.uint32))
        assert np.abs(z[..., 1]).sum() > 0 and not np.array_equal(z[..., 0], z[..., 1])
    finally:
        dec.close()


# ---- a seeded sweep a call ----
@pytest.mark.parametrize("call", ["mel", "fbank", "mfcc", "stft"])
def test_a_seeded_sweep(call):
    """twelve geometries drawn with a fixed seed inside the classes the speech shapes do not reach, two clips each; a draw whose
    filterbank holds no bin is skipped and counted: at most 2 of 12"""
    run = RUNNERS[call][0]
    skipped = 0
    dec = cg.decoder()
    try:
        for p in draws.draw(call):
            own = cg.ref(p["stream"])[0].rate
            if call != "stft" and draws.no_band_holds_a_bin(call, p, own):
                skipped += 1
                continue
            if call in ("mel", "stft"):
                run(dec, p, modes=(p["mode"],), n_clips=2)
            elif call == "fbank":
                run(dec, p, variants=({},), n_clips=2)
            else:
                run(dec, p, n_clips=2)
    finally:
        dec.close()
    print("%s: %d of %d draws skipped (no band holds a bin)" % (call, skipped, draws.N_DRAWS))
    assert skipped <= 2


# ---- more clips than one grid: the second launch of every feature call ----
K_GRID, PERIOD, FIRST_GRID, SHIFT = 32768 + 5, 64, 32768, 32
GRID_STREAM = "32k"


def _grid_index(i):
    """which of the 64 starts clip i has: i mod 64 in the first launch, 32 further in the second -- clip 32768 + i is not clip i,
    so a value that came from the first launch's place in a scratch array (row_max, sums) would show"""
    return (i + SHIFT * (i // FIRST_GRID)) % PERIOD


@functools.lru_cache(maxsize=None)
def _audio_grid_wall():
    """the wall time, in this run, of the audio call that test_gpu_clip_audio_paths.py::test_more_clips_than_one_grid makes at the
    own rate: the same clips in a call of its own, not that test's own time (which has its reference in it)"""
    name, t, base = GRID_STREAM, 8, 50000
    offs = (np.arange(K_GRID, dtype=np.int64) * 37) % 4000
    ix = cg.ref(name)[0]
    mp3 = cg.streams()[name]
    dec = cg.decoder()
    try:
        view = cg.destination("device", K_GRID, 1, (t,))[1]
        t0 = time.perf_counter()
        dec.decode_clips_audio([(mp3, ix, int(base + o)) for o in offs], t, 0, 1, out=view)
        return time.perf_counter() - t0
    finally:
        dec.close()


def _grid_starts(ends):
    """64 starts: 5057 + 97 i inside the stream (behind the decoder's quiet onset), and from index 32 on -- the five clips of the
    second launch begin there -- the starts around the stream's end"""
    inside = [5057 + 97 * i for i in range(PERIOD - len(ends))]
    return inside[:SHIFT] + list(ends) + inside[SHIFT:]


def _grid(call, p, f, per, starts, first_rows, valid_of, mode=None):
    """32 768 + 5 clips whose starts repeat with period 64 in one call, into a sentinel-filled device buffer [K, C, per + guard];
    on the device: every row bit-equal to row _grid_index(i) and every guard untouched; rows 0 .. 63 go to the host for
    first_rows(clips, host rows [64, C, per], valid).  The five clips of the second launch have valid 0, 1 (the partial count of
    two frames) and f, and stand where the first launch had clips wholly inside the stream."""
    import torch
    name, c, guard = GRID_STREAM, p["channels"], GUARD
    assert len(starts) == PERIOD
    index = np.array([_grid_index(i) for i in range(K_GRID)])
    assert (index[:PERIOD] == np.arange(PERIOD)).all() and index[FIRST_GRID:].tolist() == list(range(SHIFT, SHIFT + K_GRID - FIRST_GRID))
    clips = [(name, starts[k]) for k in index]
    mp3, ix = cg.streams()[name], cg.ref(name)[0]
    src = [(mp3, ix, s) for _, s in clips]
    dec = cg.decoder()
    t_all = time.perf_counter()
    try:
        big = torch.full((K_GRID, c, per + guard), float(SENT), dtype=torch.float32, device="cuda")
        view = big[:, :, :per]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        kw = dict(mode=mode) if mode else {}
        out, valid = getattr(dec, "decode_clips_" + call)(src, f, out=first_rows.view(view, f), **kw, **p)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        bits = big.view(torch.int32)
        assert bool((bits[:, :, per:] == bits[0, 0, per]).all()) and float(big[0, 0, per]) == float(SENT), "written behind a row's floats"
        rows = bits[:, :, :per]
        same = (rows == rows[:PERIOD][torch.from_numpy(index).to(rows.device)]).flatten(1).all(dim=1).cpu().numpy()
        assert same.all(), "rows %s differ from their rows among 0 .. 63 (the second launch starts at 32768)" % np.flatnonzero(~same)[:8].tolist()
        valid = np.asarray(valid)
        want_valid = np.array([valid_of(s) for s in starts], dtype=valid.dtype)
        assert np.array_equal(valid, want_valid[index])
        counts = {0, 1, f} if f > 1 else {0, 1}
        assert set(want_valid.tolist()) >= counts and set(valid[FIRST_GRID:].tolist()) >= counts         # (in both launches)
        assert (want_valid[index[:K_GRID - FIRST_GRID]] == f).all()          # (the first launch's clips in those places: whole)
        host = big[:PERIOD].cpu().numpy()[:, :, :per]
        assert np.abs(host[want_valid > 0]).sum() > 0
        worst = first_rows.check(dec, clips[:PERIOD], host, valid[:PERIOD], f)
        assert 0.0 < worst <= 1.0
    finally:
        dec.close()
    total = time.perf_counter() - t_all
    audio = _audio_grid_wall()
    print("%s: %d clips of %d frames in one call: %.2f s the call, %.2f s with the checks; the audio call of as many clips of 8 samples: %.2f s "
          "(ratio %.2f); worst error / bound of rows 0 .. 63: %.4f" % (call, K_GRID, f, wall, total, audio, wall / audio, worst))


class _Rows:
    """how a call's destination view is shaped from [K, C, per], and how its first 64 rows are checked"""
    def __init__(self, view, check):
        self.view, self.check = view, check


def test_more_clips_than_one_grid_mel():
    p = dict(sample_rate=0, n_fft=16, hop=16, n_mels=5, scale="slaney", norm="slaney", channels=1)
    f, nm = 2, 5
    j = _j(GRID_STREAM, 0)
    starts = _grid_starts([j - 17, j - 16, j - 1, j, j + 5, j + 1000])

    def check(dec, clips, host, valid, f):
        sig = cg.signal(dec, clips, f, p)
        return calls.mel_check(clips, sig, host.reshape(PERIOD, 1, nm, f), valid, f, p, "whisper")
    _grid("mel", p, f, nm * f, starts, _Rows(lambda v, f: v.unflatten(2, (nm, f)), check), lambda s: mref.valid(j, s, 16, f), mode="whisper")


@pytest.mark.parametrize("call", ["fbank", "mfcc"])
def test_more_clips_than_one_grid_fbank_and_mfcc(call):
    p = dict(sample_rate=0, win_length=16, hop=16, num_mel_bins=5, channels=1, subtract_mean=True, use_energy=True, low_freq=0.0, scale=32768.0)
    if call == "mfcc":
        p["num_ceps"] = 5
    f = 2
    d = 6 if call == "fbank" else 5
    j = _j(GRID_STREAM, 0)
    starts = _grid_starts([j - 33, j - 32, j - 31, j - 16, j - 15, j, j + 1000])

    def check(dec, clips, host, valid, f):
        sig = calls.fbank_signal(dec, clips, f, p)
        return (calls.fbank_check if call == "fbank" else calls.mfcc_check)(clips, sig, host.reshape(PERIOD, 1, f, d), valid, f, p)
    _grid(call, p, f, f * d, starts, _Rows(lambda v, f: v.unflatten(2, (f, d)), check), lambda s: fref.valid(j, s, 16, 16, f))


def test_more_clips_than_one_grid_stft():
    p = dict(sample_rate=0, n_fft=16, hop=16, channels=1)
    f, nb = 2, 9
    j = _j(GRID_STREAM, 0)
    starts = _grid_starts([j - 17, j - 16, j - 1, j, j + 5, j + 1000])

    def check(dec, clips, host, valid, f):
        sig = cg.signal(dec, clips, f, p)
        return calls.stft_check(clips, sig, host.reshape(PERIOD, 1, nb, f, 2), valid, f, p, "complex")
    _grid("stft", p, f, nb * f * 2, starts, _Rows(lambda v, f: v.unflatten(2, (nb, f, 2)), check), lambda s: sref.valid(j, s, 16, f), mode="complex")


def test_more_clips_than_one_grid_stft_long():
    p = dict(sample_rate=0, n_fft=2048, hop=2048, channels=1)
    f, nb = 1, 1025
    j = _j(GRID_STREAM, 0)
    starts = _grid_starts([j - 1, j, j + 5, j + 5000])

    def check(dec, clips, host, valid, f):
        sig = cg.signal(dec, clips, f, p)
        wants = calls.stft_long_wants(clips, sig, f, p)
        return calls.stft_long_check(clips, sig, wants, host.reshape(PERIOD, 1, nb, f), valid, f, p, "power")
    _grid("stft_long", p, f, nb * f, starts, _Rows(lambda v, f: v.unflatten(2, (nb, f)), check), lambda s: sref.valid(j, s, 2048, f), mode="power")


# ---- the plan's exact 64 KB edge: last in the file ----
@pytest.mark.parametrize("call,name", EXACT_IDS, ids=["%s-%s" % i for i in EXACT_IDS])
def test_the_exact_64k_edge_of_the_plan(call, name):
    """a dynamic request of exactly 65 536 B (stft: 65 488 B) -- for the log-mel kernel beside its static `smax`.  A launch the
    runtime refuses is an error return of the call, which the test reports; nothing is tried twice."""
    run, module = RUNNERS[call]
    e = module.EDGES[name]
    dec = cg.decoder()
    try:
        run(dec, e)
    finally:
        dec.close()
