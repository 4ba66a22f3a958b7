"""Chroma features of clips on the GPU (include/pdmp3_bulk.h pdmp3_amd_bulk_decode_clips_chroma, k_clip_chroma; DESIGN.md
section 17).

The reference is made from the product's own signal, as in test_gpu_clip_cqt.py: decode_clips_audio gives the binary32 samples
a clip's frames read, tests/clip_cqt_ref.py evaluates the constant-Q transform on them in binary64 and tests/clip_chroma_ref.py
folds and normalises it; the call's output has to agree within the binary32 bound derived there -- every value of both
quantities and all four norms, none left out; the bound is 0 and the output exactly +0 on silence.  "Same chains" is pinned
apart from that: at chroma_norm None the output is bit-equal to the binary32 sequential fold of decode_clips_cqt's output on
the same clips, and at "l1" and "max" to numpy's binary32 chain and division on that fold.  Destinations are filled with a
sentinel first: nothing outside a row's floats may change.  Each device step runs once.

The LDS of a workgroup, restated from include/pdmp3_bulk.h: the span | the eight waves' partial sums | the q plane
[n_bins rounded up to 16][17]; the folded classes [n_chroma][17] lie over the partial sums."""
import numpy as np
import pytest

import clip_audio_ref as aref
import clip_chroma_ref as ref
import clip_cqt_ref as cref
import clip_forms_cases as cases
import clip_gpu as cg
import clip_gpu_calls as calls
import clip_streams
from clip_gpu import GUARD, SENT
from clip_streams import ISO_LSF

pytestmark = pytest.mark.gpu
U = ref.U
C1, C3 = ref.FMIN_C1, ref.FMIN_C3
QUANTITIES = ["magnitude", "power"]
NORMS = [None, "l1", "l2", "max"]
FOLD = ("n_chroma", "base_class")

# (a) the default spec, stereo: the static kernel, split and unsplit tiles; (b) the dynamic path; (c) 36 bins an octave from C3,
# r = 3: bin 0 and bin 107 land in other classes than k // 3 gives, base_class 0 and 5; (d) 17 bins at 12 an octave at the
# stream's own rate: classes of two bins and of one; (e) tiles of 8 and of 4 frames, the hops from the plan's restatement (at
# the second the constant-Q call itself would still take 8 frames)
PA = dict(sample_rate=22050, hop=512, channels=2, fmin=C1, n_bins=84, bins_per_octave=12, n_chroma=12, base_class=0)
PB = dict(sample_rate=16000, hop=160, channels=1, fmin=1000.0, n_bins=24, bins_per_octave=12, n_chroma=12, base_class=7, norm=2, scale=2)
PC = dict(sample_rate=22050, hop=512, channels=1, fmin=C3, n_bins=108, bins_per_octave=36, n_chroma=12, base_class=0)
PC5 = dict(PC, base_class=5)
PD = dict(sample_rate=0, hop=160, channels=1, fmin=1000.0, n_bins=17, bins_per_octave=12, n_chroma=12, base_class=0, norm=1, scale=0)
PE = dict(sample_rate=0, channels=1, fmin=C1, n_bins=24, bins_per_octave=12, n_chroma=12, base_class=3)
# the many clips: 6 bins at 3 an octave from 500 Hz at 8 kHz, filters of 61 taps, hop 1
PM = dict(sample_rate=0, hop=1, channels=1, fmin=500.0, n_bins=6, bins_per_octave=3, n_chroma=3, base_class=1)


def _hop_for(tile, sr=44100):
    """the smallest multiple of 64 at which the plan of (e) at 44.1 kHz takes `tile` frames"""
    return next(h for h in range(64, 8193, 64) if ref.plan(sr, h, **calls.cqt_shape(PE))[0] == tile)


PE8, PE4 = dict(PE, hop=_hop_for(8)), dict(PE, hop=_hop_for(4))


def _cqt_args(p):
    return {k: v for k, v in p.items() if k not in FOLD}


def _run(dec, kind, clips, f, p, quantity, norm, floor=1e-10):
    """clips: (stream name, start) -> (host copy [k, c, n_chroma, f], valid)"""
    return cg.run(dec, "decode_clips_chroma", kind, clips, f, p["channels"], (p["n_chroma"], f), quantity=quantity, chroma_norm=norm, norm_floor=floor, **p)


def _reference(dec, clips, f, p):
    """per clip and quantity the constant-Q transform of the product's own signal in binary64 with its bounds -- computed once a
    case and left unchanged"""
    sig = calls.cqt_signal(dec, clips, f, p)
    out = []
    for (n, s), (s0, y) in zip(clips, sig):
        rate = cg.rate(p, n)
        out.append({q: cref.cqt(y, s0, s, f, rate, p["hop"], cref.MODES[q], **calls.cqt_geo(p)) for q in QUANTITIES} | {"signal": float(np.abs(y).sum())})
    return out


def _check(clips, refs, got, valid, f, p, quantity, norm, floor=1e-10):
    """every row against the definition; -> worst error / bound over the rows that hold signal"""
    worst = 0.0
    for i, (n, s) in enumerate(clips):
        ix = cg.ref(n)[0]
        j_all = aref.out_length(ix.samples, ix.rate, cg.rate(p, n))
        assert int(valid[i]) == ref.valid(j_all, s, p["hop"], f), (n, s, valid[i])
        want, bound = ref.from_cqt(*refs[i][quantity], p["bins_per_octave"], p["n_chroma"], p["base_class"], ref.NORMS[norm], floor)
        assert want.shape == got[i].shape
        err = np.abs(got[i].astype(np.float64) - want)
        assert (err <= bound).all(), "%s at %d, %s / %s: error beyond the bound by %g at %s" % (
            n, s, quantity, norm, float((err - bound).max()), np.unravel_index(np.argmax(err - bound), err.shape))
        nz = bound > 0
        assert (got[i][~nz] == 0.0).all() and not np.signbit(got[i][~nz]).any()
        if refs[i]["signal"] > 0 and nz.any():
            r = float((err[nz] / bound[nz]).max())
            assert 0.0 < r <= 1.0, (n, s, quantity, norm, r)
            worst = max(worst, r)
    return worst


CASES = {
    # the spec, the streams, n_frames, the launch path, split tiles, tiles
    "a-default-stereo": (PA, ["22k", "48k", "mixed/mono-stereo"], 40, "tile16-static", 4, 6),
    "b-16k-24-bins-dynamic": (PB, ["32k", "16k-mono"], 37, "tile16-dyn", 0, 2),
    "c-36-an-octave-base-0": (PC, ["22k"], 35, "tile16-static", 7, 7),
    "c-36-an-octave-base-5": (PC5, ["48k"], 19, "tile16-static", 7, 7),
    "d-17-bins-own-rate": (PD, ["16k-mono"], 41, "tile16-dyn", 0, 2),
    "e-44k-tile-8": (PE8, ["44k-mono"], 11, "tile8-static", 2, 2),
    "e-44k-tile-4": (PE4, ["44k-mono"], 7, "tile4-static", 2, 2),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_against_binary64_and_against_the_fold_of_the_cqt_call(case):
    from pdmp3_amd import api
    p, names, f, path, n_split, n_tiles = CASES[case]
    rate = cg.rate(p, names[0])
    assert all(cg.rate(p, n) == rate for n in names)
    # the launch path and the tile, from the plan function and from its restatement
    plan = api.chroma_plan(rate, hop=p["hop"], n_chroma=p["n_chroma"], base_class=p["base_class"], **calls.cqt_shape(p))
    want = ref.plan(rate, p["hop"], **calls.cqt_shape(p))
    assert plan == want[:8] and want[8] == path and plan[5] == n_split and (p["n_bins"] + 15) // 16 == n_tiles
    tile = plan[0]
    assert f > tile                                                          # (a tile edge inside the clip)
    if case == "e-44k-tile-4":
        assert api.cqt_plan(rate, hop=p["hop"], **calls.cqt_shape(p))[0] == 8     # (the q plane costs this spec a tile size)
    cls, count = ref.class_map(p["n_bins"], p["bins_per_octave"], p["n_chroma"], p["base_class"])
    if case[0] == "c":
        assert cls[0] == cls[1] == p["base_class"] and cls[2] == p["base_class"] + 1 and cls[107] == p["base_class"] and list(count) == [9] * 12
    if case[0] == "d":
        assert sorted(set(count)) == [1, 2]
    clips = [(n, s) for n in names for s in calls.centred_starts(n, p, f)]
    dec = cg.decoder()
    try:
        refs = _reference(dec, clips, f, p)
        for quantity in QUANTITIES:
            q32, qv = calls.cqt_run(dec, "device", clips, f, _cqt_args(p), quantity)
            folded = ref.fold32(q32, cls, p["n_chroma"])
            for norm in NORMS:
                floor = 1e-10 if norm != "l1" else 0.5       # (L1 against a floor that some frames' sums reach and some do not)
                for kind in ("device", "numpy") if (quantity, norm) in (("magnitude", "max"), ("power", None)) else ("device",):
                    got, valid = _run(dec, kind, clips, f, p, quantity, norm, floor)
                    assert np.array_equal(valid, qv)
                    if norm is None:
                        assert np.array_equal(got.view(np.uint32), folded.view(np.uint32)), "not the fold of decode_clips_cqt's output"
                    elif norm != "l2":
                        assert np.array_equal(got.view(np.uint32), ref.normalise32(folded, ref.NORMS[norm], floor).view(np.uint32))
                    worst = _check(clips, refs, got, valid, f, p, quantity, norm, floor)
                    print("%s (tile %d, %s, %d of %d tiles split), %s / %s, %s: worst error / bound %.6f over %d clips of %d frames"
                          % (case, tile, path, n_split, n_tiles, quantity, norm, kind, worst, len(clips), f))
                    assert 0.0 < worst <= 1.0
                    if norm == "max":
                        full = got.max(axis=2)
                        assert (full <= 1.0).all() and (full == 1.0).any()      # (below 1 only where d < floor: a frame's faint tail)
    finally:
        dec.close()


def test_clips_wholly_behind_the_end_are_exactly_zero():
    p, f, name = PB, 18, "32k"
    ix = cg.ref(name)[0]
    j_all = aref.out_length(ix.samples, ix.rate, 16000)
    h0 = int(cref.lengths(16000, **calls.cqt_shape(p))[2][0])
    dec = cg.decoder()
    try:
        stats = dec.clip_stats()
        clips = [(name, j_all + h0), (name, j_all + 10 ** 6), (name, 2 ** 40)]
        for quantity in QUANTITIES:
            for norm in NORMS:
                got, valid = _run(dec, "device", clips, f, p, quantity, norm)
                assert list(valid) == [0, 0, 0] and (got == 0.0).all() and not np.signbit(got).any()
        assert dec.clip_stats() == stats
    finally:
        dec.close()


def test_frames_are_frames_and_slices_of_a_batch_are_slices():
    """(a): frame f of a clip at `start` is frame 0 of a clip at start + f H, bit for bit, on both sides of the kernel's tile
    edge; a clip's row does not depend on the batch around it"""
    from pdmp3_amd import api
    p = dict(PA, channels=1)
    name, start = "48k", 4321
    tile = api.chroma_plan(22050, hop=p["hop"], **calls.cqt_shape(p))[0]
    dec = cg.decoder()
    try:
        fs = [0, 1, tile - 1, tile, tile + 1, tile + 4]
        for norm in ("l2", "max"):
            long, _ = _run(dec, "device", [(name, start)], tile + 6, p, "magnitude", norm)
            batch = [(name, start + f * p["hop"]) for f in fs]
            short, _ = _run(dec, "device", batch, 2, p, "magnitude", norm)
            for i, f in enumerate(fs):
                assert np.array_equal(long[0, :, :, f].view(np.uint32), short[i, :, :, 0].view(np.uint32)), (norm, f)
                assert np.array_equal(long[0, :, :, f + 1].view(np.uint32), short[i, :, :, 1].view(np.uint32)), (norm, f)
            assert np.abs(long).sum() > 0
            mixed, _ = _run(dec, "device", [("22k", 999), batch[4], batch[1]], 2, p, "magnitude", norm)
            assert np.array_equal(mixed[1].view(np.uint32), short[4].view(np.uint32)) and np.array_equal(mixed[2].view(np.uint32), short[1].view(np.uint32))
    finally:
        dec.close()


def test_a_refused_clip_in_the_middle_of_a_batch_and_bad_arguments():
    from pdmp3_amd import api
    p, f = PB, 19
    nc = p["n_chroma"]
    bad = clip_streams.replay_stream()
    bix = api.StreamIndex(bad, ISO_LSF)
    assert bix.replay
    mix = cg.ref("mixed/mpeg1-lsf")[0]
    assert not mix.one_format
    s = cg.streams()
    good = [("48k", 100), ("22k", 3000)]
    dec = cg.decoder()
    try:
        refs = _reference(dec, good, f, p)
        per = nc * f
        for kind, norm in (("device", "max"), ("numpy", "l2")):
            for mid, exc, code in (((s["mixed/mpeg1-lsf"], mix, 0), api.MixedFormat, -3), ((bad, bix, 10), api.RingReplay, -2)):
                big, view = cg.destination(kind, 3, 1, (nc, f))
                src = [(s["48k"], cg.ref("48k")[0], 100), mid, (s["22k"], cg.ref("22k")[0], 3000)]
                with pytest.raises(exc) as e:
                    dec.decode_clips_chroma(src, f, chroma_norm=norm, out=view, **p)
                host = cg.host(big).reshape(3, 1, per + GUARD)
                assert e.value.valid[1] == code and (host[1] == SENT).all()
                assert (host[:, :, per:] == SENT).all()
                got = host[[0, 2], :, :per].reshape(2, 1, nc, f)
                assert 0.0 < _check(good, refs, got, e.value.valid[[0, 2]], f, p, "magnitude", norm) <= 1.0
        # bad arguments: nothing is written
        big, view = cg.destination("device", 1, 1, (nc, f))
        src = [(s["48k"], cg.ref("48k")[0], 0)]
        for bad_p in (dict(n_chroma=0), dict(n_chroma=5), dict(n_chroma=24), dict(base_class=12), dict(base_class=-1), dict(chroma_norm=4),
                      dict(chroma_norm="l3"), dict(norm_floor=0.0), dict(norm_floor=1e-46), dict(norm_floor=float("nan")), dict(quantity="complex"),
                      dict(quantity="log10"), dict(hop=0), dict(fmin=0.0), dict(fmin=7600.0), dict(bins_per_octave=0), dict(norm=3), dict(width=65)):
            args = dict(p, **bad_p)
            out = view if args["n_chroma"] == nc else None
            with pytest.raises(RuntimeError):
                dec.decode_clips_chroma(src, f, out=out, **args)
            assert (cg.host(big) == SENT).all(), bad_p
        with pytest.raises(RuntimeError):
            dec.decode_clips_chroma([(s["48k"], cg.ref("48k")[0], -1)], f, out=view, **p)
        with pytest.raises(RuntimeError):            # (rate 0 and clips of different rates)
            dec.decode_clips_chroma(src + [(s["32k"], cg.ref("32k")[0], 0)], f, **dict(p, sample_rate=0))
        assert (cg.host(big) == SENT).all()
    finally:
        dec.close()
        bix.close()


def test_more_clips_than_one_grid():
    """32 768 + 5 clips in one call: pdmp3_hip_clip_chroma launches the kernel twice (a grid's y extent), the second time from
    descriptor 32 768 on.  Sixty-four distinct clips are held against the definition, every row is bit-equal to its twin among
    them; the last five are other clips than rows 0 .. 4, one of them behind the end"""
    name, k, f, p = "8k", 32768 + 5, 40, PM
    ix = cg.ref(name)[0]
    assert ix.rate == 8000
    j_all = aref.out_length(ix.samples, ix.rate, ix.rate)
    h0 = int(cref.lengths(8000, **calls.cqt_shape(p))[2][0])
    starts = [1000 + 3001 * i for i in range(62)] + [j_all + h0 + 9, j_all - 5]
    assert starts[61] + f + h0 + 16 < j_all
    twin = (np.arange(k, dtype=np.int64) * 7) % 62
    twin[32768:] = [62, 63, 61, 60, 59]
    assert not np.any(twin[32768:] == twin[:5])
    mp3 = cg.streams()[name]
    dec = cg.decoder()
    try:
        first = [(name, s) for s in starts]
        refs = _reference(dec, first, f, p)
        base, valid64 = _run(dec, "device", first, f, p, "magnitude", "max")
        assert 0.0 < _check(first, refs, base, valid64, f, p, "magnitude", "max") <= 1.0
        assert list(valid64[61:]) == [f, 0, 5] and (base[62] == 0.0).all()
        nc = p["n_chroma"]
        big, view = cg.destination("device", k, 1, (nc, f))
        out, valid = dec.decode_clips_chroma([(mp3, ix, int(starts[t])) for t in twin], f, out=view, **p)
        per = nc * f
        host = cg.host(big).reshape(k, per + GUARD)
        assert (host[:, per:] == SENT).all(), "written behind a row's floats"
        assert np.array_equal(valid, valid64[twin]) and list(valid[32768:]) == [0, 5, f, f, f]
        same = (host[:, :per].view(np.uint32) == base[twin].reshape(k, per).view(np.uint32)).all(axis=1)
        bad = np.flatnonzero(~same)
        assert bad.size == 0, "%d rows differ from their twins, %d of them in the second launch: %s" % (bad.size, int((bad >= 32768).sum()), bad[:8].tolist())
        assert np.unique(base[:62, 0, 0, 0]).size > 8
    finally:
        dec.close()


def test_one_decoder_through_this_call_the_cqt_call_and_the_mel_call_twice():
    """this call, decode_clips_cqt at the same geometry (one table for both) and at more geometries than the decoder keeps
    tables, decode_clips_mel, this call with other fold arguments -- and all of it again: every call is bit-equal to its first
    answer"""
    small = [("48k", 500), ("22k", 1234)]
    dec = cg.decoder()
    try:
        def round_():
            out = []
            out.append(_run(dec, "device", small, 9, PB, "magnitude", "max"))
            out.append(calls.cqt_run(dec, "device", small, 9, _cqt_args(PB), "magnitude"))
            for i in range(5):                                                   # (more tables than the decoder keeps)
                out.append(calls.cqt_run(dec, "device", small, 3, dict(_cqt_args(PB), fmin=1000.0 + 10.0 * i), "power"))
                out.append(_run(dec, "device", small, 3, dict(PB, fmin=1005.0 + 10.0 * i), "power", "l1"))
            out.append(calls.mel_run(dec, "device", small, 9, cases.MEL_P16, "log10"))
            out.append(_run(dec, "device", small, 9, dict(PB, n_chroma=6, base_class=2), "magnitude", "l2"))
            out.append(_run(dec, "numpy", small, 9, PB, "magnitude", "max"))
            return [(cg.host(a), v) for a, v in out]
        one, two = round_(), round_()
        assert len(one) == len(two)
        for (a, va), (b, vb) in zip(one, two):
            a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
            assert a.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
            assert np.array_equal(va, vb)
        assert np.array_equal(one[0][0].view(np.uint32), one[-1][0].view(np.uint32))        # (device and numpy destinations)
        # after all the calls the first answer is still the fold of the constant-Q call's
        cls, _ = ref.class_map(PB["n_bins"], 12, 12, PB["base_class"])
        want = ref.normalise32(ref.fold32(two[1][0], cls, 12), 3, 1e-10)
        assert np.array_equal(two[0][0].view(np.uint32), want.view(np.uint32)) and np.abs(want).sum() > 0
    finally:
        dec.close()


def test_return_types_and_empty_calls():
    import torch
    src = [(cg.streams()["22k"], cg.ref("22k")[0], 1000)]
    dec = cg.decoder()
    try:
        out, valid = dec.decode_clips_chroma(src, 17)          # the defaults: 22 050 Hz, C1, 84 bins, 12 classes, magnitudes, max; the stream's channels
        assert tuple(out.shape) == (1, 2, 12, 17) and out.is_cuda and out.dtype == torch.float32 and valid[0] == 17
        plain, _ = _run(dec, "device", [("22k", 1000)], 17, PA, "magnitude", "max")
        assert np.array_equal(cg.host(out).view(np.uint32), plain.view(np.uint32)) and (plain.max(axis=2) == 1.0).all()
        out, valid = dec.decode_clips_chroma([], 10, channels=1)
        assert tuple(out.shape) == (0, 1, 12, 10) and valid.size == 0
        out, valid = dec.decode_clips_chroma(src, 0, n_chroma=6, channels=1)
        assert tuple(out.shape) == (1, 1, 6, 0) and valid[0] == 0
    finally:
        dec.close()
