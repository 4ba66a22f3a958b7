"""MFCC, deltas and dB mel of clips at n_fft 2048 / 4096 on the device: decode_clips_mfcc_long's two modes.
"db" is numpy float32 arithmetic on decode_clips_mel_long's own values, bit for bit; the cepstra are held against the binary64
DCT on the call's own dB values, the deltas against the binary64 stencil on the call's own cepstra of the widened clip and
against the full chain from the widened clip's log-mel, every value within its derived bound (tests/clip_mfcc_long_ref.py); slices
of a longer clip bit for bit; determinism, batches, refusals, more clips than one grid, destinations, types and empty calls.

Measured on an MI355X (worst error / bound, printed by the tests): see profiles/clip_mfcc_long_tests.txt."""
import numpy as np
import pytest

import clip_gpu as cg
import clip_mfcc_long_ref as ref
import clip_streams
from clip_gpu import GUARD, SENT
from clip_streams import ISO_LSF

pytestmark = pytest.mark.gpu
AMIN = 1e-10
# the defaults, spelled out
P0 = dict(sample_rate=22050, n_fft=2048, hop=512, n_mels=128, n_mfcc=20, lifter=0.0, top_db=80.0, amin=AMIN, deltas=0, delta_width=9, channels=1)
MEL_KEYS = ("sample_rate", "n_fft", "hop", "n_mels", "channels")


def _rows(p, mode):
    return p["n_mels"] if mode == "db" else (1 + p["deltas"]) * p["n_mfcc"]


def _run(dec, kind, clips, f, p, mode="mfcc", **kw):
    """clips: (stream name, start) -> (host copy [k, c, rows, f], valid); the guard floats behind every row are looked at"""
    q = dict(p, **kw)
    return cg.run(dec, "decode_clips_mfcc_long", kind, clips, f, q["channels"], (_rows(q, mode), f), out_mode=mode, **q)


def _mel(dec, clips, f, p):
    """decode_clips_mel_long's log10 values of the clips -> [k, c, n_mels, f]"""
    out, valid = dec.decode_clips_mel_long(cg.src(clips), f, mode="log10", floor=p["amin"], **{a: p[a] for a in MEL_KEYS})
    return cg.host(out)


def _valid(clips, valid, f, p):
    for i, (name, s) in enumerate(clips):
        assert int(valid[i]) == ref.valid(cg.j_all(p, name), s, p["hop"], f), (name, s, valid[i])


def _four(p, name, f, h=0):
    """a stream's start (the first frame's window reaches in front of sample 0), its middle, over its end, wholly behind it"""
    j_all, hop = cg.j_all(p, name), p["hop"]
    return [(name, h * hop + (100 if h else 0)), (name, 40000 + f), (name, j_all - 3 * hop), (name, j_all + p["n_fft"] + (h + 3) * hop)]


# ---- 1. "db": binary32 arithmetic on the log-mel call's own values, bit for bit ----
@pytest.mark.parametrize("n_mels,channels", [(40, 1), (128, 1), (40, 2), (128, 2)])
def test_db_is_float32_arithmetic_on_the_log_mel_calls_values_bit_for_bit(n_mels, channels):
    name = "48k" if channels == 2 else "44k-mono"
    p = dict(P0, n_mels=n_mels, channels=channels, sample_rate=0 if channels == 2 else 22050)
    f = 69                                               # (one tile of 64 frames and five more)
    clips = _four(p, name, f)
    dec = cg.decoder()
    try:
        l = _mel(dec, clips, f, p)
        floor_db = np.float32(10.0) * l[3, 0, 0, 0]
        assert (l[3] == l[3, 0, 0, 0]).all() and abs(float(floor_db) + 100.0) < 1e-4      # (behind the end: 10 log10 amin everywhere)
        for top in (80.0, 20.0, None):
            for kind in ("device", "numpy") if top == 20.0 else ("device",):
                got, valid = _run(dec, kind, clips, f, p, "db", top_db=top)
                _valid(clips, valid, f, p)
                assert valid[0] == f and 0 < valid[2] < f and valid[3] == 0
                for i in range(len(clips)):
                    for c in range(channels):
                        want = ref.db(l[i, c], top)
                        assert np.array_equal(cg.bits(got[i, c]), cg.bits(want)), (n_mels, channels, top, kind, i, c)
                assert (got[3] == floor_db).all()
                if top == 20.0:
                    for c in range(channels):
                        thr = got[1, c].max() - np.float32(20.0)
                        assert (got[1, c] == thr).any() and (got[1, c] > thr).any() and (np.float32(10.0) * l[1, c] < thr).any()
                    if channels == 2:                     # (one maximum per channel, not one per clip)
                        assert got[1, 0].max() != got[1, 1].max() and got[1, 0].min() != got[1, 1].min()
    finally:
        dec.close()


# ---- 2. the cepstra against the binary64 DCT on the call's own dB values ----
CEPS_CASES = {"40-13": dict(n_mels=40, n_mfcc=13), "128-20": dict(n_mels=128, n_mfcc=20), "20-20": dict(n_mels=20, n_mfcc=20),
              "256-128": dict(n_mels=256, n_mfcc=128), "128-20-4096": dict(n_mels=128, n_mfcc=20, n_fft=4096, hop=1024)}


@pytest.mark.parametrize("case", sorted(CEPS_CASES))
def test_cepstra_against_the_binary64_dct_on_the_db_modes_values(case):
    name = "44k-mono"
    p = dict(P0, **CEPS_CASES[case])
    nm, nc = p["n_mels"], p["n_mfcc"]
    dec = cg.decoder()
    try:
        worst = 0.0
        for f in (5, 69, 133):
            clips = _four(p, name, f)
            d, _ = _run(dec, "device", clips, f, p, "db")
            for lifter in (0.0, 22.0):
                got, valid = _run(dec, "device", clips, f, p, lifter=lifter)
                _valid(clips, valid, f, p)
                for i in range(len(clips)):
                    want, bound = ref.cepstra(d[i, 0], nc, lifter)
                    err = np.abs(got[i, 0].astype(np.float64) - want)
                    assert (err <= bound).all(), (case, f, lifter, i, float((err / bound).max()), np.unravel_index(np.argmax(err / bound), err.shape))
                    worst = max(worst, float((err / bound).max()))
                # behind the stream d is 10 log10 amin in every band: c[0] = d sqrt(n_mels) (times the lifter's factor), the rest 0
                lift0 = 1.0 + (lifter / 2.0) * np.sin(np.pi / lifter) if lifter else 1.0
                flat, bflat = float(d[3, 0, 0, 0]) * np.sqrt(nm) * lift0, ref.cepstra(d[3, 0], nc, lifter)[1]
                assert (np.abs(got[3, 0, 0].astype(np.float64) - flat) <= bflat[0] + abs(flat) * 4 * ref.U64).all()
                assert (np.abs(got[3, 0, 1:].astype(np.float64)) <= bflat[1:] + abs(flat) * 4 * nm * ref.U64).all()
        print("%s: worst error / bound %.4f" % (case, worst))
        assert 0.0 < worst <= 1.0
    finally:
        dec.close()


# ---- 3. the deltas against the binary64 stencil on the call's own cepstra of the widened clip ----
@pytest.mark.parametrize("w", [3, 9, 17])
def test_deltas_against_the_stencil_on_the_cepstra_of_the_widened_clip(w):
    name, f, h = "44k-mono", 69, (w - 1) // 2
    p = dict(P0, n_mels=40, n_mfcc=13, top_db=None, delta_width=w, lifter=22.0)
    hop, nc = p["hop"], p["n_mfcc"]
    clips = _four(p, name, f, h)
    assert clips[0][1] - h * hop < p["n_fft"] // 2 and clips[2][1] + (f - 1 + h) * hop > cg.j_all(p, name)
    dec = cg.decoder()
    try:
        wide, _ = _run(dec, "device", [(n, s - h * hop) for n, s in clips], f + 2 * h, p)
        plain, _ = _run(dec, "device", clips, f, p)
        worst = 0.0
        for deltas in (1, 2):
            got, valid = _run(dec, "device", clips, f, p, deltas=deltas)
            _valid(clips, valid, f, p)
            assert np.array_equal(cg.bits(got[:, :, :nc]), cg.bits(plain))
            for i in range(len(clips)):
                assert np.array_equal(cg.bits(wide[i, 0][:, h:h + f]), cg.bits(plain[i, 0]))
                for order in range(1, deltas + 1):
                    want, mass = ref.delta(wide[i, 0], w, order)
                    bound = ref.delta_bound(want, mass, w)
                    err = np.abs(got[i, 0, order * nc:(order + 1) * nc].astype(np.float64) - want)
                    assert (err <= bound).all(), (w, deltas, i, order, float((err / bound).max()))
                    worst = max(worst, float((err / bound).max()))
            # behind the end c is constant in time: the deltas are what the binary64 chain's roundings leave of 0
            assert (np.abs(got[3, 0, nc:]) <= 1e-12 * np.abs(plain[3, 0]).max()).all() and (np.abs(got[1, 0, nc:]) > 1e-6).mean() > 0.9
        # frames centred in front of sample 0: at hop = n_fft / 2 those of a clip at sample 0 read nothing of the stream, so their
        # log-mel is the floor's, the value the log-mel call gives behind the end; the full chain from the log-mel
        p2 = dict(p, hop=p["n_fft"] // 2)
        floor = _mel(dec, clips[3:], 1, p2)[0, 0, 0, 0]
        l = np.concatenate([np.full((1, 40, h), floor, dtype=np.float32), _mel(dec, [(name, 0)], f + h, p2)[0]], axis=2)
        got, _ = _run(dec, "device", [(name, 0)], f, p2, deltas=2)
        want, bound = ref.mfcc(l[0], nc, 22.0, None, 2, w, f)
        err = np.abs(got[0, 0].astype(np.float64) - want)
        assert (err <= bound).all(), (w, float((err / bound).max()))
        print("width %d: worst error / bound %.4f (the stencil alone), %.4f (a clip at sample 0, the full chain)"
              % (w, worst, float((err / bound).max())))
        assert 0.0 < worst <= 1.0
    finally:
        dec.close()


# ---- 4. the full chain with top_db: the threshold comes from the clip's own frames ----
def test_the_full_chain_with_top_db_and_a_loudest_frame_in_the_halo():
    name, f, w, h = "44k-mono", 5, 9, 4
    p = dict(P0, n_mels=40, n_mfcc=13, deltas=2)
    hop, nc = p["hop"], p["n_mfcc"]
    dec = cg.decoder()
    try:
        # a frame that is louder than the f frames behind it
        base, n_scan = 30000, 300
        scan = (np.float32(10.0) * _mel(dec, [(name, base)], n_scan, p)[0, 0]).max(axis=0)
        found = [t for t in range(h, n_scan - f) if scan[t - h:t].max() > scan[t:t + f].max() + 0.25]
        assert found, "no clip of this stream has its loudest frame in the halo"
        t = found[0]
        clips = [(name, base + t * hop), (name, 40000), (name, cg.j_all(p, name) - 2 * hop)]
        l = _mel(dec, [(n, s - h * hop) for n, s in clips], f + 2 * h, p)
        own, halo_max = (np.float32(10.0) * l[0, 0][:, h:h + f]).max(), (np.float32(10.0) * l[0, 0]).max()
        assert halo_max > own + 0.25
        worst = 0.0
        for top in (80.0, 20.0):
            got, valid = _run(dec, "device", clips, f, p, top_db=top)
            _valid(clips, valid, f, p)
            for i in range(len(clips)):
                want, bound = ref.mfcc(l[i, 0], nc, 0.0, top, 2, w, f)
                err = np.abs(got[i, 0].astype(np.float64) - want)
                assert (err <= bound).all(), (top, i, float((err / bound).max()), np.unravel_index(np.argmax(err / bound), err.shape))
                worst = max(worst, float((err / bound).max()))
        # at 20 dB the clamp is at work, and the halo's maximum would have given other cepstra
        d = ref.db(l[0, 0], 20.0, h)
        assert (d[:, h:h + f] == own - np.float32(20.0)).any()
        other = ref.cepstra(np.maximum(np.float32(10.0) * l[0, 0], halo_max - np.float32(20.0)), nc)[0][:, h:h + f]
        want, bound = ref.mfcc(l[0, 0], nc, 0.0, 20.0, 2, w, f)
        assert (np.abs(other - want[:nc]) > 2 * bound[:nc]).any() and (np.abs(got[0, 0, :nc] - want[:nc]) <= bound[:nc]).all()
        print("full chain, deltas 2, top_db 80 and 20: worst error / bound %.4f; the halo's loudest frame lies %.2f dB above the clip's own" % (worst, halo_max - own))
        assert 0.0 < worst <= 1.0
    finally:
        dec.close()


# ---- 5. slices ----
def test_a_clip_is_the_slice_of_a_longer_one():
    """at top_db None the clip (s, F) is columns a .. of the clip (s - a H, F + a), bit for bit, in both modes and with deltas"""
    name, f = "44k-mono", 13
    p = dict(P0, n_mels=40, n_mfcc=13, top_db=None)
    hop = p["hop"]
    dec = cg.decoder()
    try:
        for s, a in ((20000, 1), (20000, 9), (64 * hop + 77, 64)):
            short, long = [(name, s)], [(name, s - a * hop)]
            for mode, deltas in (("db", 0), ("mfcc", 0), ("mfcc", 2)):
                x, _ = _run(dec, "device", short, f, p, mode, deltas=deltas)
                y, _ = _run(dec, "device", long, f + a, p, mode, deltas=deltas)
                assert np.array_equal(cg.bits(x), cg.bits(y[..., a:])), (mode, deltas, s, a)
                assert np.abs(x).min() > 0
    finally:
        dec.close()


# ---- 6. plumbing ----
def test_twice_the_same_alone_as_in_a_batch_and_the_stage_is_shared():
    p = dict(P0, channels=2, n_mels=40, n_mfcc=13, deltas=2, sample_rate=0)
    f = 9
    batch = [("48k", s) for s in (70000, 100000, 69632, 123456, 90000)]
    tp = dict(sample_rate=0, n_fft=2048, hop=512, n_mels=40, channels=2)
    dec = cg.decoder()
    try:
        for mode in ref.MODES:
            t0, _ = dec.decode_clips_tempogram(cg.src(batch), f, out_mode="onset", **tp)
            t0 = cg.host(t0).copy()
            m0 = _mel(dec, batch, f, p).copy()
            a, va = _run(dec, "device", batch, f, p, mode)
            t1, _ = dec.decode_clips_tempogram(cg.src(batch), f, out_mode="onset", **tp)
            assert np.array_equal(cg.bits(t0), cg.bits(cg.host(t1))) and np.array_equal(cg.bits(m0), cg.bits(_mel(dec, batch, f, p)))
            b, vb = _run(dec, "device", batch, f, p, mode)
            assert np.array_equal(cg.bits(a), cg.bits(b)) and np.array_equal(va, vb)
            for i in (0, 2, 4):
                one, v1 = _run(dec, "device", [batch[i]], f, p, mode)
                assert np.array_equal(cg.bits(one[0]), cg.bits(a[i])) and v1[0] == va[i]
            assert np.unique(a[:, 0, 3, 3]).size == 5 and np.unique(a[:, 1, 3, 3]).size == 5
    finally:
        dec.close()


def test_a_refused_clip_in_the_middle_of_a_batch_and_bad_arguments():
    from pdmp3_amd import api
    p = dict(P0, n_mels=40, n_mfcc=13, deltas=1, delta_width=3)
    f = 9
    bad = clip_streams.replay_stream()
    bix = api.StreamIndex(bad, ISO_LSF)
    assert bix.replay
    mix = cg.ref("mixed/mpeg1-lsf")[0]
    assert not mix.one_format
    s = cg.streams()
    good = [("48k", 9000), ("22k", 30000)]
    dec = cg.decoder()
    try:
        for kind, mode in (("device", "mfcc"), ("numpy", "db"), ("numpy", "mfcc")):
            want, valid = _run(dec, "device", good, f, p, mode)
            rows = _rows(p, mode)
            per = rows * f
            for mid, exc, code in (((s["mixed/mpeg1-lsf"], mix, 0), api.MixedFormat, -3), ((bad, bix, 10), api.RingReplay, -2)):
                big, view = cg.destination(kind, 3, 1, (rows, f))
                src = [cg.source("48k") + (9000,), mid, cg.source("22k") + (30000,)]
                with pytest.raises(exc) as e:
                    dec.decode_clips_mfcc_long(src, f, out_mode=mode, out=view, **p)
                host = cg.host(big).reshape(3, 1, per + GUARD)
                assert e.value.valid[1] == code and (host[1] == SENT).all() and (host[:, :, per:] == SENT).all()
                got = host[[0, 2], :, :per].reshape(want.shape)
                assert np.array_equal(cg.bits(got), cg.bits(want)) and np.array_equal(e.value.valid[[0, 2]], valid)
        # bad arguments: nothing is written
        src = [cg.source("48k") + (9000,)]
        for mode in ref.MODES:
            big, view = cg.destination("device", 1, 1, (_rows(p, mode), f))
            common = (dict(top_db=float("nan")), dict(top_db=float("inf")), dict(top_db=-1.0), dict(n_fft=1024), dict(hop=0), dict(n_mels=0),
                      dict(n_mels=257), dict(amin=0.0), dict(f_max=12000.0), dict(width=65))
            ceps = (dict(n_mfcc=0), dict(n_mfcc=41), dict(lifter=-1.0), dict(lifter=float("nan")), dict(lifter=float("inf")), dict(deltas=3),
                    dict(deltas=-1), dict(delta_width=4), dict(delta_width=1), dict(delta_width=19), dict(n_mels=256, n_mfcc=129))
            for bad_p in common + (ceps if mode == "mfcc" else ()):
                q = dict(p, **bad_p)                       # (a destination of the shape these arguments ask for)
                big2, view2 = cg.destination("device", 1, 1, (max(_rows(q, mode), 1), f))
                with pytest.raises(RuntimeError):
                    dec.decode_clips_mfcc_long(src, f, out_mode=mode, out=view2, **q)
                assert (cg.host(big2) == SENT).all(), (mode, bad_p)
            with pytest.raises(RuntimeError):
                dec.decode_clips_mfcc_long([cg.source("48k") + (-1,)], f, out_mode=mode, out=view, **p)
            with pytest.raises(RuntimeError):            # (rate 0 and clips of different rates)
                dec.decode_clips_mfcc_long(src + [cg.source("32k") + (0,)], f, out_mode=mode, **dict(p, sample_rate=0))
            for m in ("ceps", 2, -1):
                with pytest.raises(RuntimeError):
                    dec.decode_clips_mfcc_long(src, f, out_mode=m, out=view, **p)
            assert (cg.host(big) == SENT).all()
    finally:
        dec.close()
        bix.close()


def test_more_clips_than_one_grid():
    """32 768 + 5 one-frame clips in one call with deltas 2 and top_db: pdmp3_hip_clip_mel_long and pdmp3_hip_clip_mfcc_long launch
    their kernels twice (a grid's y extent), the second time from descriptor 32 768 on.  Sixty-four distinct clips are held against
    the full chain from the log-mel call's values, every row is bit-equal to its twin among them; the last five are other clips
    than rows 0 .. 4, one of them behind the end"""
    name, k, f = "32k", 32768 + 5, 1
    p = dict(P0, sample_rate=0, hop=64, n_mels=8, n_mfcc=5, deltas=2, delta_width=3, top_db=6.0)
    rows = _rows(p, "mfcc")
    mp3, ix = cg.source(name)
    j_all = cg.j_all(p, name)
    starts = [1000 + 3001 * i for i in range(62)] + [j_all + 2048 + 200, j_all - 5]
    assert starts[61] + 2048 < j_all
    twin = (np.arange(k, dtype=np.int64) * 7) % 62
    twin[32768:] = [62, 63, 61, 60, 59]
    assert not np.any(twin[32768:] == twin[:5])
    dec = cg.decoder()
    try:
        first = [(name, s) for s in starts]
        l = _mel(dec, [(n, s - 64) for n, s in first], 3, p)
        base, valid64 = _run(dec, "device", first, f, p)
        for i in range(64):
            want, bound = ref.mfcc(l[i, 0], 5, 0.0, 6.0, 2, 3, 1)
            assert (np.abs(base[i, 0].astype(np.float64) - want) <= bound).all(), i
        assert list(valid64[61:]) == [1, 0, 1] and (base[62, 0, 5:10] == 0.0).all() and np.unique(base[:62, 0, 1, 0]).size > 8
        big, view = cg.destination("device", k, 1, (rows, f))
        out, valid = dec.decode_clips_mfcc_long([(mp3, ix, int(starts[t])) for t in twin], f, out=view, **p)
        host = cg.host(big).reshape(k, rows * f + GUARD)
        assert (host[:, rows * f:] == SENT).all(), "written behind a row's floats"
        assert np.array_equal(valid, valid64[twin]) and list(valid[32768:]) == [0, 1, 1, 1, 1]
        differ = np.flatnonzero((cg.bits(host[:, :rows * f]) != cg.bits(base[twin, 0].reshape(k, rows * f))).any(axis=1))
        assert differ.size == 0, "%d rows differ from their twins, %d of them in the second launch: %s" % (differ.size, int((differ >= 32768).sum()), differ[:8].tolist())
    finally:
        dec.close()


def test_return_types_defaults_and_empty_calls():
    import torch
    src = [cg.source("22k") + (120000,)]
    dec = cg.decoder()
    try:
        out, valid = dec.decode_clips_mfcc_long(src, 20)
        assert tuple(out.shape) == (1, 1, 20, 20) and out.is_cuda and out.dtype == torch.float32 and valid[0] == 20 and valid.dtype == np.int64
        plain, _ = _run(dec, "device", [("22k", 120000)], 20, P0)                     # (the defaults, spelled out)
        assert np.array_equal(cg.bits(cg.host(out)), cg.bits(plain)) and np.abs(plain).max() > 0.0
        out, valid = dec.decode_clips_mfcc_long(src, 20, deltas=2, channels=2)
        assert tuple(out.shape) == (1, 2, 60, 20)
        out, valid = dec.decode_clips_mfcc_long(src, 20, out_mode="db", n_mels=40)
        assert tuple(out.shape) == (1, 1, 40, 20) and float(cg.host(out).max() - cg.host(out).min()) <= 80.0
        pinned = torch.full((1, 1, 40, 20), float(SENT)).pin_memory()
        out2, _ = dec.decode_clips_mfcc_long(src, 20, out_mode="db", n_mels=40, out=pinned)
        assert out2 is pinned and np.array_equal(cg.bits(pinned.numpy()), cg.bits(cg.host(out)))
        for kw, shape in ((dict(), (0, 1, 20, 10)), (dict(deltas=1, n_mfcc=13), (0, 1, 26, 10)), (dict(out_mode="db"), (0, 1, 128, 10))):
            out, valid = dec.decode_clips_mfcc_long([], 10, **kw)
            assert tuple(out.shape) == shape and valid.size == 0
        for kw, shape in ((dict(deltas=2), (1, 1, 60, 0)), (dict(out_mode="db"), (1, 1, 128, 0))):
            out, valid = dec.decode_clips_mfcc_long(src, 0, **kw)
            assert tuple(out.shape) == shape and valid[0] == 0
    finally:
        dec.close()
