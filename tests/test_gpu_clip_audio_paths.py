"""Clips as float batches on the GPU, every path of k_clip_audio and of its host plumbing (pdmp3_amd/csrc/resample.hip,
stream.hip pdmp3_hip_clip_audio, host/clip_features.c pdmp3_amd_bulk_decode_clips_audio): the three resampling
forms by name -- plan 3: input span and table in LDS, plan 1: the span in LDS and the table from memory, plan 0: every sample
straight from memory --, output rates that are no MPEG rates, tile edges, host destinations as a loader lays them out, a call of
more clips than one grid holds, one decoder over many calls, far starts, and seeded random batches.

Every value is checked as in test_gpu_clip_audio.py (the same helpers): at the stream's own rate bit for bit against the
whole-stream decode, at another rate against clip_audio_ref.resample64 within its bound (T_j + 2) 2^-24 sum |h| |x|.  No other
tolerance.  The plan of a case is asserted from the product (api.audio_lds_plan) before the call: a change of audio_lds that
moves a case to another form fails here by name.

Plan 0 does `taps` fetches per output sample, each with 64-bit divisions: every clip sent on it has T * C * taps <= 2^27
(_cap_ok, from the table's shape -- a condition on the inputs, asserted before the call)."""
import ctypes as C
import time

import numpy as np
import pytest

import clip_audio_ref as ref
import clip_gpu as cg
import clip_streams
from clip_gpu import GUARD, SENT
from clip_gpu_calls import audio_check as _check, audio_run as _run

pytestmark = pytest.mark.gpu
PLAN0_WORK = 1 << 27


def _plan(name, rate, channels, width=0, rolloff=0.0):
    """the form of k_clip_audio a clip of this stream takes: "own" (no filter), else the product's LDS flags 0, 1 or 3"""
    from pdmp3_amd import api
    ix, _ = cg.ref(name)
    if not rate or rate == ix.rate:
        return "own"
    return api.audio_lds_plan(ix.rate, rate, channels, width, rolloff)[0]


def _cap_ok(name, rate, channels, t, width=0, rolloff=0.0):
    from pdmp3_amd import api
    if _plan(name, rate, channels, width, rolloff) != 0:
        return True
    return t * channels * api.audio_table(cg.ref(name)[0].rate, rate, width, rolloff)[0].shape[1] <= PLAN0_WORK


def _run_checked(dec, kind, clips, t, rate, channels, width=0, rolloff=0.0):
    """_run + _check on every row -> (worst error / bound per plan {plan: worst}, rows, valid)"""
    for n, s in clips:
        assert _cap_ok(n, rate, channels, t, width, rolloff), (n, rate, channels, t, width, rolloff)
    got, valid = _run(dec, kind, clips, t, rate, channels, width, rolloff)
    worst = {}
    for i, (n, s) in enumerate(clips):
        p = _plan(n, rate, channels, width, rolloff)
        worst[p] = max(worst.get(p, 0.0), _check(n, s, got[i], int(valid[i]), t, rate, channels, width or 6, rolloff or 0.99))
    return worst, got, valid


def _j(name, rate):
    ix, _ = cg.ref(name)
    return ref.out_length(ix.samples, ix.rate, rate or ix.rate)


def _starts(name, rate, t):
    """at 0, mid-stream inside a frame, across the stream's end J, behind it"""
    j = _j(name, rate)
    return [0, j // 3 + 11, max(j - t // 2, 0), j + 3]


# (stream, out rate, Z, rolloff, C, T, plan).  48 000 -> 8 000 at Z = 64 has L = 1: its table is one row of 775 (rolloff 0.99) or
# 3839 (0.2) coefficients, which fits LDS behind the span wherever the span does -- plan 3, not 1; 48 000 -> 4 000 at rolloff 0.5
# is the pair whose span fits at C = 1 without room for the table (plan 1) and not at all at C = 2 (plan 0).
PLAN_CASES = [
    ("44k-mono", 16000, 6, 0.99, 2, 5000, 3),
    ("mixed/mono-stereo", 16000, 6, 0.99, 1, 4999, 3),
    ("22k", 48000, 32, 0.99, 2, 6000, 1),
    ("mixed/mono-stereo", 44099, 6, 0.99, 2, 5000, 1),
    ("8k", 44101, 6, 0.99, 2, 5001, 1),
    ("48k", 8000, 64, 0.99, 2, 4100, 3),
    ("48k", 8000, 64, 0.2, 2, 4100, 0),
    ("48k", 8000, 64, 0.2, 1, 4100, 3),
    ("48k", 4000, 64, 0.5, 2, 4100, 0),
    ("48k", 4000, 64, 0.5, 1, 4100, 1),
    ("48k", 1000, 6, 0.99, 2, 2000, 0),
    ("mixed/mono-stereo", 100, 6, 0.99, 2, 500, 0),
]


@pytest.mark.parametrize("case", range(len(PLAN_CASES)), ids=["%s->%d-Z%d-r%g-C%d-plan%d" % (c[0].replace("/", "_"), c[1], c[2], c[3], c[4], c[6])
                                                                for c in PLAN_CASES])
def test_every_plan_by_name(case):
    from pdmp3_amd import api
    name, rate, width, rolloff, channels, t, plan = PLAN_CASES[case]
    ix, lr = cg.ref(name)
    assert api.audio_lds_plan(ix.rate, rate, channels, width, rolloff)[0] == plan, "%s: the LDS plan of this case has moved" % (PLAN_CASES[case],)
    clips = [(name, s) for s in _starts(name, rate, t)]
    if name == "mixed/mono-stereo" and rate == 16000:
        # one clip over the stream's loudest stretch: the conversion's end of range, and a downmix of it
        loud = int(np.flatnonzero((np.abs(lr) >= 32000).any(axis=0))[0])
        start = max(loud * rate // ix.rate - t // 2, 0)
        first, count = api.audio_span(ix.rate, rate, start, t, width, rolloff)
        assert first <= loud < first + count and ix.channels == 2 and (lr[0, first:first + count] != lr[1, first:first + count]).any()
        assert ((lr[0, first:first + count] + lr[1, first:first + count]) % 2 != 0).any()
        clips.append((name, start))
    dec = cg.decoder()
    try:
        for kind in ("device", "numpy"):
            worst, got, valid = _run_checked(dec, kind, clips, t, rate, channels, width, rolloff)
            assert set(worst) == {plan}
            print("plan %d, %s -> %d Hz, Z = %d, rolloff %g, %d channel(s), T = %d, %s: worst error / bound %.4f over %d clips" % (
                plan, name, rate, width, rolloff, channels, t, kind, worst[plan], len(clips)))
            assert 0.0 < worst[plan] <= 1.0
            assert valid[0] == min(t, _j(name, rate)) and valid[3] == 0 and 0 < valid[2] <= t
    finally:
        dec.close()


@pytest.mark.parametrize("kind", ["device", "numpy"])
def test_all_forms_in_one_launch(kind):
    """-> 8000 Hz at Z = 64, rolloff 0.2, two channels: 48 kHz on plan 0, 22.05 kHz on plan 1, 16 kHz on plan 3 and 8 kHz at its own
    rate in ONE call -- the launch's LDS is the largest plan's, a plan-0 and an own-rate clip use none of it"""
    rate, width, rolloff, channels, t = 8000, 64, 0.2, 2, 4100
    names = ["48k", "16k-mono", "22k", "8k", "48k", "16k-mono"]
    assert [_plan(n, rate, channels, width, rolloff) for n in names[:4]] == [0, 3, 1, "own"]
    clips = [(n, _starts(n, rate, t)[1 + i % 2]) for i, n in enumerate(names)]
    dec = cg.decoder()
    try:
        worst, got, valid = _run_checked(dec, kind, clips, t, rate, channels, width, rolloff)
        print("plans 0, 1, 3 and the own rate in one launch, %s: worst error / bound %s" % (kind, sorted(worst.items(), key=str)))
        assert set(worst) == {0, 1, 3, "own"} and all(0.0 < worst[p] <= 1.0 for p in (0, 1, 3))
    finally:
        dec.close()


EDGE_T = [1, 2, 255, 256, 257, 1023, 1024, 1025, 2048, 2049]


@pytest.mark.parametrize("kind", ["device", "numpy"])
@pytest.mark.parametrize("name,rate", [("32k", 16000), ("44k-mono", 0)])
def test_tile_edges(name, rate, kind):
    """T and J - start on and around the tile length: what nt, nv and the branch of a tile wholly behind the stream's end store"""
    ix, _ = cg.ref(name)
    j = _j(name, rate)
    assert ix.samples * (rate or ix.rate) % ix.rate == 0          # (J is N L / M exactly)
    dec = cg.decoder()
    try:
        for t in EDGE_T:
            left = sorted(set(d for d in (0, 1, 2, 1023, 1024, 1025, t - 1, t, t + 1) if d >= 0))
            clips = [(name, j - d) for d in left]
            worst, got, valid = _run_checked(dec, kind, clips, t, rate, ix.channels)
            assert [int(v) for v in valid] == [min(d, t) for d in left]
            assert worst.get(3, 0.0) <= 1.0 and (rate == 0 or _plan(name, rate, ix.channels) == 3)
            if rate and t > 2:
                assert worst[3] > 0.0
    finally:
        dec.close()


HOST_SOURCES = ["mixed/mono-stereo", "48k", "32k", "22k", "16k-mono", "8k", "44k-mono"]


def _host_clips(rate, t):
    return [(n, _starts(n, rate, t)[1 + i % 2]) for i, n in enumerate(HOST_SOURCES)]


def _decode_into(dec, clips, view, t, rate, channels):
    out, valid = dec.decode_clips_audio(cg.src(clips), t, rate, channels, out=view)
    assert out is view
    return valid


def _check_rows(clips, rows, valid, t, rate, channels, skip=()):
    worst = 0.0
    for i, (n, s) in enumerate(clips):
        if i not in skip:
            worst = max(worst, _check(n, s, rows[i], int(valid[i]), t, rate, channels))
    return worst


@pytest.mark.parametrize("channels", [1, 2])
def test_contiguous_numpy_destinations(channels):
    """a dense [K, C, T] numpy array has its rows one behind the other: they leave the device stage in ONE copy (clip_features.c, the loop
    behind pdmp3_hip_clip_audio) -- the whole array, the array in front of a guard, and with a refused clip in the middle, around
    which the merged copy must break"""
    from pdmp3_amd import api
    rate, t = 16000, 3001
    clips = _host_clips(rate, t)
    k = len(clips)
    assert k == 7 and len(set(cg.ref(n)[0].rate for n, _ in clips)) >= 6
    dec = cg.decoder()
    try:
        dense = np.full((k, channels, t), SENT, dtype=np.float32)
        assert dense.flags["C_CONTIGUOUS"]
        valid = _decode_into(dec, clips, dense, t, rate, channels)
        worst = _check_rows(clips, dense, valid, t, rate, channels)
        print("contiguous numpy [%d, %d, %d] -> %d Hz: worst error / bound %.3f" % (k, channels, t, rate, worst))
        assert 0.0 < worst <= 1.0
        # the same rows in front of a guard
        flat = np.full(k * channels * t + GUARD, SENT, dtype=np.float32)
        view = flat[:k * channels * t].reshape(k, channels, t)
        assert np.shares_memory(view, flat)
        valid = _decode_into(dec, clips, view, t, rate, channels)
        assert (flat[k * channels * t:] == SENT).all(), "written behind the last row"
        assert np.array_equal(view, dense)
        # a refused clip in the middle
        mix, _ = cg.ref("mixed/mpeg1-lsf")
        assert not mix.one_format
        holed = clips[:3] + [("mixed/mpeg1-lsf", 100)] + clips[4:]
        flat[:] = SENT
        with pytest.raises(api.MixedFormat) as e:
            _decode_into(dec, holed, view, t, rate, channels)
        assert e.value.valid[3] == api.PDMP3_BULK_MIXED_FORMAT and (view[3] == SENT).all() and (flat[k * channels * t:] == SENT).all()
        _check_rows(holed, view, e.value.valid, t, rate, channels, skip=(3,))
        assert np.array_equal(np.delete(view, 3, axis=0), np.delete(dense, 3, axis=0))
    finally:
        dec.close()


def test_stereo_rows_with_dense_channels_and_a_guard_between_rows():
    """channel stride T, row stride 2 T + GUARD: a row's two channels leave in one copy, no two rows do"""
    rate, t, channels = 16000, 3001, 2
    clips = _host_clips(rate, t)
    k = len(clips)
    dec = cg.decoder()
    try:
        big = np.full((k, 2 * t + GUARD), SENT, dtype=np.float32)
        view = np.lib.stride_tricks.as_strided(big, shape=(k, 2, t), strides=(big.strides[0], 4 * t, 4), writeable=True)
        assert np.shares_memory(view, big) and view.strides[1] == 4 * t
        valid = _decode_into(dec, clips, view, t, rate, channels)
        assert (big[:, 2 * t:] == SENT).all(), "written behind a row"
        worst = _check_rows(clips, big[:, :2 * t].reshape(k, 2, t), valid, t, rate, channels)
        print("rows of dense channels behind a guard -> %d Hz: worst error / bound %.3f" % (rate, worst))
        assert 0.0 < worst <= 1.0
    finally:
        dec.close()


@pytest.mark.parametrize("channels", [1, 2])
def test_pinned_host_destination(channels):
    import pdmp3_amd
    from pdmp3_amd import api
    rate, t = 16000, 3001
    clips = _host_clips(rate, t)
    k = len(clips)
    pin = api.PinnedPCM(2 * k * channels * (t + GUARD))
    dec = cg.decoder()
    try:
        big = pin.array.view(np.float32).reshape(k, channels, t + GUARD)
        hip = pdmp3_amd.load_library()
        hip.pdmp3_hip_host_is_pinned.argtypes = [C.c_void_p, C.c_size_t]
        assert hip.pdmp3_hip_host_is_pinned(big.ctypes.data, big.nbytes) == 1
        big[:] = SENT
        valid = _decode_into(dec, clips, big[:, :, :t], t, rate, channels)
        assert (big[:, :, t:] == SENT).all(), "written behind a row's samples"
        worst = _check_rows(clips, big[:, :, :t], valid, t, rate, channels)
        print("pinned host rows, %d channel(s) -> %d Hz: worst error / bound %.3f" % (channels, rate, worst))
        assert 0.0 < worst <= 1.0
        # ... and dense, without a guard between the rows
        dense = pin.array.view(np.float32)[:k * channels * t].reshape(k, channels, t)
        big[:] = SENT
        valid = _decode_into(dec, clips, dense, t, rate, channels)
        assert (pin.array.view(np.float32)[k * channels * t:] == SENT).all()
        _check_rows(clips, dense, valid, t, rate, channels)
        del big, dense
    finally:
        dec.close()
        pin.free()


@pytest.mark.parametrize("rate", [16000, 0])
def test_more_clips_than_one_grid(rate):
    """32 768 + 5 clips of one stream in one call: pdmp3_hip_clip_audio launches the kernel twice (a grid's y extent), the second
    time from descriptor 32 768 on"""
    name, t, k, base = "32k", 8, 32768 + 5, 50000
    ix, lr = cg.ref(name)
    offs = (np.arange(k, dtype=np.int64) * 37) % 4000
    assert base + 4000 + t < _j(name, rate) and np.unique(offs).size == 4000
    x = ref.channels64(lr, ix.channels, 1)
    y64, bound = ref.resample64(x, ix.rate, rate or ix.rate, 6, 0.99, base, 4000 + t)
    at = offs[:, None] + np.arange(t)[None, :]
    want, bnd = y64[0][at], bound[0][at]
    dec = cg.decoder()
    try:
        big, view = cg.destination("device", k, 1, (t,))
        mp3 = cg.streams()[name]
        t0 = time.perf_counter()
        out, valid = dec.decode_clips_audio([(mp3, ix, int(base + o)) for o in offs], t, rate, 1, out=view)
        wall = time.perf_counter() - t0
        host = cg.host(big)
        assert (host[:, :, t:] == SENT).all(), "written behind a row's samples"
        assert (valid == t).all()
        err = np.abs(host[:, 0, :t].astype(np.float64) - want)
        bad = np.flatnonzero((err > bnd).any(axis=1))
        assert bad.size == 0, "%d rows beyond the bound, %d of them in the second launch (rows >= 32768): %s" % (
            bad.size, int((bad >= 32768).sum()), bad[bad >= 32768][:8].tolist() or bad[:8].tolist())
        worst = float((err[bnd > 0] / bnd[bnd > 0]).max(initial=0.0))
        print("%d clips of %d samples -> %s in one call: %.2f s, worst error / bound %.3f" % (k, t, "%d Hz" % rate if rate else "own rate", wall, worst))
        if rate:
            assert 0.0 < worst <= 1.0 and (bnd[32768:] > 0).any()
        else:
            assert np.array_equal(host[:, 0, :t].astype(np.float64), want) and (want[32768:] != 0).any()
    finally:
        dec.close()


def test_one_decoder_over_many_calls():
    """a small call, a large one (both stages and the argument block are freed and allocated again), the small one again; twelve
    tables on one decoder, then the first again; plain frame ranges afterwards"""
    dec = cg.decoder()
    try:
        small = [("mixed/mono-stereo", 40000), ("48k", 7)]
        w1, first, v1 = _run_checked(dec, "numpy", small, 500, 16000, 2)
        assert 0.0 < w1[3] <= 1.0
        names = ["mixed/mono-stereo", "48k", "32k", "scfsi/joint", "h6/stereo", "44k-mono", "22k", "16k-mono"]
        t = 60000
        large = [(names[i % len(names)], 11 + 997 * i) for i in range(23)] + [("48k", 100000)]     # (the last one across its stream's end)
        assert all(_j(n, 16000) >= t // 2 for n, _ in large) and any(_j(n, 16000) < t + s for n, s in large)
        wl, _, vl = _run_checked(dec, "numpy", large, t, 16000, 2)
        assert 0.0 < wl[3] <= 1.0 and wl.get("own", 0.0) == 0.0
        w3, again, v3 = _run_checked(dec, "numpy", small, 500, 16000, 2)
        assert np.array_equal(again, first) and np.array_equal(v1, v3)
        keys = [(16000, 6, 0.99), (48000, 32, 0.99), (44099, 6, 0.99), (22051, 6, 0.99), (8000, 16, 1.0), (11025, 6, 0.5), (24000, 3, 0.99),
                (32000, 6, 0.8), (16000, 16, 0.99), (16000, 6, 0.9), (12000, 1, 1.0), (96000, 6, 0.99)]
        assert len(set(keys)) == 12
        for rate, width, rolloff in keys:
            w, got, valid = _run_checked(dec, "numpy", small, 500, rate, 2, width, rolloff)
            assert all(0.0 < x <= 1.0 for p, x in w.items() if p != "own"), (rate, width, rolloff, w)
            if (rate, width, rolloff) == keys[0]:
                assert np.array_equal(got, first)
        for kind in ("numpy", "device"):                                     # the first key again: its table is still the decoder's
            w, got, valid = _run_checked(dec, kind, small, 500, 16000, 2)
            assert np.array_equal(got, first)
        k = next(i for i, x in enumerate(clip_streams.gpu_streams()) if x[0] == "mixed/mono-stereo")
        ix, whole = cg.frames_ref(k)
        plain = dec.decode_range(clip_streams.gpu_streams()[k][1], ix, 33, 50)
        assert np.array_equal(plain, whole[int(ix.pcm_offsets[33]) // 2:int(ix.pcm_offsets[83]) // 2])
    finally:
        dec.close()


def test_far_starts_and_refusals():
    from pdmp3_amd import api
    t = 3000
    s = cg.streams()
    good, _ = cg.ref("48k")
    dec = cg.decoder()
    try:
        for kind in ("device", "numpy"):
            for rate in (16000, 0):
                _, got, valid = _run_checked(dec, kind, [("48k", 100)], t, rate, 2)
                stats = dec.clip_stats()
                _, got, valid = _run_checked(dec, kind, [("48k", 2 ** 40)], t, rate, 2)
                assert valid[0] == 0 and (got == 0).all() and dec.clip_stats() == stats
                _, got, valid = _run_checked(dec, kind, [("48k", 2 ** 40), ("48k", 100), ("48k", 2 ** 40 + 1)], t, rate, 2)
                assert list(valid) == [0, t, 0] and (got[0] == 0).all() and (got[2] == 0).all()
            big, view = cg.destination(kind, 2, 2, (t,))
            m, _ = ref.ratio(48000, 16000)
            limit = (2 ** 63 - 1) // 2 // m - t
            with pytest.raises(RuntimeError):
                dec.decode_clips_audio([(s["48k"], good, 100), (s["48k"], good, limit + 1)], t, 16000, 2, out=view)
            with pytest.raises(RuntimeError):
                dec.decode_clips_audio([(s["48k"], good, 100), (s["48k"], good, 0)], t, 2 ** 31 - 1, 2, out=view)
            assert (cg.host(big) == SENT).all()
            # at the limit itself: far behind the stream, zeros
            out, valid = dec.decode_clips_audio([(s["48k"], good, 100), (s["48k"], good, limit)], t, 16000, 2, out=view)
            host = cg.host(big)
            assert list(valid) == [t, 0] and (host[1, :, :t] == 0).all() and (host[:, :, t:] == SENT).all()
    finally:
        dec.close()


FUZZ_SEED = 20261017
FUZZ_RATES = [0] + ref.RATES + [44099, 22051, 11000, 96000, 4000, 1000]


def _fuzz_batches(index_of):
    """the 24 batches of the seed: dicts, or None for a batch dropped because pdmp3_amd_audio_table refuses one of its pairs.
    index_of(name) -> StreamIndex; needs no GPU (the seed is chosen where there is none)"""
    from pdmp3_amd import api
    rng = np.random.default_rng(FUZZ_SEED)
    names = sorted(n for n in cg.streams() if index_of(n).one_format)
    out = []
    for b in range(24):
        rate = int(rng.choice(FUZZ_RATES))
        width = int(rng.choice([1, 3, 6, 16, 64]))
        rolloff = float(rng.choice([0.99, 1.0, 0.5, 0.2]))
        channels = int(rng.choice([1, 2]))
        t = int(rng.integers(1, 6001))
        kind = str(rng.choice(["device", "numpy", "numpy-contiguous"]))
        clips, plans, refused = [], set(), False
        for _ in range(int(rng.integers(3, 11))):
            n = names[int(rng.integers(len(names)))]
            ix = index_of(n)
            start = int(rng.integers(0, ref.out_length(ix.samples, ix.rate, rate or ix.rate) + t // 2 + 1))
            if not rate or rate == ix.rate:
                plans.add("own")
                clips.append((n, start))
                continue
            try:
                taps = api.audio_table(ix.rate, rate, width, rolloff)[0].shape[1]
            except ValueError:
                refused = True
                continue
            plan = api.audio_lds_plan(ix.rate, rate, channels, width, rolloff)[0]
            if plan == 0 and t * channels * taps > PLAN0_WORK:
                continue
            plans.add(plan)
            clips.append((n, start))
        out.append(None if refused or not clips else dict(rate=rate, width=width, rolloff=rolloff, channels=channels, t=t, kind=kind, clips=clips, plans=plans))
    return out


def test_seeded_random_batches():
    batches = _fuzz_batches(lambda n: cg.ref(n)[0])
    assert sum(b is None for b in batches) <= 4
    assert set().union(*[b["plans"] for b in batches if b]) == {0, 1, 3, "own"}
    dec = cg.decoder()
    try:
        for i, b in enumerate(batches):
            if b is None:
                print("batch %d: dropped (a table of more than 2^22 coefficients)" % i)
                continue
            rate, width, rolloff, channels, t, clips = b["rate"], b["width"], b["rolloff"], b["channels"], b["t"], b["clips"]
            for n, s in clips:
                assert _cap_ok(n, rate, channels, t, width, rolloff)
            if b["kind"] == "numpy-contiguous":
                dense = np.full((len(clips), channels, t), SENT, dtype=np.float32)
                out, valid = dec.decode_clips_audio(cg.src(clips), t, rate, channels, width, rolloff, out=dense)
                got = dense
            else:
                got, valid = _run(dec, b["kind"], clips, t, rate, channels, width, rolloff)
            worst = {}
            for r, (n, s) in enumerate(clips):
                p = _plan(n, rate, channels, width, rolloff)
                worst[p] = max(worst.get(p, 0.0), _check(n, s, got[r], int(valid[r]), t, rate, channels, width, rolloff))
            assert set(worst) == b["plans"]
            print("batch %d: -> %s, Z = %d, rolloff %g, %d channel(s), T = %d, %s, %d clips: worst error / bound by plan %s" % (
                i, "%d Hz" % rate if rate else "own rate", width, rolloff, channels, t, b["kind"], len(clips), sorted(worst.items(), key=str)))
            assert all(x <= 1.0 for x in worst.values())
    finally:
        dec.close()
