"""Every decode launch shape of the engine on mixed-mode records.

The engine picks its code path from the launch size alone (pdmp3_amd/csrc/engine.hip launch_decode, auto_chunk): the
granule kernel with 8 or 16 waves per workgroup, or k_decode + k_decode_rare over chunks; each in an int16 and a float
form.  The other GPU tests meet content-rich records at 64 frames and large launches on the generator's M/S frames only.
Here one composite stream (corpus.composite: lone intensity-stereo frames in long M/S runs, mono runs shorter and longer
than a wave, every mode, three rates, the ISO switches, RESET frames in mid-stream) goes through every shape:

  * decoded into a buffer pre-filled with a sentinel: within +-1 LSB of the oracle, at most 2 % of the samples differing
    (float: 1e-5 absolute, corpus.F32_TOL_ABS's bar for the realistic level), the sentinel intact in the second half of
    every mono frame's place and behind the last frame -- a chunk neither k_decode nor k_decode_rare took shows there;
  * bit-identical to one reference decode of the whole stream, so all shapes are bit-identical to each other;
  * the kernel the case means to test is the one that ran (pdmp3_hip_last_launch_kind).

Sizes come from the device's CU count.  The CPU twin is tests/test_pipeline_emul.py (the composite cases)."""
import time

import numpy as np
import pytest

import corpus
import iso_streams
from conftest import C2_SEED
from test_lsf_pin import ISO_LSF, load_lsf_fixture, lsf_pcm_of_records
from util import GUARD, SENTINEL, SENTINEL_F32_BITS, check_launch_pcm

pytestmark = pytest.mark.gpu

CHUNKS, GRANULES8, GRANULES16 = 1, 8, 16          # include/pdmp3_hip.h PDMP3_HIP_LAUNCH_*
N_STREAM = 14400
N_MID = 3001                                      # "about 3000": fills the chip, far from either end of the 16-wave form's range
SEED_DENSE, SEED_SPARSE = 20240, 20241


class Sizes:
    def __init__(self):
        import torch
        self.cus = torch.cuda.get_device_properties(0).multi_processor_count
        self.w16_from = self.cus * 4 + 1          # first launch size with 16-wave workgroups
        self.gran_max = self.cus * 48             # last launch size the granule kernel takes
        self.chunk_slots = self.cus * 4 * 2       # waves of the chunk kernel resident at once (two per SIMD)

    def auto_chunk(self, n):
        """engine.hip auto_chunk restated: the fewest rounds of resident waves that keep a chunk at <= 32 frames"""
        if n <= self.chunk_slots:
            return 1
        rounds = -(-n // (self.chunk_slots * 32))
        return max(1, -(-n // (self.chunk_slots * rounds)))


@pytest.fixture(scope="module")
def sizes(engine):
    s = Sizes()
    assert s.w16_from < N_MID <= s.gran_max and s.gran_max + 1 + s.chunk_slots <= N_STREAM, "the composite does not fit this device"
    return s


def kind_of(eng):
    return int(eng.lib.pdmp3_hip_last_launch_kind(eng.h))


def sentinel_tensor(eng, n_values, f32=False):
    import torch
    if f32:
        return torch.full((n_values,), SENTINEL_F32_BITS, dtype=torch.int32, device=eng.tdev).view(torch.float32)
    return torch.full((n_values,), SENTINEL, dtype=torch.int16, device=eng.tdev)


def launch(eng, dsp, dsd, n, chunk, f32=False, state=None, first=0):
    """frames [first, first + n) of the uploaded records into a fresh sentinel buffer -> (numpy buffer with guard, kind)"""
    import torch
    out = sentinel_tensor(eng, n * 2304 + GUARD, f32)
    (eng.decode_f32 if f32 else eng.decode)(dsp[first:first + n], dsd[first:first + n], out, n_frames=n, state=state, chunk_frames=chunk)
    kind = kind_of(eng)
    torch.cuda.synchronize()
    return out.cpu().numpy(), kind


class Stream:
    """a composite stream, its oracle PCM (int16 and float), and on the device: the records and ONE reference decode of the
    whole of it (chunks of 257: every later shape must reproduce its prefix bit for bit -- the decode is causal)"""

    def __init__(self, engine, oracle, seed, sparse):
        self.sp, self.sd, self.segments, self.rare = corpus.composite(N_STREAM, seed, sparse=sparse)
        self.want, self.want_f32 = oracle.decode_f32(self.sp, self.sd)
        self.dsp, self.dsd = engine.upload(self.sp, self.sd)
        ref, kind = launch(engine, self.dsp, self.dsd, N_STREAM, 257)
        assert kind == CHUNKS
        check_launch_pcm(ref, self.want, self.sd, "reference decode")
        self.ref = ref[:-GUARD].reshape(N_STREAM, 2304)
        ref32, kind = launch(engine, self.dsp, self.dsd, N_STREAM, 257, f32=True)
        assert kind == CHUNKS
        self.ref_f32 = ref32[:-GUARD].reshape(N_STREAM, 2304)

    def first(self, label, nth=0):
        return [(a, b) for a, b, lab in self.segments if lab == label][nth]

    def check(self, got, n, what, first=0, f32=False):
        """got: the buffer a launch of frames [first, first + n) left -> (max difference, share of differing samples)"""
        sl = slice(first, first + n)
        if f32:
            d = check_launch_pcm(got, self.want_f32[sl], self.sd[sl], what, tol=1e-5)
            same = np.array_equal(got[:-GUARD].view(np.uint32), self.ref_f32[sl].ravel().view(np.uint32))
        else:
            d = check_launch_pcm(got, self.want[sl], self.sd[sl], what)
            same = np.array_equal(got[:-GUARD], self.ref[sl].ravel())
        assert same, "%s: PCM is not bit-identical to the reference decode's" % what
        return d


@pytest.fixture(scope="module")
def dense(engine, oracle):
    t = time.time()
    s = Stream(engine, oracle, SEED_DENSE, False)
    print("dense composite + oracle + reference decode: %.1f s" % (time.time() - t))
    return s


@pytest.fixture(scope="module")
def sparse(engine, oracle):
    s = Stream(engine, oracle, SEED_SPARSE, True)
    assert s.rare.size < N_STREAM / 300
    return s


def report(what, kind, d, f32=False):
    print("%-64s kind %2d  max %s  %.4f %% of the samples differ" % (what, kind, ("%.3g" % d[0]) if f32 else ("%d LSB" % d[0]), 100 * d[1]))


def ids(cases, k=1):
    return ["-".join(str(x) for x in c[:k]).replace(" ", "") for c in cases]


# ---- the shapes the session engine picks by size ----------------------------------------------------------------------
SIZE_SHAPES = [
    ("dense", "w16_from - 1", lambda s: s.w16_from - 1, GRANULES8),
    ("dense", "w16_from", lambda s: s.w16_from, GRANULES16),
    ("dense", "gran_max", lambda s: s.gran_max, GRANULES16),
    ("dense", "gran_max + 1", lambda s: s.gran_max + 1, CHUNKS),
    ("sparse", "gran_max", lambda s: s.gran_max, GRANULES16),
    ("sparse", "gran_max + 1", lambda s: s.gran_max + 1, CHUNKS),
    ("sparse", "gran_max + 1 + chunk_slots", lambda s: s.gran_max + 1 + s.chunk_slots, CHUNKS),
]


@pytest.mark.parametrize("which,name,size,kind", SIZE_SHAPES, ids=ids(SIZE_SHAPES, 2))
def test_gpu_engine_choice_by_size(engine, sizes, dense, sparse, which, name, size, kind):
    st = dense if which == "dense" else sparse
    n = size(sizes)
    got, k = launch(engine, st.dsp, st.dsd, n, 0)
    assert k == kind, "%d frames ran kind %d, the case is about kind %d" % (n, k, kind)
    if kind == CHUNKS:                                  # (on 256 CUs: chunks of 7 and 8, the last one partial)
        c = sizes.auto_chunk(n)
        assert c >= 2 and n % c != 0
    report("%s, %d frames (%s)" % (which, n, name), k, st.check(got, n, name))


@pytest.mark.parametrize("chunk", [2, 7, 61, 64, 65, 100, 257, N_MID])
def test_gpu_chunk_lengths(engine, sizes, dense, chunk):
    got, k = launch(engine, dense.dsp, dense.dsd, N_MID, chunk)
    assert k == CHUNKS
    kinds = corpus.rare_chunks(dense.sd[:N_MID], chunk)
    assert chunk >= 257 or (kinds.any() and not kinds.all())            # both kernels of the launch have chunks to take
    report("dense, %d frames in chunks of %d" % (N_MID, chunk), k, dense.check(got, N_MID, "chunks of %d" % chunk))


OWN_ENGINES = [("PDMP3_HIP_CHAIN", "0", CHUNKS), ("PDMP3_HIP_GRAN_W", "8", GRANULES8), ("PDMP3_HIP_SF_HINT", "1", GRANULES16),
               ("PDMP3_HIP_SF_HINT", "2", GRANULES16), ("PDMP3_HIP_DEBUG_FAR_TIMEOUT", "1", GRANULES16)]


@pytest.mark.parametrize("var,value,kind", OWN_ENGINES, ids=ids(OWN_ENGINES, 2))
def test_gpu_engines_with_a_setting(monkeypatch, engine, sizes, dense, var, value, kind):
    """engines of their own: chunks by the engine's choice (auto chunk 2), 8-wave workgroups on a launch that fills the
    chip, line tables loaded for another rate than the stream starts with, every far wait given up (the halo decode on
    rare and mono content).  Int16 and float."""
    import pdmp3_amd
    monkeypatch.setenv(var, value)
    eng = pdmp3_amd.Engine(0)
    monkeypatch.delenv(var)
    try:
        if var == "PDMP3_HIP_CHAIN":
            assert sizes.auto_chunk(N_MID) == 2
        for f32 in (False, True):
            got, k = launch(eng, dense.dsp, dense.dsd, N_MID, 0, f32=f32)
            assert k == kind
            report("dense, %d frames, %s=%s%s" % (N_MID, var, value, ", float" if f32 else ""), k,
                   dense.check(got, N_MID, "%s=%s" % (var, value), f32=f32), f32)
    finally:
        eng.close()


# ---- float PCM --------------------------------------------------------------------------------------------------------
FLOAT_SHAPES = [("w16_from - 1", lambda s: s.w16_from - 1, 0, GRANULES8), ("w16_from", lambda s: s.w16_from, 0, GRANULES16),
                ("gran_max", lambda s: s.gran_max, 0, GRANULES16), ("gran_max + 1", lambda s: s.gran_max + 1, 0, CHUNKS),
                ("N_MID in chunks of 61", lambda s: N_MID, 61, CHUNKS)]


@pytest.mark.parametrize("name,size,chunk,kind", FLOAT_SHAPES, ids=ids(FLOAT_SHAPES))
@pytest.mark.parametrize("which", ["dense", "sparse"])
def test_gpu_float_pcm_shapes(engine, sizes, dense, sparse, which, name, size, chunk, kind):
    """the <true> instantiations: 1e-5 absolute against the oracle's float PCM (the composite's sums stay below 4, where
    a binary32 ulp is 2.4e-7: the bar is 40 of them), bit-identical floats across shapes, and clip(trunc(f32 * 32767))
    == the int16 PCM of the same launch shape"""
    st = dense if which == "dense" else sparse
    n = size(sizes)
    assert 1.0 < float(np.abs(st.want_f32).max()) < 4.0
    got, k = launch(engine, st.dsp, st.dsd, n, chunk, f32=True)
    assert k == kind
    report("%s, %d frames (%s), float" % (which, n, name), k, st.check(got, n, name, f32=True), True)
    pcm, k = launch(engine, st.dsp, st.dsd, n, chunk)
    assert k == kind
    q = np.clip(np.trunc(got[:-GUARD].astype(np.float64) * 32767.0), -32767, 32767).astype(np.int16)
    written = got[:-GUARD].view(np.uint32) != SENTINEL_F32_BITS
    assert np.array_equal(q[written], pcm[:-GUARD][written]) and (pcm[:-GUARD][~written] == SENTINEL).all()


# ---- which kernel takes which chunk -----------------------------------------------------------------------------------
def test_gpu_rare_chunk_bookkeeping(engine, oracle, sizes, sparse):
    """a big launch in which a few chunks out of many are k_decode_rare's: the case the flag word exists for.  Then the SAME
    buffers with the rare frames overwritten by ordinary ones: nothing of the first launch's flag word may make
    k_decode_rare take or skip anything."""
    import torch
    n = sizes.gran_max + 1
    chunk = sizes.auto_chunk(n)
    kinds = corpus.rare_chunks(sparse.sd[:n], chunk)                    # a condition on the input, before anything is launched
    assert kinds.sum() >= 10 and (~kinds).mean() >= 0.9, "%d of %d chunks are rare" % (kinds.sum(), kinds.size)
    got, k = launch(engine, sparse.dsp, sparse.dsd, n, 0)
    assert k == CHUNKS
    report("sparse, %d frames: %d rare chunks of %d" % (n, kinds.sum(), kinds.size), k, sparse.check(got, n, "sparse big launch"))
    sd2 = sparse.sd[:n].copy()
    fr = sd2["frame"]
    rare = sparse.rare[sparse.rare < n]
    fr[rare] = (fr[rare] & ~np.uint8(3 << corpus.FR_MODEEXT_SHIFT)) | np.uint8(2 << corpus.FR_MODEEXT_SHIFT)
    assert not corpus.frame_is_rare(sd2).any() and rare.size >= 10
    want2 = oracle.decode(sparse.sp[:n], sd2)
    assert not np.array_equal(want2, sparse.want[:n])
    keep = sparse.dsd[:n].clone()
    try:
        sparse.dsd[:n].copy_(torch.from_numpy(sd2.view(np.uint8).reshape(n, 4, 128).copy()))
        got2, k = launch(engine, sparse.dsp, sparse.dsd, n, 0)
        assert k == CHUNKS
        report("the same buffers, rare frames made ordinary", k, check_launch_pcm(got2, want2, sd2, "edited stream"))
        m = sizes.gran_max
        got3, k = launch(engine, sparse.dsp, sparse.dsd, m, 0)
        assert k == GRANULES16
        check_launch_pcm(got3, want2[:m], sd2[:m], "edited stream, granule kernel")
        assert np.array_equal(got3[:-GUARD], got2[:m * 2304]), "chunk kernels != granule kernel on the edited stream"
    finally:
        sparse.dsd[:n].copy_(keep)
        torch.cuda.synchronize()


def test_gpu_back_to_back_launches_on_two_streams(engine, sizes, sparse):
    """the sparse big launch on one HIP stream and an all-ordinary big launch (generator records) on another, issued
    without a synchronise in between, three rounds: each result is what the launch gives alone"""
    import torch
    n = sizes.gran_max + 1
    gsp, gsd, _ = engine.alloc_frames(n)
    engine.generate(C2_SEED, 0, n, gsp, gsd)
    alone_a, k = launch(engine, sparse.dsp, sparse.dsd, n, 0)
    assert k == CHUNKS
    alone_b, k = launch(engine, gsp, gsd, n, 0)
    assert k == CHUNKS
    sparse.check(alone_a, n, "sparse alone")
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    outs = [(sentinel_tensor(engine, n * 2304 + GUARD), sentinel_tensor(engine, n * 2304 + GUARD)) for _ in range(3)]
    torch.cuda.synchronize()
    for a, b in outs:
        with torch.cuda.stream(sa):
            engine.decode(sparse.dsp[:n], sparse.dsd[:n], a, n_frames=n)
            assert kind_of(engine) == CHUNKS
        with torch.cuda.stream(sb):
            engine.decode(gsp, gsd, b, n_frames=n)
            assert kind_of(engine) == CHUNKS
    torch.cuda.synchronize()
    for r, (a, b) in enumerate(outs):
        assert np.array_equal(a.cpu().numpy(), alone_a), "round %d, sparse stream" % r
        assert np.array_equal(b.cpu().numpy(), alone_b), "round %d, generator stream" % r


# ---- state hand-over between launches of different kinds ------------------------------------------------------------------
def test_gpu_state_handover_across_kinds(engine, sizes, dense):
    """the stream cut in the middle of the 70- and 130-frame mono runs, behind a lone intensity-stereo frame, at a rate
    change and behind a RESET frame; the pieces decoded through ONE state block, each by another kind of launch, in three
    orders of kinds: the concatenation is the whole decode bit for bit, and so is the final state block"""
    import torch
    n = N_MID
    fr = dense.sd["frame"][:, 0, 0]
    is0 = dense.first("is")[1]                                          # the frame behind the first lone intensity-stereo frame
    m70, m130 = dense.first("mono70"), dense.first("mono130")
    rate = m130[1]                                                      # mono at 48 kHz | plain stereo at 32 kHz
    assert (fr[rate - 1] & 3) != (fr[rate] & 3)
    resets = [int(f) for f in np.flatnonzero(fr[:n] & corpus.FR_RESET) if f >= rate + sizes.w16_from]
    m70b = dense.first("mono70", 2)
    cuts = [0, is0, sum(m70) // 2, sum(m130) // 2, rate, resets[0] + 1, sum(m70b) // 2, n]
    assert cuts == sorted(cuts) and cuts[5] - cuts[4] >= sizes.w16_from
    assert max(b - a for a, b in zip(cuts, cuts[1:]) if a != rate) < sizes.w16_from
    st_whole = engine.new_state()
    whole, k = launch(engine, dense.dsp, dense.dsd, n, 257, state=st_whole)
    assert k == CHUNKS
    dense.check(whole, n, "whole, with a state block")
    g8, g16, c7, c100 = (0, GRANULES8), (0, GRANULES16), (7, CHUNKS), (100, CHUNKS)
    for order in ([g8, c7, c100, g8, g16, c7, c100], [c100, g8, c7, c100, g16, g8, c7], [c7, c100, g8, c7, g16, c100, g8]):
        st = engine.new_state()
        out = sentinel_tensor(engine, n * 2304 + GUARD)
        for (a, b), (chunk, kind) in zip(zip(cuts, cuts[1:]), order):
            engine.decode(dense.dsp[a:b], dense.dsd[a:b], out[a * 2304:], n_frames=b - a, state=st, chunk_frames=chunk)
            assert kind_of(engine) == kind, (a, b, chunk)
        torch.cuda.synchronize()
        dense.check(out.cpu().numpy(), n, "pieces %s" % (order,))
        assert torch.equal(st, st_whole), "the final state block differs from the whole decode's"


@pytest.mark.parametrize("start", ["on a lone rare frame", "inside a mono run"], ids=["rare", "mono"])
def test_gpu_smallest_launches(engine, sizes, dense, start):
    """1, 2, 15, 16, 17 frames that start on a lone intensity-stereo frame / inside a mono run, with the state the frames
    before them left, at chunk_frames 0, 1 and n: PCM of the whole decode, and the state block a single launch up to there leaves"""
    import torch
    f = dense.first("is")[0] if start == "on a lone rare frame" else dense.first("mono70")[0] + 33
    st0 = engine.new_state()
    launch(engine, dense.dsp, dense.dsd, f, 0, state=st0)
    for n in (1, 2, 15, 16, 17):
        st_want = engine.new_state()
        launch(engine, dense.dsp, dense.dsd, f + n, 0, state=st_want)
        for chunk in (0, 1, n):
            st = st0.clone()
            got, k = launch(engine, dense.dsp, dense.dsd, n, chunk, state=st, first=f)
            assert k == (GRANULES8 if chunk <= 1 else CHUNKS), (n, chunk, k)
            dense.check(got, n, "%d frames %s, chunk_frames %d" % (n, start, chunk), first=f)
            assert torch.equal(st, st_want), (n, chunk)


# ---- LSF record launches at size ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lsf_22k_msis", "lsf_16k_mono", "lsf_8k_msis"])
@pytest.mark.parametrize("odd", [False, True], ids=["even", "odd"])
def test_gpu_lsf_launch_at_size(engine, oracle, name, odd):
    """pdmp3_hip_decode_lsf_frames (chunks of 2 record-frames through k_lsf_pair) on more than 4096 frames: a fixture's
    records tiled, each tile starting with its RESET frame; +-1 LSB of the oracle on the records, int16 and float,
    nothing written outside the frames' places (mono: a pair of frames in the first half of a place; an odd count: the
    last place half filled)"""
    import torch
    from pdmp3_amd import api
    mp3, _, kw = load_lsf_fixture(name)
    nch = iso_streams.nch_of(kw)
    sp1, sd1 = api.parse_like_cli(mp3, 4096, ISO_LSF)
    assert sd1["frame"][0, 0, 0] & corpus.FR_RESET and sp1.shape[0] >= 30
    tiles = 4096 // sp1.shape[0] + 1
    n = tiles * sp1.shape[0] - (tiles * sp1.shape[0] + int(odd)) % 2
    assert n > 4096 and n % 2 == int(odd)
    sp = np.tile(sp1, (tiles, 1, 1, 1))[:n]
    sd = np.tile(sd1, (tiles, 1, 1))[:n]
    w16, w32 = oracle.decode_f32(sp, sd)
    dsp, dsd = engine.upload(sp, sd)
    places = (n + 1) // 2
    written = np.zeros((places, 2, 1152), dtype=bool)                   # [place][frame of the pair][values, 576 x nch of them used]
    written[:, :, :576 * nch] = True
    if odd:
        written[-1, 1] = False
    if nch == 2:
        written = written.reshape(places, 2304)
    else:
        written = np.concatenate([written[:, :, :576].reshape(places, 1152), np.zeros((places, 1152), bool)], axis=1)
    written = np.concatenate([written.ravel(), np.zeros(GUARD, bool)])
    outs = {}
    for f32 in (False, True):
        out = sentinel_tensor(engine, places * 2304 + GUARD, f32)
        engine.decode_lsf(dsp, dsd, out, n_frames=n)
        assert kind_of(engine) == CHUNKS
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        bits = got.view(np.uint32) if f32 else got
        assert (bits[~written] == (SENTINEL_F32_BITS if f32 else SENTINEL)).all(), "written outside the frames' places"
        want = lsf_pcm_of_records(w32 if f32 else w16, n, nch).ravel()
        d = np.abs(got[written].astype(np.float64) - want)
        outs[f32] = got[written]
        assert d.max() <= (1.0 / 32767.0 if f32 else 1), "%s PCM differs by %g" % ("float" if f32 else "int16", d.max())
        report("%s tiled to %d frames%s" % (name, n, ", float" if f32 else ""), CHUNKS, (float(d.max()) if f32 else int(d.max()), float((d > 0).mean())), f32)
    q = np.clip(np.trunc(outs[True].astype(np.float64) * 32767.0), -32767, 32767).astype(np.int16)
    assert np.array_equal(q, outs[False])
