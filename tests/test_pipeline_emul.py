"""Host build of the device pipeline (pdmp3_amd/csrc/decode_core.h compiled by
g++, tests/host_emul: the SAME source the GPU runs, one wave = 64 fibers, the matrix
instruction evaluated with the hardware's fragment layout as k-ordered fmaf chains)
against the oracle: validates the kernel's indexing, tables, fragment layouts,
chunk/halo logic and state hand-off without a GPU.  Same bars as the GPU parity
tests (test_gpu_parity.py), which go through the C-ABI on the real device."""
import ctypes as C

import numpy as np
import pytest

import corpus
from conftest import C2_SEED
from util import assert_pcm_close, check_launch_pcm, nch_of, sentinel_buffer


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def emul_decode(emul, sp, sd, chunk=0, state=None, stages=False):
    n = sp.shape[0]
    pcm = np.zeros((n, 2304), np.int16)
    stg = np.zeros((n, 2, 2, 4, 576), np.float32) if stages else None
    emul.emul_decode_frames(_p(sp), _p(sd), n, _p(state), _p(pcm), _p(stg), chunk)
    return (pcm, stg) if stages else pcm


@pytest.mark.parametrize("name", list(corpus.ALL_CASES))
def test_emul_vs_oracle(oracle, emul, name):
    """the bars of test_gpu_parity.py, literally: corpus.PCM_TOL_LSB (1 LSB but for ms_loud_clip: 32), 64 frames"""
    sp, sd = corpus.case(name)
    want, ws = oracle.decode(sp, sd, stages=True)
    got, gs = emul_decode(emul, sp, sd, stages=True)
    nch = nch_of(sd)
    for k in range(3):   # separately rounded mul / add like the reference: bit-exact
        assert np.array_equal(ws[:, :, :nch, k].view(np.uint32), gs[:, :, :nch, k].view(np.uint32)), "stage %d" % k
    amp = max(1.0, float(np.abs(ws[:, :, :nch, 3]).max()))
    err = float(np.abs(ws[:, :, :nch, 3] - gs[:, :, :nch, 3]).max())
    assert err <= 1e-5 * amp, "hybrid output differs by %g (amplitude %g)" % (err, amp)
    assert_pcm_close(got, want, corpus.PCM_TOL_LSB[name], name)
    # the stage dumps come from the general formulation of every phase; without them the wave takes the fast paths
    # (ph_requant_long for granules of long blocks): the same arithmetic per line, so the same PCM bit for bit
    assert np.array_equal(emul_decode(emul, sp, sd), got), "fast paths differ from the general formulation"


@pytest.mark.parametrize("chunk", [1, 2, 3, 5, 16])
def test_emul_chunking_is_invisible(oracle, emul, chunk):
    sp, sd = oracle.generate(C2_SEED, 0, 40)
    whole = emul_decode(emul, sp, sd, 0)
    assert np.array_equal(emul_decode(emul, sp, sd, chunk), whole)


def test_emul_state_handoff(oracle, emul):
    sp, sd = oracle.generate(C2_SEED, 0, 30)
    whole = emul_decode(emul, sp, sd, 0)
    st = np.zeros(emul.emul_state_floats(), np.float32)
    a = emul_decode(emul, sp[:11], sd[:11], 0, st)
    b = emul_decode(emul, sp[11:], sd[11:], 4, st)
    assert np.array_equal(np.concatenate([a, b]), whole)


def test_emul_generator(oracle, emul):
    sp, sd = oracle.generate(C2_SEED, 3, 9)
    sp2 = np.zeros_like(sp)
    sd2 = np.zeros_like(sd)
    emul.emul_generate_frames(C.c_uint64(C2_SEED), C.c_int64(3), 9, _p(sp2), _p(sd2))
    assert np.array_equal(sp, sp2) and np.array_equal(sd.view(np.uint8), sd2.view(np.uint8))


def _mode_switch_records():
    """stereo / mono / stereo runs, incl. single stereo frames between mono runs (records from the host parser)"""
    from pdmp3_amd import api
    from pdmp3_amd.packer import packer
    parts = [dict(n_frames=9, seed=31, bitrate_index=9), dict(n_frames=11, seed=32, mode=3, bitrate_index=7),
             dict(n_frames=2, seed=33, mode=1, mode_ext=2, bitrate_index=11, block_pct=(10, 10, 70, 10)),
             dict(n_frames=7, seed=34, mode=3, bitrate_index=7),
             dict(n_frames=12, seed=35, mode=1, mode_ext=2, bitrate_index=11, block_pct=(10, 10, 70, 10))]
    mp3 = b"".join(packer.generate(**p) for p in parts)
    return api.parse_like_cli(mp3, 64)


@pytest.mark.parametrize("chunk", [1, 2, 3, 4, 7, 16])
def test_emul_channel1_state_survives_mono_runs(oracle, emul, chunk):
    """mono frames leave channel 1's overlap / polyphase history alone (P:1777, P:2126 are per channel): a chunk
    that starts after a mono run must find channel 1 as the last stereo frame left it"""
    sp, sd = _mode_switch_records()
    assert sp.shape[0] >= 38
    want = oracle.decode(sp, sd)
    assert_pcm_close(emul_decode(emul, sp, sd, chunk), want, 1, "chunk %d" % chunk)
    assert np.array_equal(emul_decode(emul, sp, sd, chunk), emul_decode(emul, sp, sd, 0))


def test_emul_channel1_state_across_batches(oracle, emul):
    """the carried state keeps channel 1 through an all-mono batch decoded in several chunks"""
    sp, sd = _mode_switch_records()
    whole = emul_decode(emul, sp, sd, 0)
    st = np.zeros(emul.emul_state_floats(), np.float32)
    cuts = [0, 9, 14, 20, 22, 29, sp.shape[0]]          # 9..20 mono (two batches), 22..29 mono
    out = [emul_decode(emul, sp[a:b], sd[a:b], 2, st) for a, b in zip(cuts[:-1], cuts[1:])]
    assert np.array_equal(np.concatenate(out), whole)
    # batches that end in mono right after stereo frames (pre-halo touching the ordinary halo), every chunk size
    for chunk in (1, 2, 3):
        for cuts in ([0, 7, 11, 19, 24, 31, sp.shape[0]], [0, 8, 10, 21, 23, 30, sp.shape[0]]):
            st[:] = 0
            out = [emul_decode(emul, sp[a:b], sd[a:b], chunk, st) for a, b in zip(cuts[:-1], cuts[1:])]
            assert np.array_equal(np.concatenate(out), whole), (chunk, cuts)


def test_shard_cut_after_mono_frames_reaches_back_to_the_last_stereo_frame(emul):
    """pdmp3_amd.sharding.halo_start: a shard whose cut follows mono frames starts in front of the last stereo frame,
    so that channel 1 is what that frame left (the kernel's pre-halo finds it inside the shard); with the fixed
    2-frame halo alone some of these cuts come out wrong -- the test must bite"""
    from pdmp3_amd.sharding import halo_start
    sp, sd = _mode_switch_records()
    n = sp.shape[0]
    flags = sd["frame"][:, 0, 0] if sd["frame"].ndim == 3 else sd["frame"].reshape(n, -1)[:, 0]
    whole = emul_decode(emul, sp, sd, 0)
    fixed_fails = 0
    for lo in range(1, n):
        first = halo_start(lo, flags)
        assert 0 <= first <= max(0, lo - 2) or first == 0
        part = emul_decode(emul, sp[first:], sd[first:], 3)[lo - first:]
        assert np.array_equal(part, whole[lo:]), (lo, first)
        f2 = max(0, lo - 2)
        if first != f2 and not np.array_equal(emul_decode(emul, sp[f2:], sd[f2:], 3)[lo - f2:], whole[lo:]):
            fixed_fails += 1
    assert fixed_fails > 0
    assert halo_start(lo, None) == lo - 2 and halo_start(0, flags) == 0


def test_oracle_float_pcm_is_what_the_int16_comes_from(oracle):
    """float output is pinned through its quantisation: the oracle's int16 PCM -- bit-exact against the compiled
    reference (test_oracle.py) -- is clip(trunc(float * 32767)) of the float it hands out (P:2028-2031)"""
    sp, sd = oracle.generate(C2_SEED, 0, 24)
    pcm, f32 = oracle.decode_f32(sp, sd)
    assert np.array_equal(pcm, oracle.decode(sp, sd))
    q = np.clip(np.trunc(f32.astype(np.float64) * 32767.0), -32767, 32767).astype(np.int16)
    assert np.array_equal(q, pcm)
    assert np.abs(f32).max() > 0.5


@pytest.mark.parametrize("name", list(corpus.ALL_CASES))
def test_emul_float_pcm(oracle, emul, name):
    """pdmp3_hip_decode_frames_f32 on the host build: 1e-5 absolute (north_star's float tolerance) on the `_fs` cases,
    corpus.F32_TOL_ABS's literal number on the loud ones; chunked == unchunked"""
    sp, sd = corpus.case(name)
    _, want = oracle.decode_f32(sp, sd)
    n = sp.shape[0]
    got = np.zeros((n, 2304), np.float32)
    emul.emul_decode_frames_f32(_p(sp), _p(sd), n, None, _p(got), 0)
    assert float(np.abs(got - want).max()) <= corpus.F32_TOL_ABS[name]
    got2 = np.zeros((n, 2304), np.float32)
    emul.emul_decode_frames_f32(_p(sp), _p(sd), n, None, _p(got2), 3)
    assert np.array_equal(got, got2)


def emul_decode_granules(emul, sp, sd, state=None, f32=False, debug=0, sf_hint=0):
    n = sp.shape[0]
    pcm = np.zeros((n, 2304), np.float32 if f32 else np.int16)
    emul.emul_decode_frames_granules(_p(sp), _p(sd), n, _p(state), None if f32 else _p(pcm), _p(pcm) if f32 else None, debug, sf_hint)
    return pcm


@pytest.mark.parametrize("name", list(corpus.CASES))
def test_emul_granule_waves_equal_independent_chunks(emul, name):
    """run_granule (one granule per wave, tails and matrixing rows handed on) is the same arithmetic in the same order as
    run_chunk: PCM bit-identical for every block-type mix (incl. the H5 corner, whose peek values travel with the rows),
    mono corpora (run_chunk inside the granule kernel) and the long-block fast path of the requantisation"""
    sp, sd = corpus.case(name, n=13)
    want = emul_decode(emul, sp, sd, 0)
    assert np.array_equal(emul_decode_granules(emul, sp, sd), want)


def test_emul_granule_waves_states_resets_mode_and_rate_switches(emul, oracle):
    sp, sd = _mode_switch_records()
    whole = emul_decode(emul, sp, sd, 0)
    assert np.array_equal(emul_decode_granules(emul, sp, sd), whole)
    # the carried state in and out, batch after batch (granule 0 of a batch takes the caller's state; H5 at frame 0)
    sp, sd = oracle.generate(C2_SEED, 0, 64)
    whole = emul_decode(emul, sp, sd, 0)
    st = np.zeros(emul.emul_state_floats(), np.float32)
    st_ref = np.zeros(emul.emul_state_floats(), np.float32)
    cuts = [0, 1, 2, 9, 10, 31, 47, 48, 64]
    out = [emul_decode_granules(emul, sp[a:b], sd[a:b], st) for a, b in zip(cuts[:-1], cuts[1:])]
    assert np.array_equal(np.concatenate(out), whole)
    emul_decode(emul, sp, sd, 0, st_ref)
    assert np.array_equal(st.view(np.uint32), st_ref.view(np.uint32))
    # a RESET frame in the middle: its input state is zero, no wait
    sd2 = sd.copy()
    sd2["frame"][20] |= 0x40
    assert np.array_equal(emul_decode_granules(emul, sp, sd2), emul_decode(emul, sp, sd2, 0))
    # float PCM
    got = emul_decode_granules(emul, sp[:24], sd[:24], f32=True)
    want = np.zeros((24, 2304), np.float32)
    emul.emul_decode_frames_f32(_p(sp[:24]), _p(sd[:24]), 24, None, _p(want), 0)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # every frame a short block in granule 1 / channel 1 (H5: the peek values come with the rows of granule 0)
    sp3, sd3 = corpus.case("ms_short_heavy_480", n=16)
    assert np.array_equal(emul_decode_granules(emul, sp3, sd3), emul_decode(emul, sp3, sd3, 0))
    # the sampling frequency changes inside the batch, and the workgroups' line tables are for another one altogether:
    # such granules read the global line table (ph_requant's TG)
    a, sa = corpus.case("ms_long_441", n=6)
    b, sb = corpus.case("ms_short_heavy_480", n=6)
    sp4 = np.concatenate([a, b, a]); sd4 = np.concatenate([sa, sb, sa])
    for hint in (0, 1, 2):
        assert np.array_equal(emul_decode_granules(emul, sp4, sd4, sf_hint=hint), emul_decode(emul, sp4, sd4, 0)), hint


@pytest.mark.parametrize("name", ["ms_long_441", "ms_short_heavy_480", "mono_441"])
def test_emul_granule_waves_give_up_waiting_for_other_workgroups(emul, name):
    """the bounded wait (gran_far_wait): with every wait for another workgroup giving up at once, the first wave of each
    workgroup derives the state at the start of its frame the independent way (gran_slow_chunk(..., state_only): run_chunk's
    halo as a called function) and goes on as a granule wave with it -- same PCM"""
    sp, sd = corpus.case(name, n=21)
    want = emul_decode(emul, sp, sd, 0)
    assert np.array_equal(emul_decode_granules(emul, sp, sd, debug=1), want)


def emul_decode_ring(emul, sp, sd, per, state=None, f32=False, sf_hint=0):
    n = sp.shape[0]
    pcm = np.zeros((n, 2304), np.float32 if f32 else np.int16)
    emul.emul_decode_frames_ring(_p(sp), _p(sd), n, _p(state), None if f32 else _p(pcm), _p(pcm) if f32 else None, per, sf_hint)
    return pcm


@pytest.mark.parametrize("name", list(corpus.ALL_CASES))
def test_emul_persistent_granule_kernel_equals_independent_chunks(emul, name):
    """run_granule_ring (k_decode_p: 16 waves going round a range of frames, ring of LDS mailboxes, one halo per range) is the
    same arithmetic in the same order as run_chunk: PCM bit-identical on every corpus -- ranges of 8 frames (one turn of
    the ring), 9 (odd: a range ends in the middle of a turn), 23 and the whole batch; H5 frames at range starts, mono
    corpora (every frame through run_chunk inside the loop), RESET frames, intensity stereo"""
    sp, sd = corpus.case(name, n=51)
    want = emul_decode(emul, sp, sd, 0)
    for per in (8, 9, 23, 51):
        assert np.array_equal(emul_decode_ring(emul, sp, sd, per), want), per


def test_emul_persistent_granule_kernel_states_and_mode_switches(emul, oracle):
    """stereo / mono / stereo runs cut by range boundaries everywhere (the halo frame in front of a range is mono, or
    stereo right after mono: the range's first wave derives the state with run_chunk's halo; a range that starts with a
    mono frame or a RESET frame needs none), the carried state in and out batch after batch, float PCM, another
    sampling frequency than the workgroup's tables"""
    sp, sd = _mode_switch_records()
    whole = emul_decode(emul, sp, sd, 0)
    for per in (8, 9, 10, 11, 13):
        assert np.array_equal(emul_decode_ring(emul, sp, sd, per), whole), per
    sp, sd = oracle.generate(C2_SEED, 0, 96)
    whole = emul_decode(emul, sp, sd, 0)
    st = np.zeros(emul.emul_state_floats(), np.float32)
    st_ref = np.zeros(emul.emul_state_floats(), np.float32)
    cuts = [0, 17, 33, 34, 60, 96]
    out = [emul_decode_ring(emul, sp[a:b], sd[a:b], 8, st) for a, b in zip(cuts[:-1], cuts[1:])]
    assert np.array_equal(np.concatenate(out), whole)
    emul_decode(emul, sp, sd, 0, st_ref)
    assert np.array_equal(st.view(np.uint32), st_ref.view(np.uint32))
    sd2 = sd.copy()
    for f in (16, 24, 41):                                  # RESET at a range start, right before one, in the middle
        sd2["frame"][f] |= 0x40
    assert np.array_equal(emul_decode_ring(emul, sp, sd2, 8), emul_decode(emul, sp, sd2, 0))
    got = emul_decode_ring(emul, sp[:40], sd[:40], 8, f32=True)
    want = np.zeros((40, 2304), np.float32)
    emul.emul_decode_frames_f32(_p(sp[:40]), _p(sd[:40]), 40, None, _p(want), 0)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    a, sa = corpus.case("ms_long_441", n=12)
    b, sb = corpus.case("ms_short_heavy_480", n=12)
    sp4 = np.concatenate([a, b, a]); sd4 = np.concatenate([sa, sb, sa])
    for hint in (0, 1):
        assert np.array_equal(emul_decode_ring(emul, sp4, sd4, 8, sf_hint=hint), emul_decode(emul, sp4, sd4, 0)), hint


def test_emul_int16_conversion_lane_form_equals_the_reference_conversion(emul):
    """pcm_convert18_lane -- binary32 product rounded toward zero, v_med3 clamp (NaN -> min3), the wrap-around beyond
    65538 -- against pcm_from_sum (P:2028-2031: binary64 product, cvttsd2si, clip to +-32767), per sample: the
    per-sample form (`wrap`) everywhere, the fast form wherever no sample of the wave is beyond the wrap point -- NaNs
    included, which the wave-wide test (an fmax) does not see: both forms give -32767 for them"""
    rng = np.random.default_rng(7)
    n = 18 * 4000
    s = np.concatenate([
        rng.standard_normal(n).astype(np.float32),                              # around full scale
        (rng.standard_normal(n) * 1e-3).astype(np.float32),
        (rng.integers(-40000, 40000, n) / np.float32(32767.0)).astype(np.float32),   # products next to integers
        np.nextafter((rng.integers(-40000, 40000, n) / np.float32(32767.0)).astype(np.float32), np.float32(0)),
        (rng.standard_normal(n) * 3e4).astype(np.float32),                      # up to and beyond the wrap point
        rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32).view(np.float32),  # any bit pattern: NaNs, infinities, denormals
    ])
    special = np.array([np.nan, np.inf, -np.inf, 65538.0, np.nextafter(np.float32(65538.0), np.float32(1e9)), -65538.0, -70000.0,
                        1.0, -1.0, 0.0, -0.0, 32767.0 / 32767.0, 3.4e38, -3.4e38, 1e-45, 65537.99, 2.0, -2.0], np.float32)
    s = np.concatenate([s, special]).astype(np.float32)
    assert s.size % 18 == 0
    g = s.size // 18
    fast = np.zeros(s.size, np.int32); wrap = np.zeros(s.size, np.int32); exact = np.zeros(s.size, np.int32)
    with np.errstate(all="ignore"):
        emul.emul_pcm_convert18(_p(s), g, _p(fast), _p(wrap), _p(exact))
    assert np.array_equal(wrap, exact)
    ok = ~(s > np.float32(65538.0))                     # NaNs stay in: the fast form must get them right by itself
    assert np.array_equal(fast[ok], exact[ok])
    assert (exact[np.isnan(s)] == -32767).all() and (fast[np.isnan(s)] == -32767).all()


# ---- the composite stream (corpus.composite): every kind of frame the launch logic tells apart, in one stream ----------
# The CPU twin of tests/test_gpu_launch_shapes.py: the kernels' source on the host in every form -- chunks of many lengths
# (the rare / ordinary copy per chunk by chunk_is_rare, as on the device), the granule form with every line-table hint and
# with every far wait given up, float PCM -- against the oracle, into sentinel-filled buffers, bit-identical to each other.
COMPOSITE_FRAMES = 1066                            # one cycle of corpus.composite
COMPOSITE_SEED = 20240
RARE_CHUNK_LENGTHS = [1, 7, 61, 64, 65, 100, 257]


@pytest.fixture(scope="module")
def composite(oracle, emul):
    sp, sd, segments, rare = corpus.composite(COMPOSITE_FRAMES, COMPOSITE_SEED)
    want, want_f32 = oracle.decode_f32(sp, sd)
    whole, whole_state = _emul_into_sentinel(emul, sp, sd, "chunks", 0)
    return dict(sp=sp, sd=sd, segments=segments, rare=rare, want=want, want_f32=want_f32, whole=whole, whole_state=whole_state)


def _emul_into_sentinel(emul, sp, sd, form, arg=0, f32=False, debug=0):
    """-> (sentinel buffer decoded into, state block left behind)"""
    n = sp.shape[0]
    out = sentinel_buffer(n, f32)
    st = np.zeros(emul.emul_state_floats(), np.float32)
    if form == "chunks" and f32:
        emul.emul_decode_frames_f32(_p(sp), _p(sd), n, _p(st), _p(out), arg)
    elif form == "chunks":
        emul.emul_decode_frames(_p(sp), _p(sd), n, _p(st), _p(out), None, arg)
    else:
        emul.emul_decode_frames_granules(_p(sp), _p(sd), n, _p(st), None if f32 else _p(out), _p(out) if f32 else None, debug, arg)
    return out, st


def test_composite_holds_what_it_promises():
    """conditions on the input (no decoder involved): lone intensity-stereo frames 60 frames from any other, mono runs of
    1, 2, 66, 70 and 130 frames, one behind an intensity-stereo frame and one behind a RESET frame, every mode, the three
    rates, the ISO switches, RESET frames in mid-stream; the sparse form: fewer than one rare frame in 300"""
    sp, sd, segments, rare = corpus.composite(COMPOSITE_FRAMES, COMPOSITE_SEED)
    assert sp.shape[0] == COMPOSITE_FRAMES and segments[0][0] == 0 and segments[-1][1] == COMPOSITE_FRAMES
    assert all(a[1] == b[0] for a, b in zip(segments[:-1], segments[1:]))
    fr = sd["frame"][:, 0, 0].astype(int)
    mode, reset = (fr >> 2) & 3, (fr & 0x40) != 0
    lone = [a for a, b, label in segments if label == "is"]
    assert len(lone) == 4 and all(f in rare for f in lone)
    for f in lone:
        assert not any(0 < abs(int(r) - f) < 60 for r in rare), f
    assert sorted({(int(fr[f]) >> 4) & 3 for f in lone}) == [1, 3]
    runs = {label: (a, b) for a, b, label in segments if label.startswith("mono")}
    assert sorted(b - a for a, b in runs.values()) == [1, 2, 66, 70, 130]
    assert all((mode[a:b] == 3).all() and mode[a - 1] != 3 and mode[b] != 3 for a, b in runs.values() if b < COMPOSITE_FRAMES)
    assert runs["mono1"][0] - 1 in rare and runs["mono130"][0] - 1 in rare and reset[runs["mono66"][0] - 1]
    assert set(mode) == {0, 1, 2, 3} and set(fr & 3) == {0, 1, 2} and set(sd["iso"][:, 0, 0]) == {0, 7}
    assert reset[0] and reset[1:].sum() == 5 and not reset[[a for a, b, label in segments[1:]]].any()
    ext = [(a, b) for a, b, label in segments if label == "ext_varies"][0]
    k = np.isin(np.arange(*ext), rare)
    assert 10 <= k.sum() <= k.size - 10 and (k[1:] != k[:-1]).sum() >= 20             # rare and ordinary frames alternating
    n = 14400
    sp, sd, segments, rare = corpus.composite(n, COMPOSITE_SEED + 1, sparse=True)
    assert 20 <= rare.size < n / 300
    assert {"is", "mono1", "mono2", "mono70", "mono130", "mono66", "stereo", "dual", "ext_varies", "resets"} <= {s[2] for s in segments}


@pytest.mark.parametrize("chunk", RARE_CHUNK_LENGTHS + [0])
def test_emul_composite_chunks(emul, composite, chunk):
    c = composite
    got, st = _emul_into_sentinel(emul, c["sp"], c["sd"], "chunks", chunk)
    dmax, share = check_launch_pcm(got, c["want"], c["sd"], "chunk %d" % chunk)
    print("composite, chunks of %d: max %d LSB, %.4f %% of the samples differ" % (chunk, dmax, 100 * share))
    assert np.array_equal(got, c["whole"]), "chunks of %d: PCM differs from the whole stream as one chunk" % chunk
    assert np.array_equal(st.view(np.uint32), c["whole_state"].view(np.uint32))
    kinds = corpus.rare_chunks(c["sd"], chunk or COMPOSITE_FRAMES)
    assert chunk in (257, 0) or (kinds.any() and not kinds.all())                      # both copies of the chunk code ran


@pytest.mark.parametrize("sf_hint,debug", [(0, 0), (1, 0), (2, 0), (0, 1), (2, 1)])
def test_emul_composite_granules(emul, composite, sf_hint, debug):
    c = composite
    got, st = _emul_into_sentinel(emul, c["sp"], c["sd"], "granules", sf_hint, debug=debug)
    dmax, share = check_launch_pcm(got, c["want"], c["sd"], "granules, hint %d, debug %d" % (sf_hint, debug))
    print("composite, granule form (sf_hint %d, debug %d): max %d LSB, %.4f %% differ" % (sf_hint, debug, dmax, 100 * share))
    assert np.array_equal(got, c["whole"])
    assert np.array_equal(st.view(np.uint32), c["whole_state"].view(np.uint32))


def test_emul_composite_float_pcm(emul, composite):
    c = composite
    assert 1.0 < float(np.abs(c["want_f32"]).max()) < 1.5             # (the level the 1e-5 bar is literal at)
    outs = []
    for form, arg, debug in (("chunks", 0, 0), ("chunks", 61, 0), ("chunks", 7, 0), ("granules", 0, 0), ("granules", 1, 1)):
        got, st = _emul_into_sentinel(emul, c["sp"], c["sd"], form, arg, f32=True, debug=debug)
        dmax, _ = check_launch_pcm(got, c["want_f32"], c["sd"], "float, %s %d" % (form, arg), tol=1e-5)
        print("composite, float PCM (%s %d): max difference %.3g" % (form, arg, dmax))
        body = got[:-64].astype(np.float64)
        q = np.clip(np.trunc(body * 32767.0), -32767, 32767).astype(np.int16)
        same = q == c["whole"][:-64]
        assert same[c["whole"][:-64] != 0x5A5A].all(), "trunc(f32 * 32767) != the int16 PCM"
        assert np.array_equal(st.view(np.uint32), c["whole_state"].view(np.uint32))
        outs.append(got)
    assert all(np.array_equal(o.view(np.uint32), outs[0].view(np.uint32)) for o in outs[1:])


def _emul_rare(emul, sd, chunk):
    out = np.zeros((sd.shape[0] + chunk - 1) // chunk, np.uint8)
    emul.emul_chunk_is_rare(_p(sd), sd.shape[0], chunk, _p(out))
    return out.astype(bool)


def test_chunk_is_rare_on_the_composite(emul, composite):
    """chunk_is_rare() as a wave against corpus.rare_chunks (the rule restated): beyond its first trip of 64 frames, and
    through mono runs longer than a wave.  A false negative decodes an intensity-stereo frame without intensity stereo."""
    sd = composite["sd"]
    for chunk in RARE_CHUNK_LENGTHS:
        want = corpus.rare_chunks(sd, chunk)
        assert np.array_equal(_emul_rare(emul, sd, chunk), want), chunk
        assert want.any() and not want.all()
    sd2 = corpus.composite(5000, COMPOSITE_SEED + 1, sparse=True)[1]
    for chunk in RARE_CHUNK_LENGTHS:
        assert np.array_equal(_emul_rare(emul, sd2, chunk), corpus.rare_chunks(sd2, chunk)), chunk


def test_chunk_is_rare_one_rare_frame_around_mono_runs(emul):
    """200 random placements: joint stereo, a mono run of 0 .. 140 frames somewhere (a RESET frame in or before it now and
    then), ONE intensity-stereo frame anywhere near it.  Only the frame bytes matter to chunk_is_rare."""
    rs = np.random.RandomState(77)
    n = 420
    hits = 0
    for trial in range(200):
        sd = np.zeros((n, 2, 2), dtype=corpus.SIDE_DTYPE)
        fr = np.full(n, (corpus.MODE_JOINT << corpus.FR_MODE_SHIFT) | (2 << corpus.FR_MODEEXT_SHIFT), np.uint8)
        m = int(rs.randint(0, 141))
        a = int(rs.randint(5, n - m - 5))
        fr[a:a + m] = (corpus.MODE_MONO << corpus.FR_MODE_SHIFT) | (int(rs.randint(0, 4)) << corpus.FR_MODEEXT_SHIFT)
        near = [a - 2, a - 1, a, a + m - 1, a + m, a + m + 1]
        q = int(near[rs.randint(0, 6)] if rs.rand() < 0.6 else rs.randint(0, n))
        q = min(max(q, 0), n - 1)
        if (fr[q] >> corpus.FR_MODE_SHIFT) & 3 == corpus.MODE_JOINT:
            fr[q] |= 1 << corpus.FR_MODEEXT_SHIFT
        if rs.rand() < 0.3:
            fr[min(n - 1, max(0, a + int(rs.randint(-3, m + 3))))] |= corpus.FR_RESET
        fr[0] |= corpus.FR_RESET
        sd["frame"] = fr[:, None, None]
        for chunk in RARE_CHUNK_LENGTHS:
            want = corpus.rare_chunks(sd, chunk)
            assert np.array_equal(_emul_rare(emul, sd, chunk), want), (trial, chunk, a, m, q)
            hits += int(want.any())
    assert hits > 700
