"""How the granule kernel's bytes leave it (pdmp3_amd/csrc/decode_core.h pcm_emit_through; the far block of chain_state):
the PCM of a stereo granule is staged in the wave's LDS and written through in 16-byte pieces, beside the state a
workgroup's last wave hands to the next workgroup through memory.  That changes no bit:

  * 1, 2 and 17 frames (workgroups of 8 waves: a workgroup boundary every 4 frames) and the smallest launch with
    workgroups of 16 (1025 frames on 256 CUs: a boundary every 8 frames), cut out of corpus.composite from frame 96 on,
    as int16 and float PCM, with and without the caller's state block, with and without a RESET frame INSIDE the batch:
    bit for bit the PCM of a launch of chunks on the same records, the state block handed on equal to that launch's
    (and, without the RESET, the oracle's PCM within the launch-shape tests' bars);
  * launches into pcm[lo:hi] of a larger buffer, at frame offsets: the frames' places hold the chunk launch's PCM, every
    other value of the buffer is untouched;
  * a mono frame in the last frame of a workgroup (frame 3 of 17, frame 7 of 1025) and in the frame before it, stereo
    frames behind: the frame that closes the workgroup is then decoded as a whole (gran_slow_chunk) and publishes from
    registers -- gran_publish_regs' far branch -- for the first wave of the next workgroup, which reads with run_granule's
    loads (mono in the last frame: the publisher is the mono frame; mono before it: the stereo frame behind the mono one,
    whose successor takes its state from the chain);
  * all of it once more with every wait for another workgroup given up (PDMP3_HIP_DEBUG_FAR_TIMEOUT)."""
import os

import numpy as np
import pytest

import corpus
from test_gpu_gran_entry import FIRST, Cut
from test_gpu_launch_shapes import CHUNKS, GRANULES8, GRANULES16, kind_of, launch, sentinel_tensor
from util import GUARD, SENTINEL, SENTINEL_F32_BITS, check_launch_pcm

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 17, "w16_from"]


class Data:
    """the cut of test_gpu_gran_entry.py, a copy of its records with a RESET frame inside each batch size, and the chunk
    launches' results (computed once per case, shared by the plain and the give-up run)"""

    def __init__(self, engine, oracle):
        self.engine = engine
        self.cut = Cut(engine, oracle)
        self.w16_from = self.cut.w16_from
        sd = self.cut.sd[False].copy()
        self.inside = {n: FIRST + n // 2 for n in (1, 2, 17, self.w16_from)}      # (1 frame: the frame itself)
        self.sd_inside = {}
        self.dev_inside = {}
        for n, at in self.inside.items():
            s = sd.copy()
            s["frame"][at] |= np.uint8(corpus.FR_RESET)
            self.sd_inside[n] = s
            self.dev_inside[n] = engine.upload(self.cut.sp, s)
        self._chunks = {}

    def n_of(self, size):
        return self.w16_from if size == "w16_from" else size

    def records(self, n, reset):
        return self.dev_inside[n] if reset else self.cut.dev[False]

    def chunks(self, key, dsp, dsd, n, f32, with_state, first=FIRST):
        """-> (PCM buffer, state block or None) of a launch of chunks on frames [first, first + n)"""
        key = (key, n, f32, with_state, first)
        if key not in self._chunks:
            st = self.cut.state0.clone() if with_state else None
            ref, k = launch(self.engine, dsp, dsd, n, 2 if n <= 2 else 7, f32=f32, state=st, first=first)
            assert k == CHUNKS
            ref.setflags(write=False)
            self._chunks[key] = (ref, st)
        return self._chunks[key]


@pytest.fixture(scope="module")
def data(engine, oracle):
    return Data(engine, oracle)


@pytest.fixture(scope="module")
def engines(engine):
    """False: the session's engine; True: one that gives up every wait for another workgroup"""
    import pdmp3_amd
    old = os.environ.get("PDMP3_HIP_DEBUG_FAR_TIMEOUT")
    os.environ["PDMP3_HIP_DEBUG_FAR_TIMEOUT"] = "1"
    try:
        gave_up = pdmp3_amd.Engine(0)
    finally:
        if old is None:
            del os.environ["PDMP3_HIP_DEBUG_FAR_TIMEOUT"]
        else:
            os.environ["PDMP3_HIP_DEBUG_FAR_TIMEOUT"] = old
    yield {False: engine, True: gave_up}
    gave_up.close()


def bits(a, f32):
    return a.view(np.uint32 if f32 else np.int16)


GIVE_UP = pytest.mark.parametrize("give_up", [False, True], ids=["wait", "giveup"])


@GIVE_UP
@pytest.mark.parametrize("reset", [False, True], ids=["plain", "reset_inside"])
@pytest.mark.parametrize("with_state", [False, True], ids=["nostate", "state"])
@pytest.mark.parametrize("f32", [False, True], ids=["int16", "float"])
@pytest.mark.parametrize("size", SIZES)
def test_gpu_granule_store_sizes_and_forms(engines, data, size, f32, with_state, reset, give_up):
    import torch
    eng = engines[give_up]
    n = data.n_of(size)
    dsp, dsd = data.records(n, reset)
    what = "%d frames, %s, %s, %s%s" % (n, "float" if f32 else "int16", "state" if with_state else "no state",
                                        "RESET at frame %d" % (data.inside[n] - FIRST) if reset else "no RESET", ", waits given up" if give_up else "")
    st = data.cut.state0.clone() if with_state else None
    got, k = launch(eng, dsp, dsd, n, 0, f32=f32, state=st, first=FIRST)
    assert k == (GRANULES16 if size == "w16_from" else GRANULES8), "%s ran kind %d" % (what, k)
    ref, st_c = data.chunks("cut-reset" if reset else "cut", dsp, dsd, n, f32, with_state)
    assert np.array_equal(bits(got, f32), bits(ref, f32)), "%s: not the chunk launch's PCM" % what
    if with_state:
        assert torch.equal(st, st_c), "%s: the state handed on is not the chunk launch's" % what
        assert not torch.equal(st, data.cut.state0)
    if not reset:
        check_launch_pcm(got, data.cut.want(n, False, with_state, f32), data.cut.sd[False][FIRST:FIRST + n], what, tol=1e-5 if f32 else None)


@GIVE_UP
@pytest.mark.parametrize("f32", [False, True], ids=["int16", "float"])
@pytest.mark.parametrize("lo,size", [(5, 1), (3, 17), (2, 2), (1, "w16_from")], ids=["5+1", "3+17", "2+2", "1+w16_from"])
def test_gpu_granule_store_into_slices_at_frame_offsets(engines, data, lo, size, f32, give_up):
    import torch
    eng = engines[give_up]
    n = data.n_of(size)
    total = lo + n + 3
    dsp, dsd = data.cut.dev[False]
    pcm = sentinel_tensor(eng, total * 2304 + GUARD, f32)
    out = pcm[lo * 2304:(lo + n) * 2304]
    assert out.data_ptr() % 16 == 0
    (eng.decode_f32 if f32 else eng.decode)(dsp[FIRST:FIRST + n], dsd[FIRST:FIRST + n], out, n_frames=n, chunk_frames=0)
    assert kind_of(eng) == (GRANULES16 if size == "w16_from" else GRANULES8)
    torch.cuda.synchronize()
    got = bits(pcm.cpu().numpy(), f32)
    ref, _ = data.chunks("cut", dsp, dsd, n, f32, False)
    sent = SENTINEL_F32_BITS if f32 else SENTINEL
    assert np.array_equal(got[lo * 2304:(lo + n) * 2304], bits(ref, f32)[:n * 2304]), "frames [%d, %d): not the chunk launch's PCM" % (lo, lo + n)
    assert (got[:lo * 2304] == sent).all() and (got[(lo + n) * 2304:] == sent).all(), "written outside pcm[%d:%d]" % (lo, lo + n)


def mono_batch(n, mono_at, seed):
    """n M/S frames of mixed block types with ONE mono frame at mono_at (frame 0 carries RESET, no other frame)"""
    ms = dict(mode=corpus.MODE_JOINT, mode_ext=2, block_mix=(40, 15, 30, 15), sfreq=0, gain_range=corpus.FS_GAIN, sf_max=8)
    mono = dict(mode=corpus.MODE_MONO, mode_ext=0, block_mix=(50, 15, 20, 15), sfreq=0, gain_range=corpus.FS_GAIN, sf_max=8)
    parts = [corpus.make_frames(mono_at, seed, **ms), corpus.make_frames(1, seed + 1, **mono), corpus.make_frames(n - mono_at - 1, seed + 2, **ms)]
    for _, sd in parts[1:]:
        sd["frame"][0] &= ~np.uint8(corpus.FR_RESET)
    sp, sd = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    assert np.flatnonzero(((sd["frame"][:, 0, 0] >> corpus.FR_MODE_SHIFT) & 3) == corpus.MODE_MONO).tolist() == [mono_at]
    assert not corpus.frame_is_rare(sd).any()
    return sp, sd


# (size, the mono frame): the last frame of the first workgroup, and the frame before it
MONO_CASES = [(17, 3), (17, 2), ("w16_from", 7), ("w16_from", 6)]


@pytest.fixture(scope="module")
def mono(engine, oracle, data):
    out = {}
    for i, (size, at) in enumerate(MONO_CASES):
        n = data.n_of(size)
        sp, sd = mono_batch(n, at, 20250 + 10 * i)
        out[(size, at)] = (sd, engine.upload(sp, sd), oracle.decode_f32(sp, sd))
    return out


@GIVE_UP
@pytest.mark.parametrize("f32", [False, True], ids=["int16", "float"])
@pytest.mark.parametrize("size,at", MONO_CASES, ids=["17-mono3", "17-mono2", "w16_from-mono7", "w16_from-mono6"])
def test_gpu_granule_store_mono_frame_closes_a_workgroup(engines, data, mono, size, at, f32, give_up):
    import torch
    eng = engines[give_up]
    n = data.n_of(size)
    sd, (dsp, dsd), want = mono[(size, at)]
    what = "%d frames, mono frame %d, %s%s" % (n, at, "float" if f32 else "int16", ", waits given up" if give_up else "")
    st = eng.new_state()
    got, k = launch(eng, dsp, dsd, n, 0, f32=f32, state=st)
    assert k == (GRANULES16 if size == "w16_from" else GRANULES8), "%s ran kind %d" % (what, k)
    key = ("mono", size, at)
    if (key, n, f32, True, 0) not in data._chunks:
        st_c = data.engine.new_state()
        ref, kc = launch(data.engine, dsp, dsd, n, 7, f32=f32, state=st_c)
        assert kc == CHUNKS
        ref.setflags(write=False)
        data._chunks[(key, n, f32, True, 0)] = (ref, st_c)
    ref, st_c = data._chunks[(key, n, f32, True, 0)]
    assert np.array_equal(bits(got, f32), bits(ref, f32)), "%s: not the chunk launch's PCM" % what
    assert torch.equal(st, st_c), "%s: the state handed on is not the chunk launch's" % what
    check_launch_pcm(got, want[int(f32)], sd, what, tol=1e-5 if f32 else None)
