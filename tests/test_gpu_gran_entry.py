"""The granule kernel behind its own argument struct (pdmp3_amd/csrc/engine.hip k_decode_g: GranArgs, the tables at constant
offsets of one allocation, the stamped k_decode_g_prof) on the device, at the launch sizes and in the forms that reach it:

  * 1, 2 and 17 frames (workgroups of 8 waves) and the smallest launch that takes workgroups of 16 (1025 frames on 256
    CUs), cut out of corpus.composite from frame 96 on -- M/S frames, a lone intensity-stereo frame (100), a mono frame
    behind it (101), and in the long one mono runs, rate changes and RESET frames in mid-stream;
  * each as int16 and float PCM, with and without the caller's state block (the state the 96 frames before leave), with and
    without RESET on its first frame: within the launch-shape tests' bars of the oracle (+-1 LSB, at most 2 % of the samples
    differing; float 1e-5), bit-identical to a launch of chunks on the same frames, and the state block handed on equal to
    the one that launch of chunks hands on;
  * the development launch with stamps (chunk_frames = -2): a tick in every slot of every wave;
  * every wait for another workgroup given up (PDMP3_HIP_DEBUG_FAR_TIMEOUT): still the oracle's PCM."""
import ctypes as C

import numpy as np
import pytest

import corpus
from conftest import C2_SEED
from test_gpu_launch_shapes import CHUNKS, GRANULES8, GRANULES16, Sizes, kind_of, launch
from util import GUARD, check_launch_pcm

pytestmark = pytest.mark.gpu

FIRST = 96
SEED = 20242
PROF_SLOTS = 12                                    # decode_core.h kProfSlots


class Cut:
    """the composite's first FIRST + w16_from frames: records on the device, with and without RESET on frame FIRST"""

    def __init__(self, engine, oracle):
        self.oracle = oracle
        self.w16_from = Sizes().w16_from
        self.n_all = FIRST + self.w16_from
        self.sp, sd, self.segments, rare = corpus.composite(self.n_all, SEED)
        assert 100 in rare and (sd["frame"][101, 0, 0] >> corpus.FR_MODE_SHIFT) & 3 == corpus.MODE_MONO
        assert not sd["frame"][FIRST, 0, 0] & corpus.FR_RESET
        self.sd = {False: sd, True: sd.copy()}
        self.sd[True]["frame"][FIRST] |= np.uint8(corpus.FR_RESET)
        self.dev = {r: engine.upload(self.sp, self.sd[r]) for r in (False, True)}
        # the state the frames in front leave (a launch of chunks), and the oracle's PCM behind it
        self.state0 = engine.new_state()
        _, k = launch(engine, *self.dev[False], FIRST, 32, state=self.state0)
        assert k == CHUNKS
        self.want_chained = {r: oracle.decode_f32(self.sp, self.sd[r]) for r in (False, True)}
        self._alone = {}

    def want(self, n, reset, with_state, f32):
        """the oracle's PCM of frames [FIRST, FIRST + n): behind the frames in front, or from silence"""
        if with_state:
            return self.want_chained[reset][int(f32)][FIRST:FIRST + n]
        if (n, reset) not in self._alone:
            self._alone[(n, reset)] = self.oracle.decode_f32(self.sp[FIRST:FIRST + n], self.sd[reset][FIRST:FIRST + n])
        return self._alone[(n, reset)][int(f32)]


@pytest.fixture(scope="module")
def cut(engine, oracle):
    return Cut(engine, oracle)


@pytest.mark.parametrize("reset", [False, True], ids=["plain", "reset"])
@pytest.mark.parametrize("with_state", [False, True], ids=["nostate", "state"])
@pytest.mark.parametrize("f32", [False, True], ids=["int16", "float"])
@pytest.mark.parametrize("size", [1, 2, 17, "w16_from"])
def test_gpu_granule_entry_sizes_and_forms(engine, cut, size, f32, with_state, reset):
    import torch
    n = cut.w16_from if size == "w16_from" else size
    kind = GRANULES16 if size == "w16_from" else GRANULES8
    dsp, dsd = cut.dev[reset]
    sd = cut.sd[reset][FIRST:FIRST + n]
    what = "%d frames, %s, %s, %s" % (n, "float" if f32 else "int16", "state" if with_state else "no state", "RESET" if reset else "no RESET")
    st = cut.state0.clone() if with_state else None
    got, k = launch(engine, dsp, dsd, n, 0, f32=f32, state=st, first=FIRST)
    assert k == kind, "%s ran kind %d" % (what, k)
    d = check_launch_pcm(got, cut.want(n, reset, with_state, f32), sd, what, tol=1e-5 if f32 else None)
    print("%-48s kind %2d  max %s  %.4f %% of the samples differ" % (what, k, d[0], 100 * d[1]))
    # the same frames as chunks (a chunk length of 1 would be the granule kernel again)
    st_c = cut.state0.clone() if with_state else None
    ref, k = launch(engine, dsp, dsd, n, 2 if n <= 2 else 7, f32=f32, state=st_c, first=FIRST)
    assert k == CHUNKS
    assert np.array_equal(got.view(np.uint32 if f32 else np.int16), ref.view(np.uint32 if f32 else np.int16)), "%s: not the chunk launch's PCM" % what
    if with_state:
        assert torch.equal(st, st_c), "%s: the state handed on is not the chunk launch's" % what
        assert not torch.equal(st, cut.state0)


def test_gpu_granule_stamps_in_every_slot(engine):
    """chunk_frames = -2 with a profile buffer: k_decode_g_prof.  M/S frames from the generator: every wave goes the
    granule way and passes every stamp"""
    import torch
    n = 17
    lib = engine.lib
    lib.pdmp3_hip_debug_profile_phases.argtypes = [C.c_void_p] * 3 + [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    sp, sd, pcm = engine.alloc_frames(n)
    engine.generate(C2_SEED, 0, n, sp, sd)
    prof = torch.zeros((2 * n, PROF_SLOTS), dtype=torch.int64, device=engine.tdev)
    rc = lib.pdmp3_hip_debug_profile_phases(engine.h, sp.data_ptr(), sd.data_ptr(), n, pcm.data_ptr(), -2, prof.data_ptr(), None)
    assert rc == 0, lib.pdmp3_hip_last_error()
    assert kind_of(engine) == GRANULES8
    torch.cuda.synchronize()
    p = prof.cpu().numpy()
    assert (p != 0).all(), "slots without a tick: %s" % (np.argwhere(p == 0)[:8],)
    assert (p[:, 1:] >= p[:, :-1]).all(), "a wave's stamps go backwards"
    # ... and the launch decoded what the plain one decodes
    plain = torch.empty_like(pcm)
    engine.decode(sp, sd, plain, chunk_frames=1)
    assert kind_of(engine) == GRANULES8
    torch.cuda.synchronize()
    assert torch.equal(pcm, plain)


@pytest.mark.parametrize("size", [17, "w16_from"])
def test_gpu_granule_entry_far_waits_given_up(monkeypatch, cut, size):
    import pdmp3_amd
    monkeypatch.setenv("PDMP3_HIP_DEBUG_FAR_TIMEOUT", "1")
    eng = pdmp3_amd.Engine(0)
    monkeypatch.delenv("PDMP3_HIP_DEBUG_FAR_TIMEOUT")
    n = cut.w16_from if size == "w16_from" else size
    try:
        for f32 in (False, True):
            got, k = launch(eng, *cut.dev[False], n, 0, f32=f32, first=FIRST)
            assert k == (GRANULES16 if size == "w16_from" else GRANULES8)
            check_launch_pcm(got, cut.want(n, False, False, f32), cut.sd[False][FIRST:FIRST + n], "give-up path, %d frames" % n, tol=1e-5 if f32 else None)
    finally:
        eng.close()
