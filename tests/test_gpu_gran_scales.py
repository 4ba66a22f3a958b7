"""The granule kernel's band scales from tables, its window taps in 16-byte reads and its long-only IMDCT tiles
(pdmp3_amd/csrc/decode_core.h ph_scales_tab, ph_window_own, ph_imdct_tiles; engine.hip gran_workgroup's ScaleTabs) on the device,
against the chunk kernel, which computes its scales and keeps the other form of the other two -- the batches of
tests/test_gran_scales_emul.py (scalefactors up to 15, global_gain over 0 .. 255, every block type; every global_gain 0; every
global_gain 255; levelled to the full-scale range) at 1, 2, 17 frames (workgroups of 8 waves: 17 crosses workgroup
boundaries) and the first size that takes workgroups of 16 with a ragged last one (1025 frames on 256 CUs), as int16 and
float PCM, with and without the caller's state block, with a RESET inside the batch, and all of it once more with every wait for another workgroup given up
(PDMP3_HIP_DEBUG_FAR_TIMEOUT: the frame that closes a workgroup is then decoded as a whole, gran_slow_chunk, in a workgroup
whose shared memory holds the new tables).

  * the granule launch bit for bit the chunk launch of the same records, PCM and state block: every case;
  * within the launch-shape bars of the oracle (util.check_launch_pcm: +-1 LSB, at most 2 % of the samples differing; float
    1e-5), from silence, without a RESET inside: every batch, size and PCM type, with and without the waits given up.  (The
    batches are levelled to the full-scale range -- tests/test_gran_scales_emul.py level_spectra -- so that the bars can
    hold at global_gain 255 too.)"""
import os

import numpy as np
import pytest

import corpus
from test_gpu_launch_shapes import CHUNKS, GRANULES8, GRANULES16, Sizes, launch
from test_gran_scales_emul import BATCHES, batch
from util import check_launch_pcm

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 17, "w16_from"]
SEED_STATE = 20279


class Data:
    """per batch: the records of the longest size (the shorter sizes are its first frames) on the device, a copy with a RESET
    frame inside each size; the state a launch of chunks on other frames leaves (the caller's state block); the chunk
    launches' results, computed once per case and shared by the plain and the give-up run"""

    def __init__(self, engine):
        self.engine = engine
        self.w16_from = Sizes().w16_from
        self.rec, self.dev, self.dev_inside, self.sd_inside = {}, {}, {}, {}
        for name in BATCHES:
            sp, sd = batch(name, self.w16_from)
            sd["frame"][0] &= ~np.uint8(corpus.FR_RESET)          # (so that a caller's state block is taken; without one the launch starts from silence)
            self.rec[name] = (sp, sd)
            self.dev[name] = engine.upload(sp, sd)
            for n in (1, 2, 17, self.w16_from):
                s = sd.copy()
                s["frame"][n // 2] |= np.uint8(corpus.FR_RESET)
                self.sd_inside[(name, n)] = s
                self.dev_inside[(name, n)] = engine.upload(sp, s)
        sp0, sd0 = corpus.make_frames(24, SEED_STATE, mode=corpus.MODE_JOINT, mode_ext=2, block_mix=(40, 15, 30, 15), gain_range=corpus.FS_GAIN, sf_max=15)
        self.state0 = engine.new_state()
        _, k = launch(engine, *engine.upload(sp0, sd0), 24, 7, state=self.state0)
        assert k == CHUNKS
        self._chunks = {}

    def n_of(self, size):
        return self.w16_from if size == "w16_from" else size

    def records(self, name, n, reset):
        """-> (device records, host side records) the launch of n frames reads"""
        if reset:
            return self.dev_inside[(name, n)], self.sd_inside[(name, n)]
        return self.dev[name], self.rec[name][1]

    def chunks(self, name, n, f32, with_state, reset):
        key = (name, n, f32, with_state, reset)
        if key not in self._chunks:
            (dsp, dsd), _ = self.records(name, n, reset)
            st = self.state0.clone() if with_state else None
            ref, k = launch(self.engine, dsp, dsd, n, 2 if n <= 2 else 7, f32=f32, state=st)
            assert k == CHUNKS
            ref.setflags(write=False)
            self._chunks[key] = (ref, st)
        return self._chunks[key]


@pytest.fixture(scope="module")
def data(engine):
    return Data(engine)


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
FORMS = [(False, False), (True, False), (True, True)]          # (state block, RESET inside)
FORM_IDS = ["nostate", "state", "state-reset_inside"]


def granules(eng, data, name, size, f32, with_state, reset):
    n = data.n_of(size)
    (dsp, dsd), sd = data.records(name, n, reset)
    st = data.state0.clone() if with_state else None
    got, k = launch(eng, dsp, dsd, n, 0, f32=f32, state=st)
    assert k == (GRANULES16 if size == "w16_from" else GRANULES8), "%d frames ran kind %d" % (n, k)
    return n, got, st, sd


@GIVE_UP
@pytest.mark.parametrize("with_state,reset", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("f32", [False, True], ids=["int16", "float"])
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", list(BATCHES))
def test_gpu_granule_scales_equal_the_chunk_launch(engines, data, name, size, f32, with_state, reset, give_up):
    import torch
    n, got, st, _ = granules(engines[give_up], data, name, size, f32, with_state, reset)
    what = "%s, %d frames, %s, %s%s%s" % (name, n, "float" if f32 else "int16", "state" if with_state else "no state",
                                           ", RESET at frame %d" % (n // 2) if reset else "", ", waits given up" if give_up else "")
    ref, st_c = data.chunks(name, n, f32, with_state, reset)
    assert np.array_equal(bits(got, f32), bits(ref, f32)), "%s: not the chunk launch's PCM" % what
    if with_state:
        assert torch.equal(st, st_c), "%s: the state handed on is not the chunk launch's" % what
        if name != "gain_0":
            assert not torch.equal(st, data.state0)


@pytest.fixture(scope="module")
def wanted(oracle, data):
    """the oracle's PCM from silence of each batch's first 17 frames and of all of them (no state block, no RESET inside)"""
    out = {}
    for name in BATCHES:
        sp, sd = data.rec[name]
        for n in (17, data.w16_from):
            out[(name, n)] = oracle.decode_f32(sp[:n], sd[:n])
        for n in (1, 2):
            out[(name, n)] = tuple(w[:n] for w in out[(name, 17)])
    return out


@GIVE_UP
@pytest.mark.parametrize("f32", [False, True], ids=["int16", "float"])
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", list(BATCHES))
def test_gpu_granule_scales_within_the_oracles_bars(engines, data, wanted, name, size, f32, give_up):
    n, got, _, sd = granules(engines[give_up], data, name, size, f32, False, False)
    check_launch_pcm(got, wanted[(name, n)][int(f32)], sd[:n], "%s, %d frames" % (name, n), tol=1e-5 if f32 else None)
