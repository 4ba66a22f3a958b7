"""The granule kernel's window sums on register pairs (pdmp3_amd/csrc/decode_core.h ph_window_own / ph_window_hist) on the
device, against the chunk kernel, which keeps its own form (ph_window_emit) -- on records that mix long, start, short, mixed
and stop blocks, so that the IMDCT tiles' rows 0, 1 of mixed blocks and the inverted subbands of the overlap stage, whose
arithmetic sits between the same matrix instructions, are in the batch too -- at 1, 2, 17 frames (workgroups of 8 waves: 17
crosses workgroup boundaries) and the first size that takes workgroups of 16 with a ragged last one (1025 frames on 256 CUs),
as int16 and float PCM, with and without the caller's state block, and with a RESET inside the batch.

  * the granule launch bit for bit the chunk launch of the same records, PCM and state block: every case;
  * within the launch-shape bars of the oracle (util.check_launch_pcm: +-1 LSB, at most 2 % of the samples differing; float
    1e-5): every case too -- with the caller's state block against the tail of the oracle's decode of the 24 frames that
    state came from followed by the launch's records.

The host twin of the window sums is tests/test_window_pairs_emul.py."""
import numpy as np
import pytest

import corpus
from test_gpu_launch_shapes import CHUNKS, GRANULES8, GRANULES16, Sizes, launch
from util import check_launch_pcm

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 17, "w16_from"]
SEED, SEED_STATE = 20282, 20283


def records(n):
    """n M/S frames at the full-scale level: block types 0..3 at 40 / 15 / 30 / 15 %, half of the short ones mixed"""
    sp, sd = corpus.make_frames(n, SEED, mode=corpus.MODE_JOINT, mode_ext=2, sfreq=0, block_mix=(40, 15, 30, 15), gain_range=corpus.FS_GAIN, sf_max=15)
    assert not corpus.frame_is_rare(sd).any()
    return sp, sd


def block_facts(sd):
    """per (frame, granule, channel): block type (0 without window switching), mixed"""
    fl = sd["flags"].reshape(-1, 2, 2)
    wsf = (fl & corpus.GC_WIN_SWITCH) != 0
    bt = np.where(wsf, (fl >> corpus.GC_BLOCK_TYPE_SHIFT) & 3, 0)
    return bt, wsf & ((fl & corpus.GC_MIXED) != 0)


def test_gpu_pairs_batch_holds_what_it_is_for():
    for n in (17, Sizes().w16_from):
        bt, mixed = block_facts(records(n)[1])
        assert mixed[:, :, 0].any() and mixed[:, :, 1].any(), "a mixed block in each channel"
        assert (bt[:, :, 0] != bt[:, :, 1]).any(), "a granule whose channels differ in block type"
        assert all((bt == t).any() for t in range(4)), "every block type"
        any_short = (bt == 2).any(axis=2)
        assert any_short.any() and (~any_short).any(), "granules with and without short blocks (both copies of the IMDCT tiles)"
    bt, mixed = block_facts(records(2)[1])
    assert (bt == 2).any() and (bt != 2).any(), "the smallest launches hold short and long blocks"


class Data:
    """the records of the longest size (the shorter sizes are its first frames) on the device, a copy with a RESET frame
    inside each size; the state a launch of chunks on other frames leaves (the caller's state block); the chunk launches'
    results, computed once per case"""

    def __init__(self, engine):
        self.engine = engine
        self.w16_from = Sizes().w16_from
        sp, sd = records(self.w16_from)
        sd["frame"][0] &= ~np.uint8(corpus.FR_RESET)          # (so that a caller's state block is taken; without one the launch starts from silence)
        self.rec = (sp, sd)
        self.dev = engine.upload(sp, sd)
        self.dev_inside, self.sd_inside = {}, {}
        for n in (1, 2, 17, self.w16_from):
            s = sd.copy()
            s["frame"][n // 2] |= np.uint8(corpus.FR_RESET)
            self.sd_inside[n] = s
            self.dev_inside[n] = engine.upload(sp, s)
        sp0, sd0 = self.rec0 = corpus.make_frames(24, SEED_STATE, mode=corpus.MODE_JOINT, mode_ext=2, block_mix=(40, 15, 30, 15), gain_range=corpus.FS_GAIN, sf_max=15)
        self.state0 = engine.new_state()
        _, k = launch(engine, *engine.upload(sp0, sd0), 24, 7, state=self.state0)
        assert k == CHUNKS
        self._chunks = {}

    def n_of(self, size):
        return self.w16_from if size == "w16_from" else size

    def records(self, n, reset):
        """-> (device records, host side records) the launch of n frames reads"""
        if reset:
            return self.dev_inside[n], self.sd_inside[n]
        return self.dev, self.rec[1]

    def chunks(self, n, f32, with_state, reset):
        key = (n, f32, with_state, reset)
        if key not in self._chunks:
            (dsp, dsd), _ = self.records(n, reset)
            st = self.state0.clone() if with_state else None
            ref, k = launch(self.engine, dsp, dsd, n, 2 if n <= 2 else 7, f32=f32, state=st)
            assert k == CHUNKS
            ref.setflags(write=False)
            self._chunks[key] = (ref, st)
        return self._chunks[key]


@pytest.fixture(scope="module")
def data(engine):
    return Data(engine)


def bits(a, f32):
    return a.view(np.uint32 if f32 else np.int16)


FORMS = [(False, False), (True, False), (True, True)]          # (state block, RESET inside)
FORM_IDS = ["nostate", "state", "state-reset_inside"]


def granules(eng, data, size, f32, with_state, reset):
    n = data.n_of(size)
    (dsp, dsd), sd = data.records(n, reset)
    st = data.state0.clone() if with_state else None
    got, k = launch(eng, dsp, dsd, n, 0, f32=f32, state=st)
    assert k == (GRANULES16 if size == "w16_from" else GRANULES8), "%d frames ran kind %d" % (n, k)
    return n, got, st, sd


@pytest.mark.parametrize("with_state,reset", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("f32", [False, True], ids=["int16", "float"])
@pytest.mark.parametrize("size", SIZES)
def test_gpu_granule_pairs_equal_the_chunk_launch(engine, data, size, f32, with_state, reset):
    import torch
    n, got, st, _ = granules(engine, data, size, f32, with_state, reset)
    what = "%d frames, %s, %s%s" % (n, "float" if f32 else "int16", "state" if with_state else "no state",
                                     ", RESET at frame %d" % (n // 2) if reset else "")
    ref, st_c = data.chunks(n, f32, with_state, reset)
    assert np.abs(ref[:n * 2304]).max() > 0
    assert np.array_equal(bits(got, f32), bits(ref, f32)), "%s: not the chunk launch's PCM" % what
    if with_state:
        assert torch.equal(st, st_c), "%s: the state handed on is not the chunk launch's" % what
        assert not torch.equal(st, data.state0)


@pytest.fixture(scope="module")
def wanted(oracle, data):
    """(size in frames, state block, RESET inside) -> the oracle's PCM (int16, float) of that launch.  From silence: of the
    records themselves (the shorter sizes without a RESET inside are the first frames of the 17).  With the caller's state
    block: the tail of ONE decode of the 24 frames that state came from followed by the launch's records -- the state block
    is what the stream so far leaves behind; a RESET frame inside is decoded as the oracle decodes it in mid-stream"""
    sp, sd = data.rec
    sp0, sd0 = data.rec0
    out = {}
    for n in (1, 2, 17, data.w16_from):
        for with_state, reset in FORMS:
            side = (data.sd_inside[n] if reset else sd)[:n]
            if with_state:
                w = oracle.decode_f32(np.concatenate([sp0, sp[:n]]), np.concatenate([sd0, side]))
                out[(n, with_state, reset)] = tuple(x[len(sp0):] for x in w)
            elif n <= 2:
                continue
            else:
                out[(n, with_state, reset)] = oracle.decode_f32(sp[:n], side)
    for n in (1, 2):
        out[(n, False, False)] = tuple(w[:n] for w in out[(17, False, False)])
    return out


@pytest.mark.parametrize("with_state,reset", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("f32", [False, True], ids=["int16", "float"])
@pytest.mark.parametrize("size", SIZES)
def test_gpu_granule_pairs_within_the_oracles_bars(engine, data, wanted, size, f32, with_state, reset):
    n, got, _, sd = granules(engine, data, size, f32, with_state, reset)
    what = "%d frames, %s%s" % (n, "state" if with_state else "no state", ", RESET at frame %d" % (n // 2) if reset else "")
    check_launch_pcm(got, wanted[(n, with_state, reset)][int(f32)], sd[:n], what, tol=1e-5 if f32 else None)
