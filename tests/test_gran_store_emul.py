"""The granule kernel's far hand-over and its staged PCM on the host build (tests/host_emul: decode_core.h compiled by g++,
workgroups of 16 waves, so a workgroup boundary every 8 frames): a mono frame in the last frame of the first workgroup, or
in the frame before it, with stereo frames behind.  The frame that closes the workgroup is then decoded as a whole and
publishes from registers (gran_publish_regs' far branch) for the first wave of the next workgroup, which reads with
run_granule's loads; the stereo granules around it leave their PCM through pcm_emit_through (staged in LDS, stored in
16-byte pieces over exactly the granule's bytes).  PCM bit for bit the chunk decode's, int16 and
float, also with every wait for another workgroup given up; within the oracle's bars.  The device twin is
tests/test_gpu_gran_store.py."""
import numpy as np
import pytest

import corpus
from test_pipeline_emul import _p, emul_decode, emul_decode_granules
from util import check_launch_pcm, sentinel_buffer

N = 19


def mono_batch(n, mono_at, seed):
    ms = dict(mode=corpus.MODE_JOINT, mode_ext=2, block_mix=(40, 15, 30, 15), sfreq=0, gain_range=corpus.FS_GAIN, sf_max=8)
    mono = dict(mode=corpus.MODE_MONO, mode_ext=0, block_mix=(50, 15, 20, 15), sfreq=0, gain_range=corpus.FS_GAIN, sf_max=8)
    parts = [corpus.make_frames(mono_at, seed, **ms), corpus.make_frames(1, seed + 1, **mono), corpus.make_frames(n - mono_at - 1, seed + 2, **ms)]
    for _, sd in parts[1:]:
        sd["frame"][0] &= ~np.uint8(corpus.FR_RESET)
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


@pytest.mark.parametrize("debug", [0, 1], ids=["wait", "giveup"])
@pytest.mark.parametrize("mono_at", [7, 6])
def test_emul_mono_frame_closes_a_workgroup(emul, oracle, mono_at, debug):
    sp, sd = mono_batch(N, mono_at, 20260 + mono_at)
    assert np.flatnonzero(((sd["frame"][:, 0, 0] >> corpus.FR_MODE_SHIFT) & 3) == corpus.MODE_MONO).tolist() == [mono_at]
    want, want_f32 = oracle.decode_f32(sp, sd)
    # int16, into a sentinel buffer: a mono frame's second half and the guard stay untouched
    got = sentinel_buffer(N)
    st = np.zeros(emul.emul_state_floats(), np.float32)
    emul.emul_decode_frames_granules(_p(sp), _p(sd), N, _p(st), _p(got), None, debug, 0)
    check_launch_pcm(got, want, sd, "granules, mono frame %d" % mono_at)
    st_ref = np.zeros(emul.emul_state_floats(), np.float32)
    ref = emul_decode(emul, sp, sd, 0, st_ref)
    written = np.ones((N, 2304), bool)
    written[mono_at, 1152:] = False
    assert np.array_equal(got[:N * 2304].reshape(N, 2304)[written], ref[written])
    assert np.array_equal(st.view(np.uint32), st_ref.view(np.uint32))
    # float
    got32 = emul_decode_granules(emul, sp, sd, f32=True, debug=debug)
    ref32 = np.zeros((N, 2304), np.float32)
    emul.emul_decode_frames_f32(_p(sp), _p(sd), N, None, _p(ref32), 0)
    assert np.array_equal(got32.view(np.uint32), ref32.view(np.uint32))
    assert np.abs(got32[written].astype(np.float64) - want_f32[written]).max() <= 1e-5
