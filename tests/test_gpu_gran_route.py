"""The granule kernel's routing on the device: k_decode_g decides which way a wave goes from ONE gathered word per wave
(pdmp3_amd/csrc/decode_core.h GranRoute), asked for at the kernel's entry with the wave's input, its part of the tables and
its constants.  Here the granule launch must equal the chunk launch of the same records bit for bit -- PCM in a
sentinel-guarded buffer, and the closing state -- on the generator's frames with every routing fact edited in at a
workgroup's first, inner and last frame (tests/gran_route_cases.py): a mono frame, a stereo frame right after a mono one,
RESET inside the launch, an intensity-stereo frame, a record with the lsf bits set, an H5 frame, and frame 0 with a state
block, with and without RESET.

Shapes: 1, 2 and 3 frames (one workgroup of 8 waves), 5 frames (two workgroups: the far hand-over and its first wave's
routing), and the smallest launch that takes k_decode_g<*, 16> (1025 frames on 256 CUs).  Int16 and float PCM; every
shape once more with every far wait given up (PDMP3_HIP_DEBUG_FAR_TIMEOUT=1).  The chunk launches come from an engine
that never takes the granule kernels (PDMP3_HIP_CHAIN=0).  The CPU twin is tests/test_gran_route_emul.py."""
import os

import numpy as np
import pytest

import gran_route_cases
from conftest import C2_SEED
from util import GUARD, SENTINEL, SENTINEL_F32_BITS

pytestmark = pytest.mark.gpu

CHUNKS, GRANULES8, GRANULES16 = 1, 8, 16          # include/pdmp3_hip.h PDMP3_HIP_LAUNCH_*
SHAPES = ["1", "2", "3", "5", "w16_from"]


def engine_with(var, value):
    import pdmp3_amd
    old = os.environ.get(var)
    os.environ[var] = value
    try:
        return pdmp3_amd.Engine(0)
    finally:
        if old is None:
            del os.environ[var]
        else:
            os.environ[var] = old


@pytest.fixture(scope="module")
def chunk_engine(engine):
    eng = engine_with("PDMP3_HIP_CHAIN", "0")
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def timeout_engine(engine):
    eng = engine_with("PDMP3_HIP_DEBUG_FAR_TIMEOUT", "1")
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def records(engine, oracle):
    """the generator's frames for the largest shape (the smaller shapes take their first frames)"""
    import torch
    n16 = torch.cuda.get_device_properties(0).multi_processor_count * 4 + 1
    sp, sd = oracle.generate(C2_SEED, 0, n16)
    return n16, sp, sd


@pytest.fixture(scope="module")
def state0(chunk_engine, oracle):
    """the state block three frames of another stretch of the generator's stream leave: not zero"""
    import torch
    sp, sd = oracle.generate(C2_SEED, 4096, 3)
    dsp, dsd = chunk_engine.upload(sp, sd)
    st = chunk_engine.new_state()
    out = torch.empty(3 * 2304, dtype=torch.int16, device=chunk_engine.tdev)
    chunk_engine.decode(dsp, dsd, out, n_frames=3, state=st)
    torch.cuda.synchronize()
    assert float(st.abs().max()) > 0
    return st


def sentinel_tensor(eng, n, f32):
    import torch
    if f32:
        return torch.full((n * 2304 + GUARD,), SENTINEL_F32_BITS, dtype=torch.int32, device=eng.tdev).view(torch.float32)
    return torch.full((n * 2304 + GUARD,), SENTINEL, dtype=torch.int16, device=eng.tdev)


def launch(eng, dsp, dsd, n, f32, state):
    out = sentinel_tensor(eng, n, f32)
    (eng.decode_f32 if f32 else eng.decode)(dsp, dsd, out, n_frames=n, state=state, chunk_frames=0)
    return out, int(eng.lib.pdmp3_hip_last_launch_kind(eng.h))


@pytest.mark.parametrize("far_timeout", [False, True], ids=["far_wait", "far_timeout"])
@pytest.mark.parametrize("f32", [False, True], ids=["int16", "float"])
@pytest.mark.parametrize("shape", SHAPES)
def test_gpu_granule_launch_equals_chunk_launch(engine, chunk_engine, timeout_engine, records, state0, shape, f32, far_timeout):
    import torch
    n16, sp, sd = records
    n = n16 if shape == "w16_from" else int(shape)
    kind = GRANULES16 if shape == "w16_from" else GRANULES8
    eng = timeout_engine if far_timeout else engine
    dsp, _ = engine.upload(sp[:n], sd[:n])
    seen = set()
    for edit, f, esd in gran_route_cases.streams(sd[:n], kind):
        dsd = torch.from_numpy(np.ascontiguousarray(esd).view(np.uint8).reshape(n, 4, 128).copy()).to(engine.tdev)
        for with_state in (False, True):
            st_g = state0.clone() if with_state else None
            st_c = state0.clone() if with_state else None
            want, k = launch(chunk_engine, dsp, dsd, n, f32, st_c)
            assert k == CHUNKS
            got, k = launch(eng, dsp, dsd, n, f32, st_g)
            assert k == kind, "%d frames ran kind %d, the case is about kind %d" % (n, k, kind)
            what = "%s at frame %d of %d%s" % (edit, f, n, ", state block" if with_state else "")
            bits_g, bits_c = (got.view(torch.int32), want.view(torch.int32)) if f32 else (got, want)
            sent = SENTINEL_F32_BITS if f32 else SENTINEL
            assert bool((bits_g[n * 2304:] == sent).all()), "%s: written behind the last frame" % what
            assert bool((bits_c[:n * 2304] != sent).any()), "%s: the chunk launch wrote nothing" % what
            assert torch.equal(bits_g, bits_c), "%s: PCM of the granule launch != the chunk launch's" % what
            if with_state:
                assert torch.equal(st_g.view(torch.int32), st_c.view(torch.int32)), "%s: closing state differs" % what
                assert not torch.equal(st_g, state0)
        seen.add(edit)
    assert seen == {"plain"} | {e for e, needs_prev in gran_route_cases.EDITS.items() if n > 1 or not needs_prev}
