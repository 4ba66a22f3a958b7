"""The granule kernel's routing word -- one byte per lane, one predicate per lane, one ballot (pdmp3_amd/csrc/decode_core.h:
GranRoute, gran_route_offset, gran_route_pred) -- against the expressions run_granule_wave, run_granule and
frame_is_rare() decided from before it, kept verbatim in tests/host_emul/gran_route_emul.cpp.

A stand-alone program built from the kernel's own header: for each of the frames f - 1, f, f + 1 every combination of mode,
mode_extension bit 0, RESET and the lsf version bits; times the H5 flag of record (f, 1, 1) (and, on a subset, all 256
values of that byte), the granule of the frame, f first / middle / last of a launch of three and the only frame of a
launch of one, and a state block or none.  Every fact the wave routes by -- stereo, fresh, prev_stereo, the three rare
flags, h5, next_takes, from_caller -- must be equal, and no lane of the gather may read outside the launch's records."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import gran_route_cases
from conftest import C2_SEED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("n,debug", [(1, 0), (2, 0), (3, 0), (5, 0), (9, 0), (9, 1)])
def test_emul_granule_launch_equals_chunk_launch_on_edited_records(emul, oracle, n, debug):
    """the CPU twin of tests/test_gpu_gran_route.py on the host build of the kernels (workgroups of 16 waves: 9 frames are two
    of them): the generator's frames with each routing fact planted at a workgroup's first, inner and last frame, decoded
    through a state block the granule way and in independent chunks -- PCM and closing state equal in every bit;
    debug = 1: every wait for another workgroup given up"""
    sp, sd = oracle.generate(C2_SEED, 0, n)
    st0 = np.zeros(emul.emul_state_floats(), np.float32)
    sp0, sd0 = oracle.generate(C2_SEED, 4096, 3)
    emul.emul_decode_frames(_p(sp0), _p(sd0), 3, _p(st0), _p(np.zeros((3, 2304), np.int16)), None, 0)
    assert np.abs(st0).max() > 0
    seen = set()
    for edit, f, esd in gran_route_cases.streams(sd, 16):
        st_c, st_g = st0.copy(), st0.copy()
        want, got = np.zeros((n, 2304), np.int16), np.zeros((n, 2304), np.int16)
        emul.emul_decode_frames(_p(sp), _p(esd), n, _p(st_c), _p(want), None, 0)
        emul.emul_decode_frames_granules(_p(sp), _p(esd), n, _p(st_g), _p(got), None, debug, 0)
        assert np.array_equal(got, want), "%s at frame %d of %d" % (edit, f, n)
        assert np.array_equal(st_g.view(np.uint32), st_c.view(np.uint32)), "%s at frame %d of %d: closing state" % (edit, f, n)
        seen.add(edit)
    assert seen == {"plain"} | {e for e, needs_prev in gran_route_cases.EDITS.items() if n > 1 or not needs_prev}


def test_route_word_equals_the_expressions_of_before():
    d = os.path.join(ROOT, "tests", "host_emul")
    exe = os.path.join(d, "gran_route_emul")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unused-function", "-o", exe,
                           os.path.join(d, "gran_route_emul.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stderr
    m = re.match(r"cases (\d+) mismatches (\d+)", r.stdout)
    # three frames x 64 cases each, x 2 flags x 2 granules x 2 states in the middle position alone
    assert m and int(m.group(2)) == 0 and int(m.group(1)) >= 64 ** 3 * 8
