"""The window sums of a stereo granule in the granule kernel's form -- ph_window_own, then ph_window_hist, written on register
pairs (pdmp3_amd/csrc/decode_core.h) -- against the chunk kernels' ph_window_emit on the host build, for the same slots,
history and taps (tests/host_emul/window_pairs_emul.cpp; both channels in one wave, the taps from the host tables):

  * the eighteen sums of every lane equal in every bit, and equal to the plain chain of sixteen fmaf per sum (k ascending,
    we[k] before wo[k]);
  * the history handed to the next granule equal in every bit;
  * the same chains with wo[k] before we[k] differ on these inputs, so the order is something the data can see.

Inputs: random finite slots and history at several magnitudes, slots that are zero, a history that is zero, the two
channels drawn apart.  The library is built twice: the pair form and, with -DPD_EXP_WINDOW_SCALAR, the form of before."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = {"pairs": [], "scalar": ["-DPD_EXP_WINDOW_SCALAR"]}

# name -> (magnitude of the slots, magnitude of the history); per channel: channel 1 is drawn 16 times smaller
CASES = {
    "unit": (1.0, 1.0),
    "small": (1e-3, 1e-3),
    "large": (1e4, 1e4),
    "slots_over_history": (1e2, 1e-2),
    "history_over_slots": (1e-2, 1e2),
    "tiny": (1e-30, 1e-30),
    "zero_slots": (0.0, 1.0),
    "zero_history": (1.0, 0.0),
    "all_zero": (0.0, 0.0),
}


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module", params=list(FORMS))
def lib(request):
    d = os.path.join(ROOT, "tests", "host_emul")
    so = os.path.join(d, "libwindow_pairs_emul_%s.so" % request.param)
    fma = ["-mfma"] if " fma " in open("/proc/cpuinfo").read() else []
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared"] + fma + FORMS[request.param] +
                          ["-o", so, os.path.join(d, "window_pairs_emul.cpp")])
    lib = C.CDLL(so)
    assert lib.window_pairs_emul_form() == (1 if request.param == "pairs" else 0)
    return lib


def inputs(name):
    mag_s, mag_h = CASES[name]
    rs = np.random.RandomState(20281 + sorted(CASES).index(name))
    slots = (rs.standard_normal((2, 18, 33)) * mag_s).astype(np.float32)
    he = (rs.standard_normal((15, 64)) * mag_h).astype(np.float32)
    ho = (rs.standard_normal((15, 64)) * mag_h).astype(np.float32)
    slots[1] *= np.float32(1 / 16.0)
    he[:, 32:] *= np.float32(1 / 16.0)
    ho[:, 32:] *= np.float32(1 / 16.0)
    assert np.isfinite(slots).all() and np.isfinite(he).all() and np.isfinite(ho).all()
    return slots, he, ho


def run(lib, name):
    slots, he, ho = inputs(name)
    out = dict(pcm_gran=np.full(1152, np.nan, np.float32), pcm_emit=np.full(1152, np.nan, np.float32),
               hist_gran=np.full((2, 15, 64), np.nan, np.float32), hist_emit=np.full((2, 15, 64), np.nan, np.float32),
               ref=np.full((64, 18), np.nan, np.float32), ref_swapped=np.full((64, 18), np.nan, np.float32))
    lib.window_pairs_emul(_p(slots), _p(he), _p(ho), *[_p(out[k]) for k in ("pcm_gran", "pcm_emit", "hist_gran", "hist_emit", "ref", "ref_swapped")])
    return out


def sums_of(pcm):
    """float PCM of a stereo granule (value 64 t + 2 i + ch) -> [lane = 32 ch + i][t]"""
    return np.ascontiguousarray(pcm.reshape(18, 32, 2).transpose(2, 1, 0)).reshape(64, 18)


def bits(a):
    return a.view(np.uint32)


@pytest.mark.parametrize("name", list(CASES))
def test_granule_window_sums_equal_the_chunk_form(lib, name):
    o = run(lib, name)
    assert not np.isnan(o["pcm_gran"]).any() and not np.isnan(o["pcm_emit"]).any()
    assert np.array_equal(bits(o["pcm_gran"]), bits(o["pcm_emit"])), "%s: the sums of the two forms differ" % name
    assert np.array_equal(bits(sums_of(o["pcm_gran"])), bits(o["ref"])), "%s: not the plain chains" % name
    for ch in range(2):
        assert np.array_equal(bits(sums_of(o["pcm_gran"])[32 * ch:32 * ch + 32]), bits(sums_of(o["pcm_emit"])[32 * ch:32 * ch + 32])), "channel %d" % ch


@pytest.mark.parametrize("name", list(CASES))
def test_granule_window_history_equals_the_chunk_form(lib, name):
    o = run(lib, name)
    assert not np.isnan(o["hist_gran"]).any()
    assert np.array_equal(bits(o["hist_gran"]), bits(o["hist_emit"])), "%s: the history handed on differs" % name
    slots, _, _ = inputs(name)
    if slots.any():
        assert o["hist_gran"][:, :, :32].any() and o["hist_gran"][:, :, 32:].any()


@pytest.mark.parametrize("name", [n for n in CASES if n != "all_zero"])
def test_a_reordered_sum_differs(lib, name):
    """wo[k] before we[k] is another rounding sequence: unless the data can tell, the equalities above say nothing about order"""
    o = run(lib, name)
    differ = bits(o["ref_swapped"]) != bits(o["ref"])
    print("%-20s reordered chains differ in %d of %d sums" % (name, differ.sum(), differ.size))
    assert differ[:32].any() and differ[32:].any(), "%s: the reordered sums equal the ordered ones in a channel" % name
    if CASES[name][0] and CASES[name][1]:
        assert differ.mean() > 0.25
    assert not np.array_equal(bits(sums_of(o["pcm_gran"])), bits(o["ref_swapped"]))
