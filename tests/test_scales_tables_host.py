"""The granule kernel's band scales from tables (pdmp3_amd/csrc/decode_core.h ScaleTabs, ph_scales_tab; host_tables.h builds the
tables), compiled here with g++ into tests/host_emul/scales_emul.cpp, against the form that computes them (ph_scales), which the
chunk kernels keep -- exhaustively, bit for bit on uint32 views of L.scale:

  * t1[min(n, 300)] = pow2_neg_half(n) for every n = 0 .. 2 * 400 + 2 (the clamp at 400, pretab's 2 on top, scalefac_scale's
    doubling), t2[k + 266] = pow2_quarter(k) for every k = -266 .. 45, and both against the reference's pow() expressions;
  * the lane constants: every field of the 64 dwords is what ph_scales' formulas give for that lane;
  * every lane x scalefac_scale x preflag x long / short / mixed x subblock_gain 0 .. 7 x every global_gain 0 .. 255, the
    scalefactor bytes 0, 1, 15, 16, 149, 150, 151, 200 and 255 (= PDMP3_SF_PEEK: at the H5 mark it swaps the peek value in)
    in every scalefactor place, the peek values 0, 1.0f, 3e9f (past the clamp) and NaN."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRETAB = [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 3, 2, 0]      # P:2123, [21] = 0 (H4)


@pytest.fixture(scope="module")
def lib():
    d = os.path.join(ROOT, "tests", "host_emul")
    so = os.path.join(d, "libscales_emul.so")
    fma = ["-mfma"] if " fma " in open("/proc/cpuinfo").read() else []
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared"] + fma + ["-o", so, os.path.join(d, "scales_emul.cpp")])
    lib = C.CDLL(so)
    lib.scales_emul_sweep.restype = C.c_long
    lib.scales_emul_sweep.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_long)]
    return lib


def test_tables_are_the_functions_and_the_references_pow(lib):
    assert lib.scales_emul_forms_exact() == 1, "a table entry is not the bit pattern of the reference's pow() expression"
    assert lib.scales_emul_check_tables(2 * 400 + 2) == 0


def test_lane_constants_decode_to_the_formulas(lib):
    c = np.zeros(64, np.uint32)
    lib.scales_emul_lane_consts(c.ctypes.data_as(C.c_void_p))
    for lane in range(64):
        is_long = lane < 22
        ll = lane if is_long else 21
        q = 0 if is_long else (lane - 22 if lane < 61 else 38)
        sfb, win = divmod(q, 3)
        v = int(c[lane])
        got = dict(sf_at=v & 127, sbg_at=(v >> 7) & 7, pre=(v >> 10) & 3, h5=(v >> 12) & 1, is_long=(v >> 13) & 1, win=(v >> 14) & 3,
                   ll=(v >> 16) & 31, q=(v >> 21) & 63, rest=v >> 27)
        want = dict(sf_at=8 + ll if is_long else 30 + q, sbg_at=4 + win, pre=PRETAB[ll] if is_long else 0, h5=int(sfb == 12),
                    is_long=int(is_long), win=win, ll=ll, q=q, rest=0)
        assert got == want, "lane %d" % lane


def test_table_form_equals_formula_form_everywhere(lib):
    vals = np.array([0, 1, 15, 16, 149, 150, 151, 200, 255], np.uint8)
    peeks = np.array([0.0, 1.0, 3e9, np.nan], np.float32)
    gains = np.arange(256, dtype=np.uint8)
    n = C.c_long(0)
    bad = lib.scales_emul_sweep(vals.ctypes.data_as(C.c_void_p), vals.size, peeks.ctypes.data_as(C.c_void_p), peeks.size,
                                gains.ctypes.data_as(C.c_void_p), gains.size, C.byref(n))
    assert n.value == 256 * 4 * 3 * 8 * vals.size * peeks.size * 128
    assert bad == 0, "%d of %d band scales differ between the two forms" % (bad, n.value)


def test_one_configuration_by_hand(lib):
    """the sweep's comparison is not vacuous: a record whose scales are known"""
    s = np.zeros((2, 128), np.uint8)
    s[:, 2] = 210                    # global_gain: t2 = 1
    s[0, 8:30] = 2                   # long scalefactors: 2^-(2 / 2) = 0.5
    s[1, 3] = 1                      # scalefac_scale: 2^-2
    s[1, 8:30] = 2
    s[:, 30:69] = 4                  # short: 2^-2 (2^-4 with scalefac_scale), subblock_gain 0
    pk = np.zeros(4, np.float32)
    f = np.zeros((2, 64), np.uint32)
    t = np.zeros((2, 64), np.uint32)
    lib.scales_emul_both(s[0].ctypes.data_as(C.c_void_p), s[1].ctypes.data_as(C.c_void_p), pk.ctypes.data_as(C.c_void_p),
                         f.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p))
    assert np.array_equal(f, t)
    v = t.view(np.float32)
    assert (v[0, :22] == 0.5).all() and (v[1, :22] == 0.25).all() and (v[0, 22:61] == 0.25).all() and (v[1, 22:61] == 0.0625).all()
    assert (t[:, 61:] == 0xa5a5a5a5).all(), "lanes 61 .. 63 store nothing"
