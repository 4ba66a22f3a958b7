"""The granule kernel's own forms of three phases on the host build (decode_core.h compiled by g++, workgroups of 16 waves) against
the chunk decode, which keeps the other form of each: the band scales looked up (ph_scales_tab, the workgroup's ScaleTabs --
tests/host_emul/scales_emul.cpp hands run_granule_wave the tables the way engine.hip does) where run_chunk computes them
(ph_scales); the window taps read per lane in 16-byte pieces (ph_window_own, TabLds::taps) where run_chunk takes them from the
global table; the IMDCT tiles of a granule without short blocks fed from the long transform's fragments where they are
(ph_imdct_tiles<false>) where run_chunk goes through ph_mfma.

Batches of 19 frames (two workgroup boundaries) from corpus.make_frames: scalefactors up to 15 (long and short), global_gain
over the whole 0 .. 255, long, start, short, mixed and stop blocks in one stream (granules with and without short blocks
alternate, and H5 frames -- a short block's band 12 scaled by the peek values -- occur); one batch with every global_gain 0, one
with 255.  make_frames' spectra are at full scale near global_gain 134 (corpus.FS_GAIN); left as drawn, these batches would be
up to 1e8 times past it, where the chunk decode itself is 3-5 LSB and, in float, 1 .. 56 off the oracle (measured before the
batches were levelled: the same bits as the commit before gives).  So each granule keeps the lines with the smallest
|xr| = scale x |is|^(4/3), as many as add up to BUDGET, and loses the others (level_spectra): every gain still reaches the PCM
through the scales -- at 255 through the bands with large scalefactors, scalefac_scale and subblock_gain -- and the PCM peaks
at 0.14-0.17 of full scale (4.5-5.6 k LSB), the level of corpus.CASES_FS, where the oracle's bars hold literally.

  * PCM (int16 and float) and the state block bit for bit the chunk decode's, also with every wait for another workgroup
    given up;
  * within the oracle's bars (util.check_launch_pcm: +-1 LSB, at most 2 % of the samples differing; float 1e-5 absolute).
    On the host build: gains_0_255 and gain_255 1 LSB on 0.005 % of the samples, float 3e-8; gain_0 0 LSB, float 7e-18.
The device twin is tests/test_gpu_gran_scales.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import corpus
from test_pipeline_emul import _p, emul_decode
from util import check_launch_pcm, sentinel_buffer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 19
BATCHES = {
    "gains_0_255": dict(gain_range=(0, 255), seed=20270),
    "gain_0": dict(gain_range=(0, 0), seed=20271),
    "gain_255": dict(gain_range=(255, 255), seed=20276),      # (a seed whose last frame keeps lines in both granules: the state block is not silence)
}


SFB_LONG = np.array([0, 4, 8, 12, 16, 20, 24, 30, 36, 44, 52, 62, 74, 90, 110, 134, 162, 196, 238, 288, 342, 418, 576])   # 44.1 kHz
SFB_SHORT = np.array([0, 4, 8, 12, 16, 22, 30, 40, 52, 66, 84, 106, 136, 192])
PRETAB = np.array([0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 3, 2, 0])
LONG_BAND = np.repeat(np.arange(22), np.diff(SFB_LONG))                         # band of a line, long blocks
SHORT_BAND = np.repeat(np.arange(13), 3 * np.diff(SFB_SHORT))                   # ... short blocks, lines as Huffman-decoded: [sfb][win][j]
SHORT_WIN = np.concatenate([np.repeat(np.arange(3), w) for w in np.diff(SFB_SHORT)])
BUDGET = 0.25                                     # sum of |xr| a granule keeps, both channels together (level_spectra)


def line_scales(s):
    """the band scale of each of the 576 lines (in Huffman-decoded order) of one record, as the decoders form it, in binary64;
    the H5 band -- whose scalefactor is three PCM-dependent values -- at the largest it can be (scalefactor 0)"""
    gain, fl = int(s["global_gain"]), int(s["flags"])
    m = 1.0 if fl & corpus.GC_SCALEFAC_SCALE else 0.5
    short = bool(fl & corpus.GC_WIN_SWITCH) and ((fl >> corpus.GC_BLOCK_TYPE_SHIFT) & 3) == 2
    xl = s["scalefac_l"].astype(np.int64) + (PRETAB if fl & corpus.GC_PREFLAG else 0)
    long_sc = 2.0 ** (-m * xl[LONG_BAND]) * 2.0 ** ((gain - 210) / 4.0)
    if not short:
        return long_sc
    xs = s["scalefac_s"].astype(np.int64)[SHORT_BAND, SHORT_WIN]
    if (s["scalefac_s"][12] == corpus.SF_PEEK).any():
        xs = np.where(SHORT_BAND == 12, 0, xs)
    short_sc = 2.0 ** (-m * xs) * 2.0 ** ((gain - 210 - 8 * s["subblock_gain"].astype(np.int64)[SHORT_WIN]) / 4.0)
    if fl & corpus.GC_MIXED:
        short_sc[:36] = long_sc[:36]
    return short_sc


def level_spectra(sp, sd):
    """Brings a batch whose global_gain goes up to 255 -- full scale is near 134 for make_frames' spectra, at 255 the PCM would
    be 1e8 times that, where no two binary32 summation orders agree to an LSB -- down to a level at which the oracle's bars
    mean what they say: of every granule, the lines with the smallest |xr| = scale x |is|^(4/3) stay, as many as add up to
    BUDGET over both channels, the others are zeroed.  A granule at a moderate gain keeps all its lines; at 255 the lines of
    the bands with the smallest scales stay (large scalefactors, scalefac_scale, subblock_gain), so every gain still reaches
    the PCM through the scales.  Side records are left as they are."""
    sp = sp.copy()
    for f in range(sp.shape[0]):
        for g in range(2):
            xr = np.concatenate([line_scales(sd[f, g, c]) * np.abs(sp[f, g, c].astype(np.float64)) ** (4.0 / 3.0) for c in range(2)])
            order = np.argsort(xr, kind="stable")
            drop = order[np.cumsum(xr[order]) > BUDGET]
            flat = sp[f, g].reshape(-1)
            flat[drop] = 0
    return sp


def batch(name, n=N):
    """n M/S frames: block types 0..3 at 40 / 15 / 30 / 15 %, half of the short ones mixed, scalefactors 0 .. 14 (long and
    short), levelled (level_spectra)"""
    kw = BATCHES[name]
    sp, sd = corpus.make_frames(n, kw["seed"], mode=corpus.MODE_JOINT, mode_ext=2, sfreq=0, block_mix=(40, 15, 30, 15),
                                gain_range=kw["gain_range"], sf_max=15, is_pos_max=15)
    assert not corpus.frame_is_rare(sd).any()
    return level_spectra(sp, sd), sd


@pytest.fixture(scope="module")
def scales_emul():
    d = os.path.join(ROOT, "tests", "host_emul")
    so = os.path.join(d, "libscales_emul.so")
    fma = ["-mfma"] if " fma " in open("/proc/cpuinfo").read() else []
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared"] + fma + ["-o", so, os.path.join(d, "scales_emul.cpp")])
    return C.CDLL(so)


@pytest.fixture(scope="module")
def decoded(emul, scales_emul):
    """per (batch, debug): the table-form granule decode and the chunk decode, int16 (sentinel buffer) and float, with state"""
    out = {}

    def get(name, debug):
        if (name, debug) not in out:
            sp, sd = batch(name)
            got = sentinel_buffer(N)
            st = np.zeros(emul.emul_state_floats(), np.float32)
            scales_emul.scales_emul_decode_frames_granules(_p(sp), _p(sd), N, _p(st), _p(got), None, debug, 0)
            st_ref = np.zeros(emul.emul_state_floats(), np.float32)
            ref = emul_decode(emul, sp, sd, 0, st_ref)
            got32 = sentinel_buffer(N, f32=True)
            st32 = np.zeros(emul.emul_state_floats(), np.float32)
            scales_emul.scales_emul_decode_frames_granules(_p(sp), _p(sd), N, _p(st32), None, _p(got32), debug, 0)
            ref32 = np.zeros((N, 2304), np.float32)
            st32_ref = np.zeros(emul.emul_state_floats(), np.float32)
            emul.emul_decode_frames_f32(_p(sp), _p(sd), N, _p(st32_ref), _p(ref32), 0)
            out[(name, debug)] = dict(sd=sd, got=got, st=st, ref=ref, st_ref=st_ref, got32=got32, st32=st32, ref32=ref32, st32_ref=st32_ref)
        return out[(name, debug)]
    return get


def test_batches_hold_what_they_are_for():
    sp, sd = batch("gains_0_255")
    fl = sd["flags"].reshape(N, 2, 2)
    short = ((fl & corpus.GC_WIN_SWITCH) != 0) & (((fl >> corpus.GC_BLOCK_TYPE_SHIFT) & 3) == 2)
    any_short = short.any(axis=2)
    assert any_short.any() and (~any_short).any(), "granules with and without short blocks"
    assert (short & ((fl & corpus.GC_MIXED) != 0)).any(), "mixed blocks"
    assert short[:, 1, 1].any() and (sd["scalefac_s"][:, 1, 1, 12] == corpus.SF_PEEK).all(), "H5 frames"
    assert sd["scalefac_l"][..., :21].max() == 14 and sd["scalefac_s"][..., :12, :].max() == 14
    kept = (sp != 0).reshape(N * 2, -1).sum(axis=1)
    loud = (sd["global_gain"].reshape(N * 2, 2) > 200).all(axis=1)
    assert loud.any() and (kept[loud] > 0).any(), "granules at the top gains that still carry lines"
    g = sd["global_gain"]
    assert g.min() < 16 and g.max() > 240
    assert (batch("gain_0")[1]["global_gain"] == 0).all() and (batch("gain_255")[1]["global_gain"] == 255).all()


@pytest.mark.parametrize("debug", [0, 1], ids=["wait", "giveup"])
@pytest.mark.parametrize("name", list(BATCHES))
def test_emul_table_form_granules_equal_chunks(decoded, name, debug):
    d = decoded(name, debug)
    assert np.array_equal(d["got"][:N * 2304].reshape(N, 2304), d["ref"]), "%s: not the chunk decode's PCM" % name
    assert np.array_equal(d["st"].view(np.uint32), d["st_ref"].view(np.uint32)), "%s: not the chunk decode's state" % name
    assert np.array_equal(d["got32"][:N * 2304].view(np.uint32).reshape(N, 2304), d["ref32"].view(np.uint32)), "%s: not the chunk decode's float PCM" % name
    assert np.array_equal(d["st32"].view(np.uint32), d["st32_ref"].view(np.uint32)), "%s: not the chunk decode's state (float launch)" % name
    if name != "gain_0":
        assert np.abs(d["ref"]).max() > 0 and d["st"].any()


@pytest.fixture(scope="module")
def wanted(oracle):
    return {name: oracle.decode_f32(*batch(name)) for name in BATCHES}


@pytest.mark.parametrize("debug", [0, 1], ids=["wait", "giveup"])
@pytest.mark.parametrize("name", list(BATCHES))
def test_emul_table_form_granules_within_the_oracles_bars(decoded, wanted, name, debug):
    d = decoded(name, debug)
    want, want_f32 = wanted[name]
    dmax = np.abs(d["got32"][:N * 2304].reshape(N, 2304).astype(np.float64) - want_f32).max()
    di = np.abs(d["got"][:N * 2304].reshape(N, 2304).astype(np.int32) - want.astype(np.int32))
    print("%-12s int16: max %d LSB, %.4f %% differ; float: max %g at a peak of %g" % (name, di.max(), 100 * (di > 0).mean(), dmax, np.abs(want_f32).max()))
    check_launch_pcm(d["got"], want, d["sd"], "granules, %s" % name)
    check_launch_pcm(d["got32"], want_f32, d["sd"], "granules, %s, float" % name, tol=1e-5)
