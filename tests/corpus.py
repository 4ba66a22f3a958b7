"""Synthetic gc-record corpora for the parity tests.

Deterministic (numpy's legacy MT19937 RandomState) so that the committed golden
fixtures (tests/golden/, made by tools/make_golden.py from the compiled
reference) can be re-derived from (name, seed) alone.

Records obey the boundary contract of include/pdmp3_hip.h: spectra are zero at
and above count1 (what the reference's Read_Huffman guarantees) and the two
out-of-bounds scalefactor slots carry what the reference's memory layout would
yield, via resolve_aliases().
"""
import numpy as np

from oracle.oracle import (SIDE_DTYPE, GC_SCALEFAC_SCALE, GC_PREFLAG, GC_WIN_SWITCH, GC_MIXED,
                           GC_BLOCK_TYPE_SHIFT, FR_MODE_SHIFT, FR_MODEEXT_SHIFT, FR_RESET, SF_PEEK)

MODE_STEREO, MODE_JOINT, MODE_DUAL, MODE_MONO = 0, 1, 2, 3


def resolve_aliases(side):
    """side: array [n][2][2] of SIDE_DTYPE with scalefac_l[:21], scalefac_s[:12] filled."""
    for f in range(side.shape[0]):
        s = side[f]
        for g in range(2):
            s[g, 0]["scalefac_l"][21] = s[g, 1]["scalefac_l"][0]
            s[g, 0]["scalefac_s"][12] = s[g, 1]["scalefac_s"][0]
        s[0, 1]["scalefac_l"][21] = s[1, 0]["scalefac_l"][0]
        s[0, 1]["scalefac_s"][12] = s[1, 0]["scalefac_s"][0]
        s[1, 1]["scalefac_l"][21] = s[0, 0]["scalefac_s"][0][0]
        s[1, 1]["scalefac_s"][12] = SF_PEEK
    return side


def make_frames(n, seed, mode=MODE_JOINT, mode_ext=2, sfreq=0, block_mix=(70, 10, 10, 10),
                mixed_prob=0.5, count1_range=(0, 576), gain_range=(120, 170), big_prob=1 / 200.0,
                max_small=15, sf_max=8, reset_every=0, zero_gc_prob=0.05, is_pos_max=8, iso=0, mode_ext_choices=None):
    """Random frames.  block_mix = percentages of block types 0,1,2,3.  mode_ext_choices: the frame's mode_extension is
    drawn from these (frames with and without intensity stereo in one stream: the kernels' two copies of their code)"""
    rs = np.random.RandomState(seed)
    spectra = np.zeros((n, 2, 2, 576), dtype=np.int16)
    side = np.zeros((n, 2, 2), dtype=SIDE_DTYPE)
    cum = np.cumsum(block_mix)
    for f in range(n):
        if mode_ext_choices is not None:
            mode_ext = int(mode_ext_choices[rs.randint(0, len(mode_ext_choices))])
        fr = (sfreq & 3) | (mode << FR_MODE_SHIFT) | (mode_ext << FR_MODEEXT_SHIFT)
        if f == 0 or (reset_every and f % reset_every == 0):
            fr |= FR_RESET
        for g in range(2):
            for c in range(2):
                s = side[f, g, c]
                s["frame"] = fr
                s["iso"] = iso
                lo, hi = count1_range
                count1 = int(rs.randint(lo, hi + 1))
                count1 -= count1 % 2
                if rs.rand() < zero_gc_prob:
                    count1 = 0 if rs.rand() < 0.5 else count1
                s["count1"] = count1
                s["global_gain"] = rs.randint(gain_range[0], gain_range[1] + 1)
                fl = 0
                if rs.rand() < 0.5:
                    fl |= GC_SCALEFAC_SCALE
                if rs.rand() < 0.5:
                    fl |= GC_PREFLAG
                pct = rs.randint(0, 100)
                bt = int(np.searchsorted(cum, pct, side="right"))
                bt = min(bt, 3)
                if bt:
                    fl |= GC_WIN_SWITCH | (bt << GC_BLOCK_TYPE_SHIFT)
                    if bt == 2 and rs.rand() < mixed_prob:
                        fl |= GC_MIXED
                s["flags"] = fl
                s["subblock_gain"] = rs.randint(0, 8, size=3)
                s["scalefac_l"][:21] = rs.randint(0, sf_max, size=21)
                s["scalefac_s"][:12] = rs.randint(0, min(sf_max, is_pos_max), size=(12, 3))
                mags = rs.randint(0, max_small + 1, size=576)
                big = rs.rand(576) < big_prob
                mags[big] = rs.randint(0, 8207, size=int(big.sum()))
                sign = rs.randint(0, 2, size=576) * 2 - 1
                v = (mags * sign).astype(np.int16)
                v[count1:] = 0
                spectra[f, g, c] = v
        if mode == MODE_MONO:
            spectra[f, :, 1] = 0
    resolve_aliases(side)
    return spectra, side


# name -> kwargs; every entry is a golden fixture (tools/make_golden.py) and a parity case
CASES = {
    "ms_long_441": dict(mode=MODE_JOINT, mode_ext=2, sfreq=0, block_mix=(100, 0, 0, 0)),
    "ms_mixed_blocks_441": dict(mode=MODE_JOINT, mode_ext=2, sfreq=0, block_mix=(40, 15, 30, 15)),
    "ms_short_heavy_480": dict(mode=MODE_JOINT, mode_ext=2, sfreq=1, block_mix=(10, 10, 70, 10), count1_range=(380, 576)),
    "stereo_plain_320": dict(mode=MODE_STEREO, mode_ext=0, sfreq=2, block_mix=(50, 15, 20, 15)),
    "dual_480": dict(mode=MODE_DUAL, mode_ext=2, sfreq=1, block_mix=(60, 10, 20, 10)),
    "mono_441": dict(mode=MODE_MONO, mode_ext=0, sfreq=0, block_mix=(50, 15, 20, 15)),
    "mono_320": dict(mode=MODE_MONO, mode_ext=2, sfreq=2, block_mix=(30, 10, 50, 10)),
    "ms_count1_skew": dict(mode=MODE_JOINT, mode_ext=2, sfreq=0, count1_range=(0, 576), zero_gc_prob=0.3),
    "ms_loud_clip": dict(mode=MODE_JOINT, mode_ext=2, sfreq=0, gain_range=(170, 215), big_prob=0.02),
    "ms_sf15": dict(mode=MODE_JOINT, mode_ext=2, sfreq=0, block_mix=(40, 15, 30, 15), sf_max=16),
    "ms_resets": dict(mode=MODE_JOINT, mode_ext=2, sfreq=0, block_mix=(40, 15, 30, 15), reset_every=3),
    # intensity stereo with is_pos <= 7 (the part of H3 that is well defined: larger values read past is_ratios[6])
    "is_long_441": dict(mode=MODE_JOINT, mode_ext=1, sfreq=0, block_mix=(100, 0, 0, 0), count1_range=(100, 500), sf_max=8),
    "ms_is_long_480": dict(mode=MODE_JOINT, mode_ext=3, sfreq=1, block_mix=(100, 0, 0, 0), count1_range=(100, 500), sf_max=8),
    # ... and on short / mixed blocks (Stereo_Process_Intensity_Short, P:2190-2220): the oracle equals oracle/_ref there
    "is_short_441": dict(mode=MODE_JOINT, mode_ext=1, sfreq=0, block_mix=(30, 10, 50, 10), count1_range=(100, 500), sf_max=8),
    "ms_is_short_480": dict(mode=MODE_JOINT, mode_ext=3, sfreq=1, block_mix=(20, 10, 60, 10), count1_range=(100, 500), sf_max=8),
}


# Twins of every case at a REALISTIC level: the cases above drive the synthesis 4x .. 150 000x
# past full scale (global_gain 120..170: 6-98 % of the samples clip), these stay below it -- |PCM| peaks 5-16 k, nothing
# clipped, median 80-1600 LSB -- so that every mode / rate / block mix meets the +-1 LSB and the 1e-5 (float) bar LITERALLY
# on a signal that is neither silent nor clipped.
FS_GAIN = (128, 140)
FS_GAIN_OF = {"ms_loud_clip": (122, 134)}         # big_prob 0.02: more linbits-sized lines, same level with less gain
CASES_FS = {name + "_fs": dict(kw, gain_range=FS_GAIN_OF.get(name, FS_GAIN)) for name, kw in CASES.items()}
ALL_CASES = dict(CASES, **CASES_FS)

# The ISO-correct switches (include/pdmp3_hip.h PDMP3_GC_ISO_*: 1 = MS on every line, 2 = intensity stereo on
# short blocks multiplies by the ratios, 4 = the rest of the standard's intensity stereo) as record corpora: the kernels
# against the oracle's restatement of the same switches.  What pins that restatement is not here: FFmpeg's decode of
# conforming packer streams, tests/golden/iso_*.npz (tests/test_iso_pin.py).
ISO_CASES = {
    "iso_ms_all_441": dict(CASES["ms_mixed_blocks_441"], iso=1, gain_range=FS_GAIN),
    "iso_ms_count1_skew": dict(CASES["ms_count1_skew"], iso=1, gain_range=FS_GAIN),
    "iso_is_short_441": dict(CASES["is_short_441"], iso=2, gain_range=FS_GAIN),
    "iso_ms_is_short_480": dict(CASES["ms_is_short_480"], iso=3, gain_range=FS_GAIN),
    "iso_ms_is_long_480": dict(CASES["ms_is_long_480"], iso=3, gain_range=FS_GAIN),
    "iso_bits_on_stereo_plain": dict(CASES["stereo_plain_320"], iso=7, gain_range=FS_GAIN),      # (no joint stereo: the bits change nothing)
    # round 6, PDMP3_GC_ISO_IS_STD (4): the whole of the standard's intensity stereo -- positions from the right channel,
    # bound by its last non-zero line (per window), last band included, no M/S on intensity-coded lines.  The two
    # channels draw their block shapes independently here: the right channel's counts, in the kernel and in the oracle
    "iso_std_is_long_441": dict(CASES["is_long_441"], iso=7, gain_range=FS_GAIN),
    "iso_std_ms_is_long_480": dict(CASES["ms_is_long_480"], iso=7, gain_range=FS_GAIN),
    "iso_std_is_short_441": dict(CASES["is_short_441"], iso=7, gain_range=FS_GAIN),
    "iso_std_ms_is_short_480": dict(CASES["ms_is_short_480"], iso=7, gain_range=FS_GAIN),
    # frames with and without intensity stereo side by side: the granule kernel sends the former down its whole-frame path
    # (like mono frames), the chunk kernel runs its RARE copy for chunks that hold one (decode_core.h frame_is_rare)
    "iso_std_ext_varies_441": dict(mode=MODE_JOINT, mode_ext=2, mode_ext_choices=(2, 2, 2, 3, 1, 0, 2), sfreq=0, block_mix=(40, 15, 30, 15),
                                   count1_range=(100, 576), sf_max=8, iso=7, gain_range=FS_GAIN),
    "ref_ext_varies_480": dict(mode=MODE_JOINT, mode_ext=2, mode_ext_choices=(2, 2, 3, 1, 0, 2, 2), sfreq=1, block_mix=(40, 15, 30, 15),
                               count1_range=(100, 500), sf_max=8, iso=0, gain_range=FS_GAIN),
    "iso_std_ms_is_mixed_320": dict(mode=MODE_JOINT, mode_ext=3, sfreq=2, block_mix=(20, 10, 60, 10), mixed_prob=0.8,
                                    count1_range=(20, 400), sf_max=8, iso=7, gain_range=FS_GAIN, zero_gc_prob=0.15),
}

# int16 tolerance per case, in LSB, as literal numbers.  +-1 LSB (north_star; P:2028-2031 is the step an LSB is defined
# by) for every case but ONE: ms_loud_clip is driven to 4.5e5 x full scale (99 % of its samples clip), where one ulp of
# the binary32 sums is 0.03 = 1000 LSB, and the few samples that come back inside the int16 range differ by up to 21 LSB
# between two f32 summation orders (measured, 64 frames, host build and GPU).
PCM_TOL_LSB = {name: 1 for name in ALL_CASES}
PCM_TOL_LSB["ms_loud_clip"] = 32
# float PCM tolerance per case, absolute, as literal numbers.  1e-5 (north_star) LITERALLY for every `_fs` case.  The
# loud cases leave the range where that bar can be met by ANY binary32 evaluation in another summation order -- their
# sums reach 19 .. 141 x full scale, one ulp there is 1.9e-6 .. 1.5e-5 -- so they carry the measured difference x 2
# (64 frames; = 1.5 .. 3.5 ulp of the case's amplitude); ms_is_short_480 has one intensity-stereo band that reaches
# 4.3e9 (ulp 512), ms_loud_clip 4.5e5 (ulp 0.031).
F32_TOL_ABS = {name: 1e-5 for name in ALL_CASES}
F32_TOL_ABS.update({"ms_long_441": 4e-5, "ms_mixed_blocks_441": 6e-5, "ms_short_heavy_480": 5e-5, "stereo_plain_320": 5e-5,
                    "dual_480": 1.1e-4, "mono_441": 7e-5, "mono_320": 8e-5, "ms_count1_skew": 1.2e-5, "ms_loud_clip": 0.16,
                    "ms_sf15": 2e-5, "ms_resets": 4e-5, "is_long_441": 5e-5, "ms_is_long_480": 8e-5, "is_short_441": 4e-5,
                    "ms_is_short_480": 1536.0})
N_GOLDEN = 64                                     # frames per golden fixture (>= 64 per block-type mix)


def case(name, n=N_GOLDEN, seed=None):
    kw = ALL_CASES[name] if name in ALL_CASES else ISO_CASES[name]
    if seed is None:
        seed = (sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) * 2654435761) & 0x7FFFFFFF
    return make_frames(n, seed, **kw)


def frame_is_rare(side):
    """per frame: does the kernels' frame_is_rare() (pdmp3_amd/csrc/decode_core.h) hold -- joint stereo with
    mode_extension bit 0 (intensity stereo), or an LSF record"""
    fr = side["frame"].reshape(side.shape[0], -1)[:, 0].astype(np.int64)
    lsf = side["lsf"].reshape(side.shape[0], -1)[:, 0].astype(np.int64)
    return (((fr >> FR_MODE_SHIFT) & 3) == MODE_JOINT) & (((fr >> FR_MODEEXT_SHIFT) & 1) != 0) | ((lsf & 3) != 0)


def composite(n_frames, seed, sparse=False):
    """One stream with every kind of frame the launch logic tells apart, for the launch-shape tests (the other corpora are
    one kind of frame each, 64 frames long).  make_frames() segments at the realistic level, joined without a reset (only
    frame 0 and the `reset_every` segment carry FR_RESET); the cycle below repeats, with other seeds, up to n_frames:

      long M/S runs of mixed block types at 44.1 and 48 kHz with LONE intensity-stereo frames in them (mode_ext 1 and 3,
      long and short blocks; at least 60 frames without intensity stereo on either side), mono runs of 1, 2, 70, 130 and 66
      frames -- the run of 1 and the run of 130 directly behind an intensity-stereo frame, the run of 66 directly behind a
      RESET frame --, plain stereo and dual channel at 32 kHz, a segment that draws mode_ext per frame with all the ISO
      switches set, a segment with a RESET every 17 frames that ends in one.  The rate changes at segment boundaries.

    sparse: the same, the M/S runs four times as long and the mode_ext-per-frame segment 8 frames, which leaves fewer than
    one frame_is_rare() frame in 300 (a big launch of chunks: most chunks ordinary, a few rare).

    -> (spectra, side, segments, rare): segments = [(first frame, end, label)], rare = indices of the frame_is_rare() frames"""
    k = 4 if sparse else 1
    ms = dict(mode=MODE_JOINT, mode_ext=2, block_mix=(40, 15, 30, 15))
    mono = dict(mode=MODE_MONO, mode_ext=0, block_mix=(50, 15, 20, 15))
    lng, sht = dict(block_mix=(100, 0, 0, 0), count1_range=(100, 500)), dict(block_mix=(10, 0, 90, 0), count1_range=(100, 500))
    cycle = [
        ("ms", 100 * k, dict(ms, sfreq=0)),
        ("is", 1, dict(lng, mode=MODE_JOINT, mode_ext=1, sfreq=0)),
        ("mono1", 1, dict(mono, sfreq=0)),
        ("ms", 70 * k, dict(ms, sfreq=0)),
        ("is", 1, dict(sht, mode=MODE_JOINT, mode_ext=3, sfreq=0)),
        ("ms", 64 * k, dict(ms, sfreq=0)),
        ("mono70", 70, dict(mono, sfreq=0)),
        ("ms", 61 * k, dict(ms, sfreq=1, block_mix=(10, 10, 70, 10), count1_range=(380, 576))),
        ("is", 1, dict(sht, mode=MODE_JOINT, mode_ext=1, sfreq=1)),
        ("ms", 62 * k, dict(ms, sfreq=1)),
        ("mono2", 2, dict(mono, sfreq=1)),
        ("ms", 60 * k, dict(ms, sfreq=1)),
        ("is", 1, dict(lng, mode=MODE_JOINT, mode_ext=3, sfreq=1)),      # (M/S + intensity stereo: channel 1 is not what plain M/S makes of it)
        ("mono130", 130, dict(mono, sfreq=1, mode_ext=2, block_mix=(30, 10, 50, 10))),
        ("stereo", 70, dict(mode=MODE_STEREO, mode_ext=0, sfreq=2, block_mix=(50, 15, 20, 15))),
        ("dual", 60, dict(mode=MODE_DUAL, mode_ext=2, sfreq=2, block_mix=(60, 10, 20, 10))),
        ("ext_varies", 8 if sparse else 100, dict(ms, sfreq=0, mode_ext_choices=(2, 2, 2, 3, 1, 0, 2), count1_range=(100, 576), iso=7)),
        ("ms", 60 * k, dict(ms, sfreq=0, iso=7)),
        ("resets", 86, dict(ms, sfreq=1, reset_every=17)),          # (86 = 5 x 17 + 1: the segment's last frame is a RESET frame)
        ("mono66", 66, dict(mono, sfreq=1)),
    ]
    sp_parts, sd_parts, segments = [], [], []
    at = i = 0
    while at < n_frames:
        label, n, kw = cycle[i % len(cycle)]
        n = min(n, n_frames - at)
        sp, sd = make_frames(n, (int(seed) * 1000003 + 7919 * i) & 0x7FFFFFFF, gain_range=FS_GAIN, sf_max=8, **kw)
        if i:
            sd["frame"][0] &= ~np.uint8(FR_RESET)
        sp_parts.append(sp)
        sd_parts.append(sd)
        segments.append((at, at + n, label))
        at += n
        i += 1
    spectra, side = np.concatenate(sp_parts), np.concatenate(sd_parts)
    return spectra, side, segments, np.flatnonzero(frame_is_rare(side))


def rare_chunks(side, chunk_frames):
    """Which chunks of a launch cut into chunks of chunk_frames frames must run the copy of the chunk code that has intensity
    stereo in it (on the device: are k_decode_rare's, not k_decode's).  The rule, restated from what a chunk decodes: its own
    frames; its halo (inside the four frames before it); and, when the frame before it is a mono frame without RESET, the
    pre-halo that fetches channel 1 from the last two-channel-or-RESET frame before that one, and the frame in front of it.
    -> bool per chunk"""
    n = side.shape[0]
    fr = side["frame"].reshape(n, -1)[:, 0].astype(np.int64)
    rare = frame_is_rare(side)
    mono = ((fr >> FR_MODE_SHIFT) & 3) == MODE_MONO
    reset = (fr & FR_RESET) != 0
    anchor = np.maximum.accumulate(np.where(~mono | reset, np.arange(n), -1))      # last two-channel-or-RESET frame <= f
    out = np.zeros((n + chunk_frames - 1) // chunk_frames, dtype=bool)
    for c in range(out.size):
        f0, f1 = c * chunk_frames, min(n, (c + 1) * chunk_frames)
        if rare[max(0, f0 - 4):f1].any():
            out[c] = True
        elif f0 >= 2 and mono[f0 - 1] and not reset[f0 - 1]:
            fs = int(anchor[f0 - 2])
            out[c] = fs >= 0 and bool(rare[fs] or (fs > 0 and rare[fs - 1]))
    return out
