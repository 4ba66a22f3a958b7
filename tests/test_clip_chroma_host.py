"""Chroma features of clips, the part that needs no GPU: the planning calls of
pdmp3_amd/host/clip_chroma.c against the restatement tests/clip_chroma_ref.py, every refusal, the plan over all hops, and
k_clip_chroma's own indexing and arithmetic (pdmp3_amd/csrc/chroma_core.h over cqt_core.h, compiled here with g++ into
tests/host_emul/chroma_emul.cpp's loops) on random float32 rows: bit-equal to the sequential binary32 fold of the constant-Q
emulator's output, and within the derived binary32 bound of the binary64 definition -- no value left out.

The LDS of a workgroup, restated from include/pdmp3_bulk.h: the span | the eight waves' partial sums (4352 floats) | the q plane
[n_bins rounded up to 16][17]; the folded classes [n_chroma][17] lie OVER the partial sums, behind the barrier that follows
their last read."""
import ctypes as C
import functools

import numpy as np
import pytest

import clip_chroma_ref as ref
import clip_cqt_ref as cref
import test_clip_cqt_host as tch
from clip_host import build_emul, run_sanitizer_program

U = ref.U
C1, C2, C3 = ref.FMIN_C1, ref.FMIN_C2, ref.FMIN_C3
NORM_NAMES = {0: None, 1: "l1", 2: "l2", 3: "max"}


class ChromaParams(C.Structure):                   # include/pdmp3_hip.h pdmp3_chroma_params
    _fields_ = [("cqt", tch.CqtParams), ("n_chroma", C.c_int32), ("r", C.c_int32), ("base_class", C.c_int32), ("chroma_norm", C.c_int32),
                ("norm_floor", C.c_float), ("q_at", C.c_uint32), ("class_at", C.c_uint32)]


# the specs of the GPU cases (tests/test_gpu_clip_chroma.py): sampling frequency, the geometry, the hop
GPU_SPECS = {
    "a": (22050, dict(fmin=C1, n_bins=84, bins_per_octave=12), 512),
    "b": (16000, dict(fmin=1000.0, n_bins=24, bins_per_octave=12), 160),
    "c": (22050, dict(fmin=C3, n_bins=108, bins_per_octave=36), 512),
    "d": (16000, dict(fmin=1000.0, n_bins=17, bins_per_octave=12), 160),
    "e": (44100, dict(fmin=C1, n_bins=24, bins_per_octave=12), 1024),
}


def _emul():
    lib = build_emul("chroma")
    lib.emul_clip_chroma.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p]
    assert lib.emul_chroma_desc_bytes() == C.sizeof(tch.MelDesc) and lib.emul_chroma_params_bytes() == C.sizeof(ChromaParams)
    return lib


@pytest.mark.parametrize("n_bins", [1, 16, 17, 84, 108])
@pytest.mark.parametrize("b", [12, 24, 36, 96])
def test_map_and_counts_are_the_restatement(b, n_bins):
    """every base_class at n_chroma in {1, 12, 24, B} (those that divide B): the class of every bin and the bins of every class,
    partial octaves and classes without a bin included; the kernel's own map (chroma_core.h) beside the host's"""
    from pdmp3_amd import api
    lib = _emul()
    sr = 48000                                     # (108 bins at 12 an octave from C1 end at 15.8 kHz)
    fmin = C1 if b == 12 else sr / (12000.0 * (2.0 ** (1.0 / b) - 1.0))      # (the longest filter about 12 000 taps: the table stays small)
    geo = dict(fmin=fmin, n_bins=n_bins, bins_per_octave=b)
    assert api.cqt_check(sr, **geo)
    empty = partial = 0
    for n_chroma in sorted({1, 12, 24, b}):
        if b % n_chroma:
            assert not api.chroma_check(sr, n_chroma=n_chroma, **geo)
            continue
        r = b // n_chroma
        for base in range(n_chroma):
            cls, count = api.chroma_map(sr, n_chroma=n_chroma, base_class=base, **geo)
            want, wcount = ref.class_map(n_bins, b, n_chroma, base)
            assert np.array_equal(cls, want) and np.array_equal(count, wcount) and count.sum() == n_bins and len(count) == n_chroma
            assert cls[0] == base % n_chroma
            assert all(lib.emul_chroma_class(k, r, base, n_chroma) == want[k] for k in range(0, n_bins, max(1, n_bins // 9)))
            empty += int((count == 0).sum())
            partial += int(count.max() != count.min())
        if r == 3 and n_bins >= 3:
            # the centring: class p collects bins 3 p - 1, 3 p, 3 p + 1 -- bins 0 and 1 in class 0, bin 2 already in class 1
            cls, _ = api.chroma_map(sr, n_chroma=n_chroma, **geo)
            assert list(cls[:3]) == [0, 0, 1 % n_chroma]
            if n_bins == 108 and n_chroma == 12:
                assert cls[107] == 0 and 107 // 3 % 12 == 11
    if n_bins < b:
        assert empty > 0
    if n_bins % b:
        assert partial > 0


def test_the_defaults_and_the_octaves_that_fit():
    """36 bins an octave from C1 at 22 050 Hz is refused by the constant-Q transform's own limit (N_0 = 34 683 > 32 767); 36 from
    C2 and 24 from C1 are planned"""
    from pdmp3_amd import api
    assert api.chroma_check() and api.chroma_plan() == ref.plan(22050, 512)[:8] == (16, 2, 102064, 512, 8, 4, 23884, 19532)
    cls, count = api.chroma_map()
    assert list(cls[:13]) == list(range(12)) + [0] and list(count) == [7] * 12
    g36 = dict(n_bins=108, bins_per_octave=36)
    assert 2 * int(cref.lengths(22050, fmin=C1, **g36)[2][0]) + 1 == 34683 > cref.MAX_LEN
    assert not api.cqt_check(22050, fmin=C1, **g36) and not api.chroma_check(22050, fmin=C1, **g36)
    assert 2 * int(cref.lengths(22050, fmin=C2, **g36)[2][0]) + 1 == 17341
    assert api.chroma_check(22050, fmin=C2, **g36) and api.chroma_plan(22050, fmin=C2, **g36) == ref.plan(22050, 512, fmin=C2, **g36)[:8]
    g24 = dict(n_bins=84, bins_per_octave=24)
    assert 2 * int(cref.lengths(22050, fmin=C1, **g24)[2][0]) + 1 == 23011
    assert api.chroma_check(22050, fmin=C1, **g24) and api.chroma_plan(22050, fmin=C1, **g24) == ref.plan(22050, 512, fmin=C1, **g24)[:8]


def _raw(lib, name, spec, sr, *args):
    return getattr(lib, name)(C.byref(spec) if spec is not None else None, int(sr), *args)


def test_refusals_of_the_planning_calls():
    from pdmp3_amd import api
    lib = api.load_library()
    sr = 22050
    assert api.chroma_check(sr)
    ok = [dict(n_chroma=1), dict(n_chroma=96, bins_per_octave=96, fmin=200.0), dict(n_chroma=6), dict(base_class=11), dict(n_chroma=1, base_class=0),
          dict(chroma_norm=0), dict(chroma_norm=3), dict(chroma_norm="l1"), dict(chroma_norm="l2"), dict(chroma_norm=None), dict(quantity="power"),
          dict(quantity=1), dict(norm_floor=1.2e-38), dict(norm_floor=3e38), dict(chroma_norm=None, norm_floor=0.0),
          dict(chroma_norm=0, norm_floor=float("nan")), dict(n_frames=0)]
    for good in ok:
        assert api.chroma_check(sr, **good), good
    refused = [dict(n_chroma=0), dict(n_chroma=-1), dict(n_chroma=97, bins_per_octave=97, fmin=200.0), dict(n_chroma=5), dict(n_chroma=24),
               dict(n_chroma=192, bins_per_octave=96, fmin=200.0), dict(base_class=-1), dict(base_class=12), dict(n_chroma=1, base_class=1),
               dict(chroma_norm=-1), dict(chroma_norm=4), dict(chroma_norm="l3"), dict(quantity="complex"), dict(quantity="log"), dict(quantity="log10"),
               dict(quantity=-1), dict(quantity=5), dict(norm_floor=0.0), dict(norm_floor=-1e-10), dict(norm_floor=1e-46), dict(norm_floor=1.1e-38),
               dict(norm_floor=3.5e38), dict(norm_floor=float("nan")), dict(norm_floor=float("inf")), dict(n_frames=-1),
               # whatever the constant-Q transform's check refuses
               dict(n_bins=0), dict(bins_per_octave=0), dict(fmin=0.0), dict(fmin=5.0), dict(fmin=7600.0), dict(hop=0), dict(hop=8193), dict(norm=3),
               dict(scale=-1), dict(filter_scale=0.0)]
    for bad in refused:
        assert not api.chroma_check(sr, **bad), bad
    assert not api.chroma_check(0) and not api.chroma_check(-1)
    # a spec for which the plan finds no tile although the constant-Q transform's does: the q plane is what is missing
    geo = dict(fmin=C1, n_bins=24, bins_per_octave=12)
    only_cqt = [h for h in range(1, 8193) if cref.plan(44100, h, **geo) is not None and ref.plan(44100, h, **geo) is None]
    assert only_cqt, "no hop at which the q plane alone is too much"
    for h in (only_cqt[0], only_cqt[-1]):
        assert api.cqt_check(44100, hop=h, **geo) and not api.chroma_check(44100, hop=h, **geo)
    # nothing is written: refused specs, NULL pointers, a short cap
    good = api._chroma_spec(sample_rate=sr)
    cls = np.full(84, -7, dtype=np.int32)
    count = np.full(12, -7, dtype=np.int32)
    ints = [C.c_int(-7) for _ in range(5)]
    uints = [C.c_uint(7) for _ in range(3)]

    def untouched():
        return (cls == -7).all() and (count == -7).all() and all(i.value == -7 for i in ints) and all(u.value == 7 for u in uints)
    plan_args = (C.byref(ints[0]), C.byref(ints[1]), C.byref(uints[0]), C.byref(ints[2]), C.byref(ints[3]), C.byref(ints[4]), C.byref(uints[1]),
                 C.byref(uints[2]))
    for spec in (api._chroma_spec(sample_rate=sr, n_chroma=5), api._chroma_spec(sample_rate=sr, quantity=0), api._chroma_spec(sample_rate=sr, n_bins=0),
                 None):
        assert _raw(lib, "pdmp3_amd_chroma_check", spec, sr) == -1
        assert _raw(lib, "pdmp3_amd_chroma_map", spec, sr, cls.ctypes.data, 84, count.ctypes.data) == -1
        assert _raw(lib, "pdmp3_amd_chroma_plan", spec, sr, *plan_args) == -1
        assert untouched()
    assert _raw(lib, "pdmp3_amd_chroma_map", good, sr, cls.ctypes.data, 83, count.ctypes.data) == -1
    assert _raw(lib, "pdmp3_amd_chroma_map", good, 0, cls.ctypes.data, 84, count.ctypes.data) == -1
    assert untouched()
    # NULL outputs are allowed
    assert _raw(lib, "pdmp3_amd_chroma_map", good, sr, None, 0, None) == 84
    assert _raw(lib, "pdmp3_amd_chroma_plan", good, sr, *([None] * 8)) == 0
    assert untouched()
    assert _raw(lib, "pdmp3_amd_chroma_map", good, sr, cls.ctypes.data, 84, count.ctypes.data) == 84
    assert list(count) == [7] * 12 and (cls >= 0).all()
    for kw in (dict(n_chroma=0), dict(n_chroma=5), dict(quantity="log")):
        for call in (api.chroma_map, api.chroma_plan):
            with pytest.raises(ValueError):
                call(sr, **kw)


@pytest.mark.parametrize("case", sorted(GPU_SPECS))
def test_the_plan_is_the_restatement_over_all_hops(case):
    """hops 1 .. 8192 at the specs of the GPU cases: the call's plan is the restated one at every hop -- so on both sides of every
    threshold between two tiles and of the 64 KB edge -- and keeps the kernel's preconditions"""
    from pdmp3_amd import api
    sr, geo, _ = GPU_SPECS[case]
    rows, _ = cref.tiles(sr, **geo)
    n16 = len(rows) * 16
    paths, edges, prev, smaller = {}, [], None, 0
    for hop in range(1, 8193):
        want = ref.plan(sr, hop, **geo)
        if want is None:
            assert not api.chroma_check(sr, hop=hop, **geo), hop
            path = None
        else:
            got = api.chroma_plan(sr, hop=hop, **geo)
            assert got == want[:8], (hop, got, want)
            tile, pad, lds = got[:3]
            q_at, class_at = got[6:]
            assert (hop + pad) % 32 == 2 and 0 <= pad < 32 and lds <= ref.LDS_MAX and lds % 16 == 0
            assert class_at >= -(-((tile - 1) * hop + int(rows[0])) // hop) * (hop + pad) and q_at == class_at + ref.PART_FLOATS
            assert (q_at + n16 * 17) * 4 == lds and 96 * 17 <= ref.PART_FLOATS
            assert got[5] == int((rows >= 512).sum())
            smaller += tile < cref.plan(sr, hop, **geo)[0]
            path = want[8]
        paths[path] = paths.get(path, 0) + 1
        if prev is not None and path != prev[1]:
            edges.append((prev[0], prev[1], hop, path))
        prev = (hop, path)
    print("case %s: %s; the plan changes at %s; a smaller tile than the constant-Q call's at %d hops" % (case, paths, edges[:12], smaller))
    expect = {"a": {"tile16-static", "tile8-static", "tile4-static"}, "b": {"tile16-dyn", "tile16-static", "tile8-static"},
              "c": {"tile16-static", "tile8-static", "tile4-static"}, "d": {"tile16-dyn", "tile16-static", "tile8-static"},
              "e": {"tile16-static", "tile8-static", "tile4-static", None}}[case]
    assert expect <= set(paths), (expect, set(paths))
    assert edges and (case != "e" or smaller > 0)


def _params(api, sr, geo, hop, quantity, F, T, channels, n_chroma, base, norm, floor):
    shape = {k: v for k, v in geo.items() if k not in ("norm", "scale")}
    tile, pad, lds, split_rows, segs, n_split, q_at, class_at = api.chroma_plan(sr, hop=hop, n_chroma=n_chroma, base_class=base, **shape)
    tab, rows, at = api.cqt_table(sr, **geo)
    f, h = api.cqt_lengths(sr, **shape)
    S = ChromaParams(n_chroma=n_chroma, r=geo.get("bins_per_octave", 12) // n_chroma, base_class=base, chroma_norm=norm, norm_floor=floor, q_at=q_at,
                     class_at=class_at)
    P = S.cqt
    P.n_in, P.rows0, P.half0, P.hop, P.row_pad, P.n_bins, P.n_tiles, P.n_split = T, int(rows[0]), int(h[0]), hop, pad, geo.get("n_bins", 84), len(rows), n_split
    P.n_frames, P.tile, P.channels, P.out_mode, P.floor, P.span_floats, P.lds_bytes = F, tile, channels, quantity, 0.0, class_at, lds
    for t in range(len(rows)):
        P.tile_rows[t], P.tile_base[t], P.tile_at[t] = int(rows[t]), int(h[0] - h[16 * t]), int(at[t])
    return S, tab, int(h[0])


def _emulate(api, lib, sr, geo, hop, quantity, y, s0, start, F, n_chroma, base, norm, floor=1e-10):
    """y [C, T] from position s0 on -> the emulated kernel's output [C, n_chroma, F]"""
    channels, T = y.shape
    S, tab, h0 = _params(api, sr, geo, hop, quantity, F, T, channels, n_chroma, base, norm, floor)
    Ts = (T + 3) // 4 * 4
    stage = np.full(channels * Ts + 16, np.float32(7e8), dtype=np.float32)        # (guards: nothing outside [0, T) may be read)
    rows = stage[8:8 + channels * Ts].reshape(channels, Ts)
    rows[:, :T] = y
    per = n_chroma * F
    out = np.full((channels, per + 8), np.float32(-3e9), dtype=np.float32)
    d = tch.MelDesc(src=rows.ctypes.data, dst=out.ctypes.data, src_chan_stride=Ts, dst_chan_stride=per + 8, lead=s0 - (start - h0))
    assert lib.emul_clip_chroma(C.byref(d), 1, tab.ctypes.data, tab.shape[0], C.byref(S)) == 0
    assert (out[:, per:] == np.float32(-3e9)).all()
    return out[:, :per].reshape(channels, n_chroma, F), S


EMUL_CASES = {
    # sr, geometry, hop, channels, start, n_frames, J - start (None: the row is all signal), n_chroma, base_class, the launch path, split tiles
    "a-split-and-unsplit-static": (22050, dict(fmin=C1, n_bins=84, bins_per_octave=12), 512, 2, 57, 20, None, 12, 0, "tile16-static", 4),
    "a-across-the-end-base-9": (22050, dict(fmin=C1, n_bins=84, bins_per_octave=12, norm=2, scale=2), 512, 1, 30000, 19, 3000, 12, 9, "tile16-static", 4),
    "b-dynamic": (16000, dict(fmin=1000.0, n_bins=24, bins_per_octave=12), 160, 2, 0, 35, None, 12, 0, "tile16-dyn", 0),
    "c-36-an-octave-r-3": (22050, dict(fmin=C3, n_bins=108, bins_per_octave=36), 512, 1, 4321, 18, None, 12, 5, "tile16-static", 7),
    "d-17-bins-behind-the-end": (16000, dict(fmin=1000.0, n_bins=17, bins_per_octave=12, norm=0, scale=0), 160, 1, 100000, 18, -7, 12, 0, "tile16-dyn", 0),
    "d-17-bins-six-classes": (16000, dict(fmin=1000.0, n_bins=17, bins_per_octave=12), 160, 1, 300, 18, 2000, 6, 4, "tile16-dyn", 0),
    "e-tile-8": (44100, dict(fmin=C1, n_bins=24, bins_per_octave=12), 896, 1, 5000, 11, None, 12, 0, "tile8-static", 2),
    "e-tile-4": (44100, dict(fmin=C1, n_bins=24, bins_per_octave=12), 1728, 1, 300, 8, 100, 12, 3, "tile4-static", 2),
    "many-classes-96": (22050, dict(fmin=220.0, n_bins=120, bins_per_octave=96), 64, 1, 1000, 17, None, 96, 95, "tile16-static", 8),
    "seven-bins-empty-classes": (16000, dict(fmin=1000.0, n_bins=7, bins_per_octave=12), 160, 1, 500, 17, None, 12, 10, "tile16-dyn", 0),
}


@functools.lru_cache(maxsize=None)
def _case_rows(case):
    """the case's random rows, the constant-Q emulator's magnitudes and powers of them (binary32) and the binary64 reference with
    its bounds -- computed once"""
    from pdmp3_amd import api
    sr, geo, hop, channels, start, F, left, n_chroma, base, path, n_split = EMUL_CASES[case]
    shape = {k: v for k, v in geo.items() if k not in ("norm", "scale")}
    rng = np.random.default_rng(sum(map(ord, case)))
    h0 = int(api.cqt_lengths(sr, **shape)[1][0])
    s0 = max(0, start - h0)
    T = (F - 1) * hop + 2 * h0 + 1
    y = ((rng.random((channels, T), dtype=np.float32) * 2 - 1) * np.float32(0.7)).astype(np.float32)
    if left is not None:
        y[:, max(0, start + left - s0):] = 0.0
    q32 = {m: tch._emulate(api, tch._emul(), sr, geo, hop, m, y, s0, start, F)[0] for m in (1, 2)}
    q64 = {m: cref.cqt(y, s0, start, F, sr, hop, m, **geo) for m in (1, 2)}
    return y, s0, q32, q64


@pytest.mark.parametrize("case", sorted(EMUL_CASES))
def test_kernel_arithmetic_on_the_host(case):
    """both quantities x four norms: chroma_norm 0 bit-equal to numpy's binary32 sequential fold of the constant-Q emulator's
    output, L1 and max bit-equal to numpy's binary32 chain and division on it, everything within the bound of the binary64
    definition, silent frames exactly +0"""
    from pdmp3_amd import api
    lib = _emul()
    sr, geo, hop, channels, start, F, left, n_chroma, base, path, n_split = EMUL_CASES[case]
    shape = {k: v for k, v in geo.items() if k not in ("norm", "scale")}
    want_plan = ref.plan(sr, hop, **shape)
    assert want_plan[8] == path and want_plan[5] == n_split
    y, s0, q32, q64 = _case_rows(case)
    b = geo.get("bins_per_octave", 12)
    cls, count = ref.class_map(geo["n_bins"], b, n_chroma, base)
    for quantity in (1, 2):
        folded = ref.fold32(q32[quantity], cls, n_chroma)
        for norm in range(4):
            floor = 1e-10 if norm != 1 else 1e3       # (L1 with a floor above most frames' sums: the max takes the floor)
            got, S = _emulate(api, lib, sr, geo, hop, quantity, y, s0, start, F, n_chroma, base, norm, floor)
            assert S.cqt.tile == want_plan[0]
            if norm == 0:
                assert np.array_equal(got.view(np.uint32), folded.view(np.uint32))
                assert (got[:, count == 0] == 0.0).all() and not np.signbit(got[:, count == 0]).any()
            elif norm in (1, 3):
                assert np.array_equal(got.view(np.uint32), ref.normalise32(folded, norm, floor).view(np.uint32))
            want, bound = ref.from_cqt(*q64[quantity], b, n_chroma, base, norm, floor)
            err = np.abs(got.astype(np.float64) - want)
            assert (err <= bound).all(), (quantity, norm, float((err - bound).max()))
            nz = bound > 0
            ratio = float((err[nz] / bound[nz]).max()) if nz.any() else 0.0
            print("%s quantity %d norm %s tile %d (%s, %d of %d tiles split): worst error / bound %.6f"
                  % (case, quantity, NORM_NAMES[norm], S.cqt.tile, path, n_split, S.cqt.n_tiles, ratio))
            assert np.abs(y).sum() == 0 or 0.0 < ratio <= 1.0
            # silence: the bound is 0 there and the value exactly +0
            assert (got[~nz] == 0.0).all() and not np.signbit(got[~nz]).any()
            if norm == 3 and left is None:
                assert (got.max(axis=1) == 1.0).all()
    if left is not None:
        # the frames whose longest filter lies behind the end are silent: all classes exactly +0, whatever the norm
        h0 = int(api.cqt_lengths(sr, **shape)[1][0])
        silent = [f for f in range(F) if start + f * hop - h0 >= start + left]
        assert silent and (got[:, :, silent] == 0.0).all()


@pytest.mark.parametrize("case", ["a-split-and-unsplit-static", "e-tile-8", "e-tile-4", "b-dynamic"])
def test_frames_are_frames_on_the_host(case):
    """frame f of a row is frame 0 of the row shifted by f H, bit for bit, on both sides of a tile's edge: a value's chains do
    not depend on the frame's place in a tile"""
    from pdmp3_amd import api
    lib = _emul()
    sr, geo, hop, _, _, _, _, n_chroma, base, path, _ = EMUL_CASES[case]
    tile = int(path.split("-")[0][4:])
    h0 = int(api.cqt_lengths(sr, **geo)[1][0])
    start = h0 + 77                                # (the whole row is signal)
    F = tile + 3
    rng = np.random.default_rng(tile)
    T = (F - 1) * hop + 2 * h0 + 1
    y = ((rng.random((1, T), dtype=np.float32) * 2 - 1) * np.float32(0.7)).astype(np.float32)
    for norm in (2, 3):
        long, _ = _emulate(api, lib, sr, geo, hop, 1, y, start - h0, start, F, n_chroma, base, norm)
        for f in (1, tile - 1, tile, tile + 1):
            short, _ = _emulate(api, lib, sr, geo, hop, 1, y[:, f * hop:f * hop + hop + 2 * h0 + 1], start - h0 + f * hop, start + f * hop, 2, n_chroma,
                                base, norm)
            assert np.array_equal(long[:, :, f].view(np.uint32), short[:, :, 0].view(np.uint32)), f
            assert np.array_equal(long[:, :, f + 1].view(np.uint32), short[:, :, 1].view(np.uint32)), f
        assert np.abs(long).sum() > 0


@pytest.mark.parametrize("spec", ["default", "r-3-base-5"])
def test_a_tone_at_a_bins_frequency_gives_its_class_the_maximum(spec):
    """a sinusoid at f_k through the product's own table and the kernel's arithmetic: the class of bin k, by the host's map, is
    the frame's maximum -- 1.0 at chroma_norm max -- whatever the octave; section 16 pins the table's cosine the same way"""
    from pdmp3_amd import api
    lib = _emul()
    sr, hop = 22050, 512
    geo, n_chroma, base, ks = {"default": (dict(fmin=C1, n_bins=84, bins_per_octave=12), 12, 0, (0, 30, 47, 83)),
                               "r-3-base-5": (dict(fmin=C3, n_bins=108, bins_per_octave=36), 12, 5, (0, 2, 52, 107))}[spec]
    f, h = api.cqt_lengths(sr, **geo)
    cls, _ = api.chroma_map(sr, n_chroma=n_chroma, base_class=base, **geo)
    h0 = int(h[0])
    t = np.arange(-h0, h0 + 1, dtype=np.float64)
    for k in ks:
        y = (0.5 * np.cos(2.0 * np.pi * f[k] * t / sr + 0.7)).astype(np.float32)[None, :]
        for quantity in (1, 2):
            got, _ = _emulate(api, lib, sr, geo, hop, quantity, y, 0, h0, 1, n_chroma, base, 3)
            assert int(np.argmax(got[0, :, 0])) == cls[k] and got[0, cls[k], 0] == 1.0, (k, quantity, got[0, :, 0])
            assert np.sort(got[0, :, 0])[-2] < 1.0       # (the neighbours' Hann filters answer with about a half)


def test_the_sanitizer_program_of_the_planning_calls(tmp_path):
    """tools/sanitize/chroma_plan.c: pdmp3_amd/host/clip_chroma.c's check, map and plan over clip_cqt.c under AddressSanitizer and
    UBSan, a stand-alone program on the CPU"""
    run_sanitizer_program(tmp_path, "chroma_plan", ("clip_chroma.c", "clip_cqt.c"))
