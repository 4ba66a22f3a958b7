"""The constant-Q transform of clips, the part that needs no GPU: the planning calls of
pdmp3_amd/host/clip_cqt.c against the binary64 restatement tests/clip_cqt_ref.py, the normalisation pinned on a cosine, every
refusal, the plan over all hops, and k_clip_cqt's own indexing and arithmetic (pdmp3_amd/csrc/cqt_core.h, compiled here with
g++ into tests/host_emul/cqt_emul.cpp's loops) on random float32 rows against the definition, within the derived binary32
bound -- no value left out."""
import ctypes as C

import numpy as np
import pytest

import clip_cqt_ref as ref
from clip_host import MelDesc, build_emul, run_sanitizer_program

U = ref.U
C1 = ref.FMIN_C1


class CqtParams(C.Structure):                      # include/pdmp3_hip.h pdmp3_cqt_params
    _fields_ = [("n_in", C.c_int64), ("rows0", C.c_int32), ("half0", C.c_int32), ("hop", C.c_int32), ("row_pad", C.c_int32),
                ("n_bins", C.c_int32), ("n_tiles", C.c_int32), ("n_split", C.c_int32), ("n_frames", C.c_int32), ("tile", C.c_int32),
                ("channels", C.c_int32), ("out_mode", C.c_int32), ("floor", C.c_float), ("span_floats", C.c_uint32), ("lds_bytes", C.c_uint32),
                ("tile_rows", C.c_int32 * 32), ("tile_base", C.c_int32 * 32), ("tile_at", C.c_uint32 * 32)]


# the specs of the GPU cases (tests/test_gpu_clip_cqt.py): sampling frequency, the geometry, the hop
GPU_SPECS = {
    "a": (22050, dict(fmin=C1, n_bins=84, bins_per_octave=12), 512),
    "b": (48000, dict(fmin=55.0, n_bins=96, bins_per_octave=24), 256),
    "c": (16000, dict(fmin=1000.0, n_bins=17, bins_per_octave=12), 160),
    "d": (8000, dict(fmin=500.0, n_bins=3, bins_per_octave=1, filter_scale=0.875), 1),
    "e": (44100, dict(fmin=C1, n_bins=24, bins_per_octave=12), 1024),
}


def _emul():
    lib = build_emul("cqt")
    lib.emul_clip_cqt.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p]
    assert lib.emul_cqt_desc_bytes() == C.sizeof(MelDesc) and lib.emul_cqt_params_bytes() == C.sizeof(CqtParams)
    return lib


def _fmin_for(sr, b, n_bins):
    """C1 where the check's limits allow it at this (sr, B, n_bins), else the lowest frequency whose filter is short enough,
    else (the top bin at or above sr / 2) None"""
    q = 1.0 / (2.0 ** (1.0 / b) - 1.0)
    fmin = max(C1, q * sr / 32000.0)
    return fmin if fmin * 2.0 ** ((n_bins - 1) / b) < 0.5 * sr else None


@pytest.mark.parametrize("n_bins", [1, 16, 17, 84])
@pytest.mark.parametrize("b", [1, 12, 24, 36])
@pytest.mark.parametrize("sr", [22050, 44100, 48000, 16000, 8000])
def test_lengths_and_table_are_the_definition_in_binary64_rounded_once(sr, b, n_bins):
    from pdmp3_amd import api
    fmin = _fmin_for(sr, b, n_bins)
    if fmin is None:                               # (84 bins at one an octave and the like: no such spec; the check says so)
        assert not api.cqt_check(sr, fmin=C1, n_bins=n_bins, bins_per_octave=b)
        return
    geo = dict(fmin=fmin, n_bins=n_bins, bins_per_octave=b)
    assert api.cqt_check(sr, **geo)
    f, h = api.cqt_lengths(sr, **geo)
    wf, wl, wh = ref.lengths(sr, **geo)
    assert np.array_equal(h, wh) and (np.abs(f - wf) <= 4 * np.spacing(wf)).all()
    assert h[0] == h.max() and 2 * h[0] + 1 <= ref.MAX_LEN and h.min() >= 1
    worst = 0.0
    for norm in range(3):
        for scale in range(3):
            t, rows, at = api.cqt_table(sr, norm=norm, scale=scale, **geo)
            want, own, wrows, wat = ref.table(sr, norm=norm, scale=scale, **geo)
            assert np.array_equal(rows, wrows) and np.array_equal(at, wat) and t.shape == want.shape and t.dtype == np.float32
            assert (rows % 4 == 0).all() and rows[0] == (2 * h[0] + 1 + 3) // 4 * 4 and at[0] == 0
            # one rounding to binary32 of a binary64 value; the two binary64 evaluations differ by a few 2^-53 of the angle in
            # turns (at most Q / 2 < 2^6 turns) times the filter's peak: 2^-36 of the peak is far above that, and 1 / 4096 of
            # a rounding there
            peak = np.abs(want).max(axis=0, keepdims=True)
            err = np.abs(t.astype(np.float64) - want)
            assert (err <= U * np.abs(want) + 2.0 ** -36 * peak).all(), (norm, scale, float((err / np.maximum(peak, 1e-300)).max()))
            # exact zeros outside each bin's own support, in the padding rows and in the padding bins
            assert (t[~own] == 0.0).all() and (~own).sum() > 0 and np.isfinite(t).all()
            assert (np.abs(t).sum(axis=0)[np.r_[:min(n_bins, 16), 16:16 + min(n_bins, 16)]] > 0).all()
            worst = max(worst, float((err[own] / (U * np.maximum(np.abs(want[own]), 2.0 ** -20 * peak.max()))).max()))
    print("sr %d B %d bins %d fmin %.3f: N_0 %d, rows %s, worst |table - binary64| / (u |value|) = %.3f" % (sr, b, n_bins, fmin, 2 * h[0] + 1, list(rows), worst))


def test_the_default_spec_is_the_sketch():
    """22 050 Hz, C1, 84 bins, 12 an octave: the rows of the six tiles, the table's size and the LDS of the plans"""
    from pdmp3_amd import api
    t, rows, at = api.cqt_table(22050)
    assert list(rows) == [11340, 4500, 1788, 712, 284, 112] and t.shape == (18736, 32) and list(at) == [0, 11340, 15840, 17628, 18340, 18624]
    f, h = api.cqt_lengths(22050)
    assert 2 * h[0] + 1 == 11339 and abs(f[0] - C1) < 1e-12 and abs(f[83] / f[0] - 2.0 ** (83 / 12)) < 1e-12
    assert api.cqt_plan(22050, hop=512) == (16, 2, 95536, 512, 8, 4)
    assert api.cqt_plan(44100, hop=512)[:3] == (16, 2, 140768) and 2 * api.cqt_lengths(44100)[1][0] + 1 == 22677
    assert api.cqt_plan(16000, hop=160)[:3] == (16, 2, 60832)
    assert api.cqt_plan(48000, hop=256, fmin=55.0, n_bins=96, bins_per_octave=24)[:3] == (16, 2, 153632)


@pytest.mark.parametrize("k", [0, 42, 83])
def test_a_unit_cosine_at_a_bins_frequency_has_magnitude_one_half(k):
    """norm 1, scale 0: |C| = a / 2 for a sinusoid of amplitude a at f_k, whatever its phase -- from the product's table and
    lengths alone, not the restatement's loops"""
    from pdmp3_amd import api
    sr = 22050
    t, rows, at = api.cqt_table(sr, norm=1, scale=0)
    f, h = api.cqt_lengths(sr)
    tile = k // 16
    m = np.arange(rows[tile], dtype=np.float64) - h[16 * tile]                  # row r stands for m = r - h_(16 t)
    for phase in (0.0, 0.7, 2.9):
        y = np.cos(2.0 * np.pi * f[k] * m / sr + phase)
        blk = t[at[tile]:at[tile] + rows[tile]].astype(np.float64)
        c = complex(blk[:, k % 16] @ y, blk[:, 16 + k % 16] @ y)
        assert abs(abs(c) - 0.5) <= 1e-4, (k, phase, abs(c))
        # the phase is referred to the frame's centre: e^(i phase) / 2
        assert abs(c - 0.5 * complex(np.cos(phase), np.sin(phase))) <= 2e-4


def _raw(lib, name, spec, sr, *args):
    return getattr(lib, name)(C.byref(spec) if spec is not None else None, int(sr), *args)


def test_refusals_of_the_planning_calls():
    from pdmp3_amd import api
    lib = api.load_library()
    sr = 22050
    assert api.cqt_check(sr)
    # each limit on both sides
    ok = [dict(n_bins=1), dict(n_bins=512, bins_per_octave=96, fmin=220.0), dict(bins_per_octave=1, n_bins=8), dict(bins_per_octave=96, fmin=200.0),
          dict(fmin=40.0), dict(filter_scale=0.03), dict(hop=1), dict(hop=8192, fmin=200.0, n_bins=24), dict(norm=0), dict(norm=2), dict(scale=0),
          dict(scale=2), dict(mode=0), dict(mode=4), dict(mode="log", floor=1.2e-38), dict(n_frames=0), dict(mode="power", floor=0.0),
          dict(mode="complex", floor=float("nan"))]
    for good in ok:
        assert api.cqt_check(sr, **good), good
    refused = [dict(n_bins=0), dict(n_bins=513, bins_per_octave=96, fmin=220.0), dict(n_bins=-1), dict(bins_per_octave=0), dict(bins_per_octave=97, fmin=200.0),
               dict(fmin=0.0), dict(fmin=-1.0), dict(fmin=float("nan")), dict(fmin=float("inf")), dict(filter_scale=0.0), dict(filter_scale=-1.0),
               dict(filter_scale=float("nan")), dict(filter_scale=float("inf")), dict(hop=0), dict(hop=8193, fmin=200.0, n_bins=24), dict(hop=-1),
               dict(norm=-1), dict(norm=3), dict(scale=-1), dict(scale=3), dict(mode=-1), dict(mode=5), dict(mode="log", floor=0.0),
               dict(mode="log10", floor=-1e-10), dict(mode="log", floor=float("nan")), dict(mode="log10", floor=1e-46),
               dict(mode="log10", floor=float("inf")), dict(n_frames=-1)]
    for bad in refused:
        assert not api.cqt_check(sr, **bad), bad
    assert not api.cqt_check(0) and not api.cqt_check(-1)
    # the top bin against sr / 2: f_83 = fmin 2^(83 / 12) just below and at it
    edge = 0.5 * sr / 2.0 ** (83 / 12)
    assert api.cqt_check(sr, fmin=edge * (1 - 1e-9)) and not api.cqt_check(sr, fmin=edge * (1 + 1e-9))
    # N_0 against PDMP3_CQT_MAX_LEN: L_0 = Q sr / fmin just below 32 768 (N_0 = 32 767) and at it (32 769)
    q = 1.0 / (2.0 ** (1.0 / 12) - 1.0)
    assert api.cqt_check(sr, fmin=q * sr / 32767.9, n_bins=12) and not api.cqt_check(sr, fmin=q * sr / 32768.1, n_bins=12)
    assert 2 * api.cqt_lengths(sr, fmin=q * sr / 32767.9, n_bins=12)[1][0] + 1 == 32767
    # a table of more than 2^22 floats: 512 bins at 96 an octave -- 32 tiles, about nine times N_0 rows, against 2^17 rows
    long = dict(fmin=220.0, n_bins=512, bins_per_octave=96, filter_scale=1.1)
    rows = ref.tiles(sr, **long)[0]
    assert rows.sum() * 32 > 2 ** 22 and 2 * rows[0] < ref.MAX_LEN and not api.cqt_check(sr, **long)
    fits = dict(long, filter_scale=1.0)
    assert ref.tiles(sr, **fits)[0].sum() * 32 <= 2 ** 22 and api.cqt_check(sr, **fits)
    # a shortest filter below 3 taps (its Hann window is 0)
    assert not api.cqt_check(8000, fmin=500.0, n_bins=3, bins_per_octave=1, filter_scale=0.49)
    assert api.cqt_check(8000, fmin=500.0, n_bins=3, bins_per_octave=1, filter_scale=0.5)
    # a spec for which no tile fits the LDS: the span of four frames at the largest hop and the longest filter
    assert ref.plan(sr, 8192, fmin=q * sr / 32767.9, n_bins=12) is None and not api.cqt_check(sr, hop=8192, fmin=q * sr / 32767.9, n_bins=12)
    # nothing is written: refused specs, NULL pointers, a short cap
    good = api._cqt_spec(sample_rate=sr)
    bad = api._cqt_spec(sample_rate=sr, n_bins=0)
    n_t = 6
    f = np.full(84, -7.0)
    h = np.full(84, -7, dtype=np.int32)
    tab = np.full(18736 * 32, -7.0, dtype=np.float32)
    rows = np.full(n_t, -7, dtype=np.int32)
    at = np.full(n_t, -7, dtype=np.int32)
    ints = [C.c_int(-7) for _ in range(5)]
    lds = C.c_uint(7)

    def untouched():
        return ((f == -7.0).all() and (h == -7).all() and (tab == -7.0).all() and (rows == -7).all() and (at == -7).all()
                and all(i.value == -7 for i in ints) and lds.value == 7)
    plan_args = (C.byref(ints[0]), C.byref(ints[1]), C.byref(lds), C.byref(ints[2]), C.byref(ints[3]), C.byref(ints[4]))
    for spec in (bad, None):
        assert _raw(lib, "pdmp3_amd_cqt_check", spec, sr) == -1
        assert _raw(lib, "pdmp3_amd_cqt_lengths", spec, sr, f.ctypes.data, h.ctypes.data, 84) == -1
        assert _raw(lib, "pdmp3_amd_cqt_table", spec, sr, tab.ctypes.data, tab.size, rows.ctypes.data, at.ctypes.data) == -1
        assert _raw(lib, "pdmp3_amd_cqt_plan", spec, sr, *plan_args) == -1
        assert untouched()
    assert _raw(lib, "pdmp3_amd_cqt_lengths", good, sr, f.ctypes.data, h.ctypes.data, 83) == -1
    assert _raw(lib, "pdmp3_amd_cqt_table", good, sr, tab.ctypes.data, tab.size - 1, rows.ctypes.data, at.ctypes.data) == -1
    assert _raw(lib, "pdmp3_amd_cqt_lengths", good, 0, f.ctypes.data, h.ctypes.data, 84) == -1
    assert untouched()
    # NULL outputs are allowed: the counts come back
    assert _raw(lib, "pdmp3_amd_cqt_lengths", good, sr, None, None, 84) == 84
    assert _raw(lib, "pdmp3_amd_cqt_table", good, sr, None, 0, None, None) == 18736 * 32
    assert _raw(lib, "pdmp3_amd_cqt_plan", good, sr, None, None, None, None, None, None) == 0
    assert untouched()
    assert _raw(lib, "pdmp3_amd_cqt_table", good, sr, tab.ctypes.data, tab.size, rows.ctypes.data, at.ctypes.data) == tab.size
    assert (tab != -7.0).all() and list(rows) == [11340, 4500, 1788, 712, 284, 112]
    for kw in (dict(n_bins=0), dict(fmin=0.0), dict(hop=0)):
        for call in (api.cqt_lengths, api.cqt_table, api.cqt_plan):
            with pytest.raises(ValueError):
                call(sr, **kw)


@pytest.mark.parametrize("case", sorted(GPU_SPECS))
def test_the_plan_is_the_restatement_over_all_hops(case):
    """hops 1 .. 8192 at the specs of the GPU cases: the call's plan is the restated one at every hop -- so on both sides of every
    threshold between two tiles and of the 64 KB edge -- and keeps the kernel's preconditions"""
    from pdmp3_amd import api
    sr, geo, _ = GPU_SPECS[case]
    rows, _ = ref.tiles(sr, **geo)
    paths = {}
    prev = None
    edges = []
    for hop in range(1, 8193):
        want = ref.plan(sr, hop, **geo)
        if want is None:
            assert not api.cqt_check(sr, hop=hop, **geo), hop
            path = None
        else:
            got = api.cqt_plan(sr, hop=hop, **geo)
            assert got == want[:6], (hop, got, want)
            tile, pad, lds = got[:3]
            assert (hop + pad) % 32 == 2 and 0 <= pad < 32 and lds <= ref.LDS_MAX and lds % 16 == 0
            first = lds // 4 - ref.PART_FLOATS
            assert first >= -(-((tile - 1) * hop + int(rows[0])) // hop) * (hop + pad)
            assert got[5] == int((rows >= 512).sum())
            path = want[6]
        paths[path] = paths.get(path, 0) + 1
        if prev is not None and path != prev[1]:
            edges.append((prev[0], prev[1], hop, path))
        prev = (hop, path)
    print("case %s: %s; the plan changes at %s" % (case, paths, edges[:12]))
    expect = {"a": {"tile16-static", "tile8-static", "tile4-static"}, "b": {"tile16-static", "tile8-static", "tile4-static", None},
              "c": {"tile16-dyn", "tile16-static", "tile8-static"}, "d": {"tile16-dyn", "tile16-static"},
              "e": {"tile16-static", "tile8-static", "tile4-static"}}[case]
    assert expect <= set(paths), (expect, set(paths))
    assert edges


def test_the_64_kb_edge_and_the_segments():
    """a hop either side of 64 KB at case (c)'s spec, found from the restatement; the segments of a split tile cover its rows once,
    in order, none empty"""
    from pdmp3_amd import api
    sr, geo, _ = GPU_SPECS["c"]
    last_dyn = max(h for h in range(1, 8193) if ref.plan(sr, h, **geo)[2] <= ref.LDS_SOFT)
    first_static = min(h for h in range(1, 8193) if ref.plan(sr, h, **geo)[2] > ref.LDS_SOFT)
    assert api.cqt_plan(sr, hop=last_dyn, **geo)[2] <= 64 * 1024 < api.cqt_plan(sr, hop=first_static, **geo)[2]
    for rows in list(range(512, 2200, 4)) + [11340, 29784, 32768]:
        seg = ref.segments_of(rows)
        assert seg[0][0] == 0 and seg[-1][1] == rows and all(a < b and a % 4 == 0 for a, b in seg)
        assert all(seg[i][1] == seg[i + 1][0] for i in range(7))


def _params(api, sr, geo, hop, mode, F, T, channels, floor):
    tile, pad, lds, split_rows, segs, n_split = api.cqt_plan(sr, hop=hop, **geo)
    tab, rows, at = api.cqt_table(sr, **geo)
    f, h = api.cqt_lengths(sr, **{k: v for k, v in geo.items() if k not in ("norm", "scale")})
    P = CqtParams(n_in=T, rows0=int(rows[0]), half0=int(h[0]), hop=hop, row_pad=pad, n_bins=geo.get("n_bins", 84), n_tiles=len(rows), n_split=n_split,
                  n_frames=F, tile=tile, channels=channels, out_mode=mode, floor=floor, span_floats=lds // 4 - ref.PART_FLOATS, lds_bytes=lds)
    for t in range(len(rows)):
        P.tile_rows[t], P.tile_base[t], P.tile_at[t] = int(rows[t]), int(h[0] - h[16 * t]), int(at[t])
    return P, tab, int(h[0])


def _emulate(api, lib, sr, geo, hop, mode, y, s0, start, F, floor=0.0):
    """y [C, T] from position s0 on -> the emulated kernel's output [C, n_bins, F(, 2)]"""
    channels, T = y.shape
    P, tab, h0 = _params(api, sr, geo, hop, mode, F, T, channels, floor)
    Ts = (T + 3) // 4 * 4
    stage = np.full(channels * Ts + 16, np.float32(7e8), dtype=np.float32)        # (guards: nothing outside [0, T) may be read)
    rows = stage[8:8 + channels * Ts].reshape(channels, Ts)
    rows[:, :T] = y
    nb = P.n_bins
    per = nb * F * (2 if mode == 0 else 1)
    out = np.full((channels, per + 8), np.float32(-3e9), dtype=np.float32)
    d = MelDesc(src=rows.ctypes.data, dst=out.ctypes.data, src_chan_stride=Ts, dst_chan_stride=per + 8, lead=s0 - (start - h0))
    assert lib.emul_clip_cqt(C.byref(d), 1, tab.ctypes.data, tab.shape[0], C.byref(P)) == 0
    assert (out[:, per:] == np.float32(-3e9)).all()
    return out[:, :per].reshape((channels, nb, F, 2) if mode == 0 else (channels, nb, F)), P


EMUL_CASES = {
    # sr, geometry, hop, channels, start, n_frames, J - start (None: the row is all signal), the launch path
    "a-split-and-unsplit-static": (22050, dict(fmin=C1, n_bins=84, bins_per_octave=12), 512, 2, 57, 20, None, "tile16-static", 4),
    "a-across-the-end": (22050, dict(fmin=C1, n_bins=84, bins_per_octave=12, norm=2, scale=2), 512, 1, 30000, 19, 4000, "tile16-static", 4),
    "c-unsplit-dynamic": (16000, dict(fmin=1000.0, n_bins=17, bins_per_octave=12), 160, 2, 0, 35, None, "tile16-dyn", 0),
    "c-behind-the-end": (16000, dict(fmin=1000.0, n_bins=17, bins_per_octave=12, norm=0, scale=0), 160, 1, 100000, 18, -7, "tile16-dyn", 0),
    "d-three-taps-hop-1": (8000, dict(fmin=500.0, n_bins=3, bins_per_octave=1, filter_scale=0.875), 1, 1, 2, 40, 30, "tile16-dyn", 0),
    "e-tile-8": (44100, dict(fmin=C1, n_bins=24, bins_per_octave=12), 1024, 1, 5000, 11, None, "tile8-static", 2),
    "e-tile-4": (44100, dict(fmin=C1, n_bins=24, bins_per_octave=12), 2048, 1, 300, 7, 9000, "tile4-static", 2),
    "split-next-to-unsplit-hop-3": (16000, dict(fmin=244.0, n_bins=20, bins_per_octave=12, scale=0), 3, 2, 1000, 19, None, "tile16-static", 1),
    "split-next-to-unsplit-dynamic": (16000, dict(fmin=244.0, n_bins=20, bins_per_octave=12), 33, 1, 100, 18, 300, "tile16-dyn", 1),
}


@pytest.mark.parametrize("case", sorted(EMUL_CASES))
def test_kernel_arithmetic_on_the_host_against_binary64(case):
    from pdmp3_amd import api
    lib = _emul()
    sr, geo, hop, channels, start, F, left, path, n_split = EMUL_CASES[case]
    want_plan = ref.plan(sr, hop, **{k: v for k, v in geo.items() if k not in ("norm", "scale")})
    assert want_plan[6] == path and want_plan[5] == n_split
    rng = np.random.default_rng(sum(map(ord, case)))
    h0 = int(api.cqt_lengths(sr, **{k: v for k, v in geo.items() if k not in ("norm", "scale")})[1][0])
    s0 = max(0, start - h0)
    T = (F - 1) * hop + 2 * h0 + 1
    y = ((rng.random((channels, T), dtype=np.float32) * 2 - 1) * np.float32(0.7)).astype(np.float32)
    if left is not None:
        y[:, max(0, start + left - s0):] = 0.0
    nv = ref.valid(start + left if left is not None else 2 ** 62, start, hop, F)
    outs = {}
    for mode in range(5):
        floor = {3: 1e-6, 4: 1e-10}.get(mode, 0.0)
        got32, P = _emulate(api, lib, sr, geo, hop, mode, y, s0, start, F, floor)
        outs[mode] = got32
        want, bound = ref.cqt(y, s0, start, F, sr, hop, mode, floor or 1e-10, **geo)
        assert want.shape == got32.shape
        err = np.abs(got32.astype(np.float64) - want)
        assert (err <= bound).all(), (mode, float((err - bound).max()))
        nz = bound > 0
        ratio = float((err[nz] / bound[nz]).max()) if nz.any() else 0.0
        print("%s mode %d tile %d (%s, %d of %d tiles split): worst error / bound %.4f (valid %d of %d)"
              % (case, mode, P.tile, path, P.n_split, P.n_tiles, ratio, nv, F))
        if np.abs(y).sum() > 0:
            assert 0.0 < ratio <= 1.0
        if mode <= 2:
            # silence: the bound is 0 there and the value exactly 0.0
            assert (got32[~nz] == 0.0).all()
    if left is not None:
        assert (outs[2][:, -1, -1] == 0.0).all()   # (the shortest bin of the last frame lies behind the end)
    # modes 1 and 2 are mode 0's pair through the product's own arithmetic, bit for bit
    import clip_stft_ref as sref
    p = sref.power_as_the_product(outs[0][..., 0], outs[0][..., 1])
    assert np.array_equal(p.view(np.uint32), outs[2].view(np.uint32))
    assert np.array_equal(np.sqrt(p).view(np.uint32), outs[1].view(np.uint32))


@pytest.mark.parametrize("case", ["a-split-and-unsplit-static", "e-tile-8", "e-tile-4", "c-unsplit-dynamic"])
def test_frames_are_frames_on_the_host(case):
    """frame f of a row is frame 0 of the row shifted by f H, bit for bit, on both sides of a tile's edge: a value's chains do
    not depend on the frame's place in a tile"""
    from pdmp3_amd import api
    lib = _emul()
    sr, geo, hop, channels, _, _, _, path, _ = EMUL_CASES[case]
    tile = int(path.split("-")[0][4:])
    h0 = int(api.cqt_lengths(sr, **geo)[1][0])
    start = h0 + 77                                # (the whole row is signal)
    F = tile + 3
    rng = np.random.default_rng(tile)
    T = (F - 1) * hop + 2 * h0 + 1
    y = ((rng.random((1, T), dtype=np.float32) * 2 - 1) * np.float32(0.7)).astype(np.float32)
    long, _ = _emulate(api, lib, sr, geo, hop, 0, y, start - h0, start, F)
    for f in (1, tile - 1, tile, tile + 1):
        short, _ = _emulate(api, lib, sr, geo, hop, 0, y[:, f * hop:f * hop + hop + 2 * h0 + 1], start - h0 + f * hop, start + f * hop, 2)
        assert np.array_equal(long[:, :, f].view(np.uint32), short[:, :, 0].view(np.uint32)), f
        assert np.array_equal(long[:, :, f + 1].view(np.uint32), short[:, :, 1].view(np.uint32)), f
    assert np.abs(long).sum() > 0


def test_the_sanitizer_program_of_the_planning_calls(tmp_path):
    """tools/sanitize/cqt_plan.c: pdmp3_amd/host/clip_cqt.c's check, lengths, table, plan and the decoder's cache of tables under
    AddressSanitizer and UBSan, a stand-alone program on the CPU"""
    run_sanitizer_program(tmp_path, "cqt_plan", ("clip_cqt.c",))
