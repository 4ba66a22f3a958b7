"""The launch forms of the clip feature kernels (k_clip_mel, k_clip_fbank, k_clip_mfcc, k_clip_stft; DESIGN.md section 10,
"launch forms"), the part that needs no GPU: the plan restated in tests/clip_*_ref.py (`form`) against the planning calls of
the product, and the assertion that the shapes the device tests run -- the cases of test_gpu_clip_*.py and the EDGES tables of
the reference modules, which tests/test_gpu_clip_forms.py runs -- reach every class of geometry a kernel treats differently:

  launch form    tile32 (mel_tile<2> in dynamic LDS), tile16-dyn (<1> in dynamic LDS), tile16-static (<1> on the 160 KB array)
  first region   sized by the tile's span, or by the mel tile [bands16][tile + 1] where that is larger (not stft)
  second region  mfcc: the powers [tile][bins16 + 2], or the cepstra [tile][ceps16 + 1] where those are larger
  hop<4          the lane walk's other branch (c += rem / hop; rem %= hop)
  rows-padded    the frame's rows rounded up to a multiple of 4: zero rows of the table behind the window
  idle-waves     fewer than four tiles of 16 bins: waves without work in the DFT stage
  bands-N        1, 15, 17 and 256 bands: one column tile with one band, a partial one either side of 16, all sixteen
  edge-64k       a dynamic request within 64 B of the 64 KB a tile of 16 frames is allowed

Removing an EDGES entry that alone reaches a class makes test_the_device_shapes_reach_every_class fail."""
import numpy as np
import pytest

import clip_fbank_ref as fref
import clip_forms_cases as cases
import clip_mel_ref as mref
import clip_mfcc_ref as cref
import clip_stft_ref as sref
import test_clip_fbank_host as tfh
import test_clip_mel_host as tmh
import test_clip_mfcc_host as tch
import test_clip_stft_host as tsh


def _fb_geometry(p):
    nw = p["win_length"]
    return nw, fref.dft_length(nw, p.get("round_to_power_of_two", True)), p["hop"], p["num_mel_bins"]


def mel_classes(p):
    return [mref.form(p["n_fft"], p["hop"], p["n_mels"])[3]]


def fbank_classes(p):
    return [fref.form(*_fb_geometry(p))[3]]


def mfcc_classes(p):
    return [cref.form(*_fb_geometry(p), p["num_ceps"])[3]]


def stft_classes(p):
    """one set a mode (a draw of the sweep has one mode; every other shape runs all five); a geometry whose modes differ in
    their launch form has "two-forms" in each"""
    if "mode" in p:
        return [sref.form(p["n_fft"], p["hop"], sref.MODES[p["mode"]])[3]]
    per = [sref.form(p["n_fft"], p["hop"], m)[3] for m in range(5)]
    launches = set(c for s in per for c in s if c.startswith("tile"))
    return [s | ({"two-forms"} if len(launches) > 1 else set()) for s in per]


# what the suite ran on the device before the EDGES tables: the cases of the four modules' comparisons with the definition
DEVICE = {
    "mel": [p for p, _, _ in cases.MEL_CASES.values()],
    "fbank": [p for p, _, _ in cases.FBANK_CASES.values()] + [dict(cases.FBANK_P16, **v) for v in cases.FBANK_VARIANTS.values()],
    "mfcc": [p for p, _, _, _ in cases.MFCC_CASES.values()],
    "stft": [p for p, _, _ in cases.STFT_CASES.values()],
}
CALLS = {"mel": (mel_classes, mref), "fbank": (fbank_classes, fref), "mfcc": (mfcc_classes, cref), "stft": (stft_classes, sref)}

_LAUNCHES = [{"tile32"}, {"tile16-dyn"}, {"tile16-static"}]
# every class, and the pairs of classes that meet in one piece of code: the mel tile over a span of either tile size, the
# hop < 4 walk in either template instance and on the static array
REQUIRED = {
    "mel": _LAUNCHES + [{"span"}, {"mel-tile"}, {"mel-tile", "tile16-dyn"}, {"mel-tile", "tile32"}, {"hop<4"}, {"hop<4", "tile32"},
                        {"hop<4", "tile16-dyn"}, {"hop<4", "tile16-static"}, {"rows-padded"}, {"idle-waves"}, {"bands-1"}, {"bands-15"},
                        {"bands-17"}, {"bands-256"}, {"edge-64k", "tile16-dyn"}],
    "fbank": _LAUNCHES + [{"span"}, {"mel-tile"}, {"mel-tile", "tile16-dyn"}, {"mel-tile", "tile32"}, {"hop<4"}, {"hop<4", "tile32"},
                          {"hop<4", "tile16-dyn"}, {"rows-padded"}, {"idle-waves"}, {"bands-1"}, {"bands-15"}, {"bands-17"}, {"bands-256"},
                          {"edge-64k", "tile16-dyn"}],
    "mfcc": _LAUNCHES + [{"span"}, {"mel-tile"}, {"mel-tile", "tile16-dyn"}, {"powers"}, {"cepstra"}, {"cepstra", "mel-tile"}, {"cepstra", "tile32"},
                         {"cepstra", "tile16-dyn"}, {"hop<4"}, {"hop<4", "tile32"}, {"hop<4", "tile16-dyn"}, {"rows-padded"}, {"idle-waves"}, {"bands-1"},
                         {"bands-15"}, {"bands-17"}, {"bands-256"}, {"edge-64k", "tile16-dyn"}],
    "stft": _LAUNCHES + [{"hop<4"}, {"rows-padded"}, {"idle-waves"}, {"edge-64k"}, {"two-forms", "tile16-dyn"}, {"two-forms", "tile32"}],
}
# what only the EDGES tables reach: the gap they close.  (A later device case may reach one of them too; then it leaves here.)
NEW = {
    "mel": [{"tile16-dyn"}, {"mel-tile"}, {"hop<4"}, {"rows-padded"}, {"idle-waves"}, {"bands-1"}, {"bands-15"}, {"bands-17"}, {"bands-256"},
            {"edge-64k", "tile16-dyn"}],
    "fbank": [{"tile16-dyn"}, {"mel-tile"}, {"hop<4"}, {"rows-padded"}, {"idle-waves"}, {"bands-1"}, {"bands-15"}, {"bands-17"}, {"bands-256"},
              {"edge-64k", "tile16-dyn"}],
    "mfcc": [{"tile16-dyn"}, {"hop<4"}, {"rows-padded"}, {"bands-1"}, {"bands-15"}, {"bands-17"}, {"bands-256"}, {"cepstra", "tile16-dyn"},
             {"edge-64k", "tile16-dyn"}],
    "stft": [{"rows-padded"}, {"edge-64k"}, {"two-forms", "tile16-dyn"}],
}


def _reached(want, sets):
    return any(want <= s for s in sets)


def _missing(call, entries):
    classes, _ = CALLS[call]
    sets = [s for p in DEVICE[call] + entries for s in classes(p)]
    return [sorted(w) for w in REQUIRED[call] if not _reached(w, sets)]


def test_form_is_the_products_plan():
    """every EDGES entry, and the grids the four host modules walk their plans' preconditions over"""
    from pdmp3_amd import api
    n = 0
    for g in list(tmh.tile_sweep()) + [(e["n_fft"], e["hop"], e["n_mels"]) for e in mref.EDGES.values()]:
        assert api.mel_tile(*g) == mref.form(*g)[:3], g
        n += 1
    for g in list(tfh.tile_sweep()) + [_fb_geometry(e) for e in fref.EDGES.values()]:
        assert api.fbank_tile(*g) == fref.form(*g)[:3], g
        n += 1
    for g in list(tch.tile_sweep()) + [_fb_geometry(e) + (e["num_ceps"],) for e in cref.EDGES.values()]:
        assert api.mfcc_tile(*g) == cref.form(*g)[:3], g
        n += 1
    for g in list(tsh.tile_sweep()) + [(e["n_fft"], e["hop"], m) for e in sref.EDGES.values() for m in range(5)]:
        assert api.stft_tile(*g) == sref.form(*g)[:3], g
        n += 1
    print("form() is the product's plan at %d geometries" % n)


def test_the_edges_are_shapes_the_product_accepts():
    from pdmp3_amd import api
    for e in mref.EDGES.values():
        assert api.mel_check(e["sample_rate"] or 44100, n_fft=e["n_fft"], hop=e["hop"], n_mels=e["n_mels"], scale=e["scale"], norm=e["norm"]), e
    for check, table, extra in ((api.fbank_check, fref.EDGES, fref.WITH_EVERYTHING), (api.mfcc_check, cref.EDGES, {})):
        for e in table.values():
            p = {k: v for k, v in e.items() if k not in ("stream", "channels")}
            assert check(**dict(p, sample_rate=e["sample_rate"] or 44100)), e
            assert check(**dict(p, sample_rate=e["sample_rate"] or 44100, **extra)), e
    for e in sref.EDGES.values():
        p = {k: v for k, v in e.items() if k not in ("stream", "channels", "modes")}
        assert api.stft_check(**dict(p, sample_rate=e["sample_rate"] or 44100)), e
    # the bytes a workgroup asks for at the shapes DESIGN.md section 10 names
    assert mref.form(1024, 256, 80)[2] == 53536 and fref.form(1024, 1024, 256, 80)[2] == 52512 and fref.form(551, 1024, 3, 256)[2] == 59968
    assert mref.form(1024, 3, 80)[2] == 82480 and mref.form(1024, 4, 80)[2] == 70784
    assert mref.form(958, 4, 80)[2] == mref.form(958, 4, 1)[2] == mref.form(958, 4, 256)[2] == 65536
    assert fref.form(900, 1024, 4, 80)[2] == fref.form(960, 960, 4, 80)[2] == cref.form(900, 1024, 4, 80, 13)[2] == 65536
    assert sref.form(944, 3, 0)[2] == 65488 and sref.form(1024, 256, 0)[2] == 54560
    for call, table in (("mel", mref), ("fbank", fref), ("mfcc", cref), ("stft", sref)):
        classes = CALLS[call][0]
        for name in table.EXACT_EDGE:
            assert any("edge-64k" in s for s in classes(table.EDGES[name])), (call, name)


@pytest.mark.parametrize("call", sorted(CALLS))
def test_the_device_shapes_reach_every_class(call):
    classes, module = CALLS[call]
    edges = list(module.EDGES.values())
    assert _missing(call, edges) == []
    # the classes the EDGES tables are there for: not reached without them
    before = [s for p in DEVICE[call] for s in classes(p)]
    for w in NEW[call]:
        assert not _reached(w, before), (call, sorted(w), "runs on the device without EDGES: take it out of NEW")
    # and every entry that alone reaches a class is missed when it is taken out
    sole = {}
    for name in module.EDGES:
        rest = [e for k, e in module.EDGES.items() if k != name]
        gone = _missing(call, rest)
        if gone:
            sole[name] = gone
    print("%s: %d of %d EDGES entries alone reach a class: %s" % (call, len(sole), len(edges), sole))
    assert sole


def test_the_mel_tile_never_sizes_the_static_kernel():
    """tile16-static with the first region sized by the mel tile is unreachable, so no case asks for it: at 16 frames the mel
    tile is at most 256 x 17 floats and the second region at most 16 x (528 + 2) -- the log-mel call's 513 bins; 514 floats
    a frame for fbank and mfcc, whose cepstra take at most 257 --, together 51 328 B, inside the 64 KB of a dynamic request"""
    assert (256 * 17 + 16 * (528 + 2)) * 4 == 51328 <= mref.LDS_SOFT and max(512 + 2, 256 + 1) <= 528 + 2
    seen = 0
    for n in range(16, 1025, 2):
        for hop in sorted(set([1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 31, 32, 33, n // 4, n // 2, n - 1, n])):
            for bands in (1, 80, 256):
                for c in (mref.form(n, hop, bands)[3], fref.form(n, n, hop, bands)[3], fref.form(n - 1, fref.dft_length(n - 1), hop if hop < n else n - 1, bands)[3],
                          cref.form(n, n, hop, bands, bands)[3]):
                    assert not {"tile16-static", "mel-tile"} <= c, (n, hop, bands)
                    seen += "mel-tile" in c
    assert seen
    for call in ("mel", "fbank", "mfcc"):
        assert {"tile16-static", "mel-tile"} not in REQUIRED[call]


def test_the_sweeps_geometries_are_drawn_inside_the_classes():
    """the seeded draws of tests/test_gpu_clip_forms.py: the same twelve every time, each in a class of REQUIRED that the speech
    shapes do not reach, and at most 2 of 12 without a band that holds a bin"""
    import clip_forms_draws as draws
    from pdmp3_amd import api
    for call in sorted(CALLS):
        got = draws.draw(call)
        assert len(got) == 12 and got == draws.draw(call)
        classes = CALLS[call][0]
        for p in got:
            assert any(s & draws.INTERESTING for s in classes(p)), (call, p)
            q = {k: v for k, v in p.items() if k not in ("stream", "channels")}
            assert getattr(api, call + "_check")(**dict(q, sample_rate=p["sample_rate"] or 44100)), (call, p)
        if call in ("mel", "stft"):
            assert len(set(p["mode"] for p in got)) >= 3
        if call != "stft":
            empty = [p for p in got if draws.no_band_holds_a_bin(call, p)]
            print("%s: %d of 12 draws have no band that holds a bin" % (call, len(empty)))
            assert len(empty) <= 2
        reached = set(frozenset(w) for w in REQUIRED[call] if any(_reached(w, classes(p)) for p in got))
        print("%s: the draws reach %d of %d classes" % (call, len(reached), len(REQUIRED[call])))
