"""Clips as float batches, the parts that need no GPU (include/pdmp3_bulk.h): what the index says of a
stream's format, the input span of a clip against brute force over the definition, the filter table against binary64, and the
kernel's own arithmetic (pdmp3_amd/csrc/resample_core.h, compiled here with g++ into tests/host_emul/resample_emul.cpp's loop)
against the binary64 restatement of tests/clip_audio_ref.py within the error bound of a binary32 dot product -- with the LDS plan
the product itself chooses (pdmp3_amd_audio_lds_plan: clip_features.c audio_lds, held here to its restatement and to the kernel's
preconditions), to MPEG rates and to odd ones, one table a launch and two."""
import ctypes as C
import random
from fractions import Fraction

import numpy as np
import pytest

import clip_audio_ref as ref
import clip_streams
from clip_host import build_emul
from clip_streams import ISO_LSF


class AudioDesc(C.Structure):                      # include/pdmp3_hip.h pdmp3_audio_desc
    _fields_ = [("src", C.c_uint64), ("dst", C.c_uint64), ("chan_stride", C.c_uint64), ("start", C.c_int64), ("n_in", C.c_int64),
                ("n_out", C.c_int64), ("frame0", C.c_int64), ("n_frames", C.c_uint32), ("frame_tab", C.c_uint32), ("M", C.c_uint32),
                ("L", C.c_uint32), ("spf", C.c_uint32), ("table", C.c_uint32), ("taps", C.c_int32), ("d0", C.c_int32),
                ("flags", C.c_uint32), ("span_cap", C.c_uint32)]


def _emul():
    lib = build_emul("resample")
    lib.emul_clip_audio.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_longlong, C.c_int]
    lib.emul_clip_audio.restype = None
    return lib


def test_index_says_what_format_a_stream_has():
    from pdmp3_amd import api
    from pdmp3_amd.packer import packer
    for version in range(3):
        for sfreq in range(3):
            for mode in (3, 1):
                mp3 = packer.generate(n_frames=24, seed=7 + sfreq, version=version, sfreq=sfreq, mode=mode, bitrate_index=6, iso_strict=True)
                ix = api.StreamIndex(mp3, ISO_LSF)
                spf = 576 if version else 1152
                assert ix.frames > 0 and ix.one_format, (version, sfreq, mode)
                assert (ix.rate, ix.channels, ix.frame_samples) == (ref.RATES[3 * version + sfreq], 1 if mode == 3 else 2, spf)
                assert ix.samples == ix.frames * spf
                ix.close()
    for name, mp3, iso in clip_streams.mixed_streams(400):
        ix = api.StreamIndex(mp3, ISO_LSF)
        rate, ch, spf = C.c_long(-5), C.c_int(-5), C.c_int(-5)
        rc = ix.lib.pdmp3_amd_index_format(ix.h, C.byref(rate), C.byref(ch), C.byref(spf))
        if name == "mixed/mono-stereo":
            assert rc == 1 and ix.one_format and (rate.value, ch.value, spf.value) == (44100, 2, 1152) and ix.samples == ix.frames * 1152
        else:
            assert name == "mixed/mpeg1-lsf" and rc == 0 and not ix.one_format and ix.samples == -1
        ix.close()
    ix = api.StreamIndex(clip_streams.replay_stream(), ISO_LSF)
    assert ix.replay and ix.lib.pdmp3_amd_index_format(ix.h, None, None, None) == -1 and ix.samples == -1 and not ix.one_format
    assert ix.lib.pdmp3_amd_index_format(None, None, None, None) == -1 and ix.lib.pdmp3_amd_index_samples(None) == -1
    ix.close()


def _needed(rate_in, rate_out, width, rolloff, j):
    """the n with |u(n, j)| < Z -- |n L - j M| grows to both sides of j M / L, so they are one run -- found by trying every n
    around the run's two ends in exact arithmetic (rolloff as the binary64 it is): (first, last)"""
    m, l = ref.ratio(rate_in, rate_out)
    ro, s = Fraction(rolloff), max(l, m)

    def inside(n):
        return ro * abs(n * l - j * m) / s < width
    reach = Fraction(width * s) / ro
    lo, hi = int((j * m - reach) // l), int((j * m + reach) // l)
    assert inside(j * m // l) and not inside(lo - 3) and not inside(hi + 3)
    first = min(n for n in range(lo - 3, lo + 4) if inside(n))
    last = max(n for n in range(hi - 3, hi + 4) if inside(n))
    assert all(inside(n) for n in range(first, min(first + 50, last + 1))) and all(inside(n) for n in range(max(last - 50, first), last + 1))
    return first, last


def test_span_against_brute_force_over_the_definition():
    from pdmp3_amd import api
    rng = random.Random(20)
    for rate_in in ref.RATES:
        for rate_out in ref.RATES:
            for trial in range(6):
                width = rng.choice([1, 2, 6, 6, 16, 32, 64])
                rolloff = rng.choice([0.99, 1.0, 0.5, rng.uniform(0.05, 1.0)])
                start = rng.choice([0, 1, rng.randrange(10 ** 4), rng.randrange(10 ** 9)])
                n = rng.choice([1, 2, rng.randrange(1, 5000)])
                first, count = api.audio_span(rate_in, rate_out, start, n, width, rolloff)
                if rate_in == rate_out:
                    assert (first, count) == (start, n)
                    continue
                lo = min(_needed(rate_in, rate_out, width, rolloff, j)[0] for j in (start, start + 1, start + n - 1))
                hi = max(_needed(rate_in, rate_out, width, rolloff, j)[1] for j in (start, start + n - 2, start + n - 1))
                what = (rate_in, rate_out, width, rolloff, start, n, first, count, lo, hi)
                assert first <= lo <= first + 1, what
                assert first + count - 1 >= hi >= first + count - 2, what
    assert api.audio_span(44100, 16000, 5, 0) == (5, 0)                      # (the defaults: width 6, rolloff 0.99)
    assert api.audio_span(44100, 16000, 0, 100) == api.audio_span(44100, 16000, 0, 100, 6, 0.99)
    for bad in ((44100, 16000, -1, 10, 6, 0.99), (44100, 16000, 0, -1, 6, 0.99), (44100, 16000, 0, 10, 65, 0.99), (44100, 16000, 0, 10, -1, 0.99),
                (44100, 16000, 0, 10, 6, 1.5), (44100, 16000, 0, 10, 6, -0.5), (0, 16000, 0, 10, 6, 0.99), (44100, -3, 0, 10, 6, 0.99)):
        with pytest.raises(ValueError):
            api.audio_span(*bad)


def test_table_is_the_definition_in_binary64_rounded_once():
    from pdmp3_amd import api
    rng = random.Random(21)
    pairs = [(44100, 16000, 6, 0.99), (11025, 32000, 64, 0.99), (8000, 48000, 32, 0.99), (48000, 8000, 16, 1.0), (44100, 48000, 6, 0.37)]
    pairs += [(rng.choice(ref.RATES), rng.choice(ref.RATES), rng.choice([1, 3, 6, 20]), rng.uniform(0.1, 1.0)) for _ in range(12)]
    for rate_in, rate_out, width, rolloff in pairs:
        if rate_in == rate_out:
            with pytest.raises(ValueError):
                api.audio_table(rate_in, rate_out, width, rolloff)
            continue
        m, l = ref.ratio(rate_in, rate_out)
        tab, d0 = api.audio_table(rate_in, rate_out, width, rolloff)
        assert tab.shape[0] == l
        # outputs 0 .. L - 1 walk through every row: j M mod L
        js = np.arange(l, dtype=np.int64)
        n, h, inside = ref.taps(rate_in, rate_out, width, rolloff, js)
        q, r = js * m // l, js * m % l
        got = np.zeros_like(h)
        for k in range(tab.shape[1]):
            col = d0 + k - (n[:, 0] - q)                   # where input sample q + d0 + k lies in the reference's columns
            ok = (col >= 0) & (col < h.shape[1])
            assert (tab[r[~ok], k] == 0).all()
            got[np.flatnonzero(ok), col[ok]] = tab[r[ok], k]
        assert (np.abs(got - h) <= 2.0 ** -24 * np.abs(h) + 1e-18).all(), (rate_in, rate_out, width, rolloff)
        assert ((got != 0) <= inside).all()
    assert api.audio_table(44100, 16000)[0].shape == (160, 34) and api.audio_table(11025, 32000, 64)[0].shape == (1280, 130)
    with pytest.raises(ValueError):                                   # more than 2^22 coefficients
        api.audio_table(48000, 47999, 64)


def _random_stream(rng, frames, spf, stereo, mixed):
    """(interleaved int16 PCM as the whole-stream decoder lays it out, byte offsets per frame, mono flags)"""
    mono = rng.random(frames) < (0.4 if mixed else 0.0) if stereo else np.ones(frames, dtype=bool)
    if stereo and mixed:
        mono[rng.integers(frames)] = False
    size = np.where(mono, spf, 2 * spf)
    off = np.concatenate([[0], np.cumsum(size * 2)]).astype(np.int64)
    kind = rng.integers(3)
    pcm = rng.integers(-32768, 32768, size=int(off[-1] // 2)).astype(np.int16)
    if kind == 1:
        pcm = (pcm // 64).astype(np.int16)
    if kind == 2:
        pcm[rng.random(pcm.size) < 0.5] = 0
    return pcm, off, mono




CASES = [(44100, 16000, 6, 0.99), (48000, 16000, 6, 0.99), (32000, 16000, 6, 0.99), (22050, 16000, 6, 0.99), (16000, 48000, 32, 0.99),
         (8000, 48000, 32, 0.99), (8000, 16000, 6, 0.99), (44100, 48000, 32, 0.99), (11025, 32000, 64, 0.99), (48000, 8000, 64, 0.99),
         (48000, 8000, 64, 0.2), (24000, 44100, 16, 1.0), (44100, 44100, 6, 0.99), (12000, 12000, 6, 0.99)] + ref.ODD_PAIRS


def _plan_pairs():
    pairs = [(a, b, z, 0.99) for z in (6, 64) for a in ref.RATES for b in ref.RATES] + CASES
    return list(dict.fromkeys(pairs))


def test_the_products_lds_plan_is_the_restatement_and_keeps_the_kernels_preconditions():
    """pdmp3_amd_audio_lds_plan (the audio_lds the decode call runs) against clip_audio_ref.lds_plan, and what resample.hip and
    stream.hip pdmp3_hip_clip_audio rely on: span_cap a multiple of four (16-byte rows behind it), a span that holds every
    tile's input, nothing beyond 64 KB"""
    from pdmp3_amd import api
    assert set(ref.ODD_PAIRS) <= set(_plan_pairs()) and len(_plan_pairs()) >= 2 * 81
    seen = {}
    for rate_in, rate_out, width, rolloff in _plan_pairs():
        for channels in (1, 2):
            what = (rate_in, rate_out, width, rolloff, channels)
            flags, cap = api.audio_lds_plan(rate_in, rate_out, channels, width, rolloff)
            if rate_in == rate_out:
                assert (flags, cap) == (0, 0), what
                continue
            m, l = ref.ratio(rate_in, rate_out)
            taps = api.audio_table(rate_in, rate_out, width, rolloff)[0].shape[1]
            assert (flags, cap) == ref.lds_plan(m, l, taps, channels), what
            span = ((l - 1) + (ref.TILE - 1) * m) // l + taps
            table = ((l * taps + 3) & ~3) * 4
            assert cap % 4 == 0 and flags in (0, ref.LDS_X, ref.LDS_X | ref.LDS_TABLE), what
            if flags & ref.LDS_X:
                assert span <= cap and cap * channels * 4 <= ref.LDS_BYTES, what
            else:
                assert cap == 0 and ((span + 3) & ~3) * channels * 4 > ref.LDS_BYTES, what
            if flags & ref.LDS_TABLE:
                assert flags & ref.LDS_X and cap * channels * 4 + table <= ref.LDS_BYTES, what
            elif flags:
                assert cap * channels * 4 + table > ref.LDS_BYTES, what
            seen.setdefault(flags, what)
    print("LDS plans: %s" % sorted(seen.items()))
    assert set(seen) == {0, 1, 3}                    # (every form of the kernel; the table without the span is no plan)
    # the plan depends on the channel count
    assert api.audio_lds_plan(48000, 8000, 1, 64, 0.2)[0] == 3 and api.audio_lds_plan(48000, 8000, 2, 64, 0.2)[0] == 0
    assert api.audio_lds_plan(48000, 4000, 1, 64, 0.5)[0] == 1 and api.audio_lds_plan(48000, 4000, 2, 64, 0.5)[0] == 0
    assert api.audio_lds_plan(44100, 16000, 2) == api.audio_lds_plan(44100, 16000, 2, 6, 0.99)       # (the defaults)
    for bad in ((44100, 16000, 0), (44100, 16000, 3), (44100, 16000, -1), (0, 16000, 1), (44100, -3, 2), (44100, 16000, 1, 65), (44100, 16000, 1, 6, 1.5)):
        with pytest.raises(ValueError):
            api.audio_lds_plan(*bad)


def _clip(api, pcm, off, mono, spf, pair, start, t_out, channels, table_at=0, frame_tab=0):
    """one clip as the decode call describes it to the kernel, with the PRODUCT's LDS plan: (descriptor, stage, frame table,
    out [channels, t_out + 8] filled with -7, table or None) -- the stage holds frames [a, e) only, behind a guard that must
    never be read"""
    rate_in, rate_out, width, rolloff = pair
    m, l = ref.ratio(rate_in, rate_out)
    n_in = (len(off) - 1) * spf
    n_out = ref.out_length(n_in, rate_in, rate_out)
    first, count = api.audio_span(rate_in, rate_out, start, t_out, width, rolloff)
    lo, hi = max(first, 0), min(first + count, n_in)
    a, e = (lo // spf, (hi - 1) // spf + 1) if hi > lo else (0, 0)
    stage = np.full(int(off[e] - off[a]) // 2 + 16, 0x5A5A, dtype=np.int16)
    stage[8:8 + int(off[e] - off[a]) // 2] = pcm[off[a] // 2:off[e] // 2]
    ft = [((int(off[f] - off[a]) // 1152) << 1) | int(mono[f]) for f in range(a, e)]
    out = np.full((channels, t_out + 8), -7.0, dtype=np.float32)
    d = AudioDesc(src=stage.ctypes.data + 16, dst=out.ctypes.data, chan_stride=t_out + 8, start=start, n_in=n_in, n_out=n_out, frame0=a,
                  n_frames=e - a, frame_tab=frame_tab, M=m, L=l, spf=spf, table=0, taps=1, d0=0, flags=0, span_cap=0)
    t2 = None
    if m != l:
        t2, d0 = api.audio_table(rate_in, rate_out, width, rolloff)
        d.table, d.taps, d.d0 = table_at, t2.shape[1], d0
        d.flags, d.span_cap = api.audio_lds_plan(rate_in, rate_out, channels, width, rolloff)
    return d, stage, ft, out, t2


@pytest.mark.parametrize("case", range(len(CASES)))
def test_kernel_arithmetic_on_the_host_against_binary64(case):
    from pdmp3_amd import api
    lib = _emul()
    assert lib.emul_audio_desc_bytes() == C.sizeof(AudioDesc) == 96
    rate_in, rate_out, width, rolloff = CASES[case]
    rng = np.random.default_rng(100 + case)
    m, l = ref.ratio(rate_in, rate_out)
    spf = 1152 if rate_in >= 32000 else 576
    worst = 0.0
    seen = set()
    for stereo, mixed, channels in ((True, True, 2), (True, True, 1), (False, False, 1), (False, False, 2), (True, False, 2)):
        frames = int(rng.integers(6, 14))
        pcm, off, mono = _random_stream(rng, frames, spf, stereo, mixed)
        n_in = frames * spf
        n_out = ref.out_length(n_in, rate_in, rate_out)
        lr = ref.timeline(pcm, off, spf, stereo)
        x = ref.channels64(lr, 2 if stereo else 1, channels)
        t_out = int(rng.integers(1500, 3000))
        for start in (0, int(rng.integers(1, max(n_out - t_out, 2))), max(n_out - t_out // 2, 0), n_out + 5):
            d, stage, ft, out, t2 = _clip(api, pcm, off, mono, spf, CASES[case], start, t_out, channels)
            ft = np.array(ft + [0], dtype=np.uint32)
            tab = np.zeros(4, dtype=np.float32)
            if m != l:
                tab = np.concatenate([t2.ravel(), np.zeros(4, dtype=np.float32)])
                assert (d.flags, d.span_cap) == ref.lds_plan(m, l, d.taps, channels)
                seen.add(d.flags)
            lib.emul_clip_audio(C.byref(d), 1, ft.ctypes.data, tab.ctypes.data, t_out, channels)
            assert (out[:, t_out:] == -7.0).all()
            y64, bound = ref.resample64(x, rate_in, rate_out, width, rolloff, start, t_out)
            got = out[:, :t_out].astype(np.float64)
            valid = min(max(n_out - start, 0), t_out)
            assert (got[:, valid:] == 0).all()
            err = np.abs(got - y64)
            if m == l:
                assert (err == 0).all()
                continue
            assert (err <= bound).all(), (CASES[case], stereo, mixed, channels, start, float((err - bound).max()))
            worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max(initial=0.0)))
    print("%s: worst error / bound %.4f, LDS plans %s" % (CASES[case], worst, sorted(seen)))
    if m != l:
        assert worst > 0.0                       # (binary32 did round somewhere: the comparison is not between two copies of one number;
                                                 #  it holds at the very low output rates too, 0.0001 of the bound at 7 Hz)


def test_two_tables_in_one_launch_on_the_emulator():
    """two clips of different pairs in one launch: the second one's table lies at the padded offset behind a first table whose
    L * taps is no multiple of four (32 000 -> 48 000 at Z = 32: 3 x 65 = 195), its frames behind the first one's in the frame
    table"""
    from pdmp3_amd import api
    lib = _emul()
    pairs = [(32000, 48000, 32, 0.99), (22050, 16000, 6, 0.99)]
    rng = np.random.default_rng(77)
    t_out = 2500
    for channels in (1, 2):
        clips, ft_all, tabs, at = [], [], [], 0
        for pair, stereo in zip(pairs, (True, False)):
            spf = 1152 if pair[0] >= 32000 else 576
            pcm, off, mono = _random_stream(rng, 9, spf, stereo, stereo)
            start = int(rng.integers(1, 3000))
            d, stage, ft, out, t2 = _clip(api, pcm, off, mono, spf, pair, start, t_out, channels, table_at=at, frame_tab=len(ft_all))
            ft_all += ft
            pad = -t2.size % 4
            tabs += [t2.ravel(), np.full(pad, np.nan, dtype=np.float32)]          # (the padding is never a coefficient)
            at += t2.size + pad
            clips.append((d, stage, out, pair, start, ref.channels64(ref.timeline(pcm, off, spf, stereo), 2 if stereo else 1, channels)))
        assert clips[0][0].L * clips[0][0].taps == 195 and clips[1][0].table == 196 and clips[1][0].frame_tab > 0
        assert clips[0][0].flags == clips[1][0].flags == 3                        # (both tables are copied into LDS, 16 bytes a load)
        descs = (AudioDesc * 2)(clips[0][0], clips[1][0])
        ftab = np.array(ft_all + [0], dtype=np.uint32)
        tab = np.concatenate(tabs + [np.zeros(4, dtype=np.float32)])
        lib.emul_clip_audio(descs, 2, ftab.ctypes.data, tab.ctypes.data, t_out, channels)
        for d, stage, out, pair, start, x in clips:
            assert (out[:, t_out:] == -7.0).all()
            y64, bound = ref.resample64(x, pair[0], pair[1], pair[2], pair[3], start, t_out)
            err = np.abs(out[:, :t_out].astype(np.float64) - y64)
            assert (err <= bound).all(), (pair, channels, start, float((err - bound).max()))
            worst = float((err[bound > 0] / bound[bound > 0]).max(initial=0.0))
            print("%s, %d channel(s), table at %d: worst error / bound %.3f" % (pair, channels, d.table, worst))
            assert worst > 0.0


def test_refusals_of_the_planning_calls():
    from pdmp3_amd import api
    for rate_in, rate_out, n in ((44100, 16000, 1000), (48000, 47999, 1), (8000, 44101, 0), (44100, 44100, 10)):
        m, _ = ref.ratio(rate_in, rate_out)
        limit = (2 ** 63 - 1) // 2 // m - n                # (j M stays inside 63 bits)
        first, count = api.audio_span(rate_in, rate_out, limit, n)
        assert count >= n and (first + count - 1) >= 0
        with pytest.raises(ValueError):
            api.audio_span(rate_in, rate_out, limit + 1, n)
        with pytest.raises(ValueError):
            api.audio_span(rate_in, rate_out, 2 ** 63 - 1, n)
    assert api.audio_span(48000, 16000, 2 ** 40, 100)[0] > 2 ** 41       # (far behind any stream: still an answer, the call clamps it)
    with pytest.raises(ValueError):
        api.audio_table(48000, 2 ** 31 - 1)
    with pytest.raises(ValueError):
        api.audio_table(2 ** 31 - 1, 48000)
    for channels in (0, 3):
        with pytest.raises(ValueError):
            api.audio_lds_plan(44100, 16000, channels)
