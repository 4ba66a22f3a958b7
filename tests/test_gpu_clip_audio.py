"""Clips by sample position as float batches on the GPU (include/pdmp3_bulk.h pdmp3_amd_bulk_decode_clips_audio; DESIGN.md
section 9).

Every value is checked against the definitions restated in tests/clip_audio_ref.py on the product's own whole-stream int16
output (BulkDecoder.decode): at the stream's own rate bit for bit -- de-interleaved, mono frames doubled, downmixed or doubled by
the channel rules, zeros from the stream's end on --, at another rate against the definition evaluated in binary64 within

    |y - y64| <= (T_j + 2) * 2^-24 * sum_n |h(n, j)| |x[n]|,       T_j = the number of n with |u(n, j)| < Z

the error bound of a length-T_j binary32 dot product with once-rounded coefficients (T_j - 1 additions, one product rounding,
one coefficient rounding, one more for second-order terms; x is exact).  It holds for any summation order, with or without FMA,
and is 0 on digital silence.  Destinations are filled with a sentinel first: nothing outside [k, :, :T] may change.

Streams (tests/clip_gpu.py): those of test_gpu_clips.py (mono runs inside stereo, MPEG-1 and LSF in one stream, the 9600-frame C3 configuration
among them) plus one each at 48 and 32 kHz and LSF ones at 22.05, 16 and 8 kHz."""
import numpy as np
import pytest

import clip_audio_ref as ref
import clip_gpu as cg
import clip_streams
from clip_gpu import SENT
from clip_gpu_calls import audio_check as _check, audio_run as _run
from clip_streams import ISO_LSF

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", ["device", "numpy"])
def test_own_rate_is_the_whole_stream_decode_bit_for_bit(kind):
    """C = Cs (channels = 0), rate = 0: clips at sample 0, across the stream's end, wholly behind it, at starts that are no
    multiples of the frame length; mono frames inside a stereo stream come out doubled"""
    t = 30000
    dec = cg.decoder()
    try:
        for names in (["mixed/mono-stereo", "48k", "32k", "22k", "8k", "scfsi/joint"], ["44k-mono", "16k-mono"]):
            clips = []
            for n in names:
                ix, _ = cg.ref(n)
                clips += [(n, 0), (n, ix.samples - t // 3), (n, ix.samples + 17), (n, 1152 * 5 + 331), (n, ix.samples // 2 + 1)]
            got, valid = _run(dec, kind, clips, t, c_out=cg.ref(names[0])[0].channels)
            for i, (n, s) in enumerate(clips):
                _check(n, s, got[i], int(valid[i]), t, 0, cg.ref(n)[0].channels)
        ix, lr = cg.ref("mixed/mono-stereo")
        mono_frames = np.flatnonzero(np.diff(ix.pcm_offsets) == 2304)
        assert mono_frames.size and (lr[0] != lr[1]).any()        # (the stream does mix mono frames into stereo)
    finally:
        dec.close()


def test_a_clip_longer_than_a_window():
    """8400 frames of the C3-configuration stream from a start inside a frame: a call of its own, device memory"""
    dec = cg.decoder()
    try:
        t = 8400 * 1152
        start = 1000 * 1152 + 37
        got, valid = _run(dec, "device", [("c3-config", start)], t, c_out=2)
        _check("c3-config", start, got[0], int(valid[0]), t, 0, 2)
        assert valid[0] == t
    finally:
        dec.close()


@pytest.mark.parametrize("kind", ["device", "numpy"])
def test_downmix_and_doubling_at_the_own_rate_are_exact(kind):
    t = 20000
    dec = cg.decoder()
    try:
        clips = [("mixed/mono-stereo", 1152 * 60 + 5), ("48k", 7), ("22k", 576 * 398), ("44k-mono", 100), ("16k-mono", 0), ("8k", 576 * 400 - 1)]
        for channels in (1, 2):
            got, valid = _run(dec, kind, clips, t, 0, channels)
            for i, (n, s) in enumerate(clips):
                _check(n, s, got[i], int(valid[i]), t, 0, channels)
        ix, lr = cg.ref("mixed/mono-stereo")
        a = 1152 * 60 + 5
        assert (lr[0, a:a + t] != lr[1, a:a + t]).any() and ((lr[0, a:a + t] + lr[1, a:a + t]) % 2 != 0).any()
    finally:
        dec.close()


RESAMPLE_SOURCES = ["mixed/mono-stereo", "48k", "32k", "22k", "16k-mono", "8k", "44k-mono", "h6/stereo"]


@pytest.mark.parametrize("rate,width,kind", [(16000, 0, "device"), (16000, 0, "numpy"), (48000, 32, "device")])
def test_resampling_a_batch_of_mixed_rates_against_binary64(rate, width, kind):
    """one batch of 44.1 / 48 / 32 kHz MPEG-1 and 22.05 / 16 / 8 kHz LSF sources to one rate, stereo and downmixed"""
    t = 24000 if rate == 16000 else 40000
    dec = cg.decoder()
    try:
        rates = set(cg.ref(n)[0].rate for n in RESAMPLE_SOURCES)
        assert rates >= {44100, 48000, 32000, 22050, 16000, 8000}
        clips = []
        for n in RESAMPLE_SOURCES:
            ix, _ = cg.ref(n)
            j_all = ref.out_length(ix.samples, ix.rate, rate)
            clips += [(n, 0), (n, j_all // 3 + 11), (n, max(j_all - t // 2, 0)), (n, j_all + 3)]
        for channels in (2, 1):
            got, valid = _run(dec, kind, clips, t, rate, channels, width)
            worst = 0.0
            for i, (n, s) in enumerate(clips):
                worst = max(worst, _check(n, s, got[i], int(valid[i]), t, rate, channels, width or 6))
            print("-> %d Hz, Z = %d, %d channel(s), %s: worst error / bound %.3f over %d clips" % (rate, width or 6, channels, kind, worst, len(clips)))
            assert 0.0 < worst <= 1.0
    finally:
        dec.close()


def test_refusals():
    import torch
    from pdmp3_amd import api
    t = 5000
    bad = clip_streams.replay_stream()
    bix = api.StreamIndex(bad, ISO_LSF)
    assert bix.replay
    mix, _ = cg.ref("mixed/mpeg1-lsf")
    assert not mix.one_format
    good, _ = cg.ref("48k")
    s = cg.streams()
    dec = cg.decoder()
    try:
        for kind in ("device", "numpy"):
            # a mixed-format clip inside a batch; with a replay clip as well the replay wins
            for clips, exc, codes in (([("48k", good, 100), ("mixed/mpeg1-lsf", mix, 0), ("48k", good, 3000)], api.MixedFormat, [None, -3, None]),
                                      ([("mixed/mpeg1-lsf", mix, 50), ("48k", good, 100), (None, bix, 10)], api.RingReplay, [-3, None, -2])):
                big, view = cg.destination(kind, 3, 2, (t,))
                with pytest.raises(exc) as e:
                    dec.decode_clips_audio([(bad if n is None else s[n], ix, st) for n, ix, st in clips], t, 16000, 2, out=view)
                host = cg.host(big)
                for i, (n, ix, st) in enumerate(clips):
                    if codes[i] is None:
                        _check(n, st, host[i, :, :t], int(e.value.valid[i]), t, 16000, 2)
                        assert (host[i, :, t:] == SENT).all()
                    else:
                        assert e.value.valid[i] == codes[i] and (host[i] == SENT).all()
        # bad arguments: nothing is written
        big, view = cg.destination("device", 1, 2, (t,))
        with pytest.raises(RuntimeError):
            dec.decode_clips_audio([(s["48k"], good, -1)], t, 16000, 2, out=view)
        with pytest.raises(RuntimeError):
            dec.decode_clips_audio([(s["48k"], good, 0)], t, 16000, 2, width=65, out=view)
        with pytest.raises(RuntimeError):
            dec.decode_clips_audio([(s["48k"], good, 0)], t, 16000, 2, rolloff=1.5, out=view)
        with pytest.raises(ValueError):
            dec.decode_clips_audio([(s["48k"], good, 0), (s["44k-mono"], cg.ref("44k-mono")[0], 0)], t, 16000, 0)
        assert (cg.host(big) == SENT).all()
    finally:
        dec.close()
        bix.close()
    # a decoder without PDMP3_ISO_LSF on an LSF index, and a host-Huffman decoder
    lsf, _ = cg.ref("22k")
    plain = api.BulkDecoder(threads=2)
    try:
        big, view = cg.destination("device", 1, 2, (t,))
        with pytest.raises(RuntimeError):
            plain.decode_clips_audio([(s["22k"], lsf, 0)], t, 16000, 2, out=view)
        assert (cg.host(big) == SENT).all()
    finally:
        plain.close()
    hh = api.BulkDecoder(threads=2, host_huffman=True)
    try:
        hh.set_quirks(ISO_LSF)
        big, view = cg.destination("device", 1, 2, (t,))
        with pytest.raises(RuntimeError):
            hh.decode_clips_audio([(s["48k"], good, 0)], t, 16000, 2, out=view)
        assert (cg.host(big) == SENT).all()
    finally:
        hh.close()
    torch.cuda.synchronize()


def test_clip_stats_count_audio_clips_and_plain_clips_still_work():
    from pdmp3_amd import api
    t, rate = 12000, 16000
    clips = [("mixed/mono-stereo", 40000), ("scfsi/joint", 0), ("22k", 90000), ("48k", 99000)]
    kept = halo = 0
    par = api.BulkDecoder(threads=2, parse_only=True)
    par.set_quirks(ISO_LSF)
    try:
        for n, st in clips:
            ix, _ = cg.ref(n)
            first, count = api.audio_span(ix.rate, rate, st, t)
            lo, hi = max(first, 0), min(first + count, ix.samples)
            a, e = lo // ix.frame_samples, (hi - 1) // ix.frame_samples + 1
            assert e > a
            f0, _, _ = par.parse_range(cg.streams()[n], ix, a, e - a)
            kept += e - a
            halo += a - f0
    finally:
        par.close()
    dec = cg.decoder()
    try:
        assert dec.clip_stats() == (0, 0)
        got, valid = _run(dec, "device", clips, t, rate, 1)
        for i, (n, st) in enumerate(clips):
            _check(n, st, got[i], int(valid[i]), t, rate, 1)
        assert dec.clip_stats() == (kept, halo)
        # the stage and the tables do not disturb the slots: plain clips on the same decoder, then audio again
        k = next(i for i, x in enumerate(clip_streams.gpu_streams()) if x[0] == "mixed/mono-stereo")
        ix, whole = cg.frames_ref(k)
        plain = dec.decode_range(clip_streams.gpu_streams()[k][1], ix, 33, 50)
        assert np.array_equal(plain, whole[int(ix.pcm_offsets[33]) // 2:int(ix.pcm_offsets[83]) // 2])
        got, valid = _run(dec, "numpy", clips, t, rate, 2)
        for i, (n, st) in enumerate(clips):
            _check(n, st, got[i], int(valid[i]), t, rate, 2)
        assert dec.clip_stats() == (2 * kept + 50, 2 * halo + 33 - cg.halo(k, 33, 50))
    finally:
        dec.close()


def test_made_output_and_empty_calls():
    """out=None: a tensor on the decoder's device; n_samples 0 and no clips are fine"""
    dec = cg.decoder()
    try:
        out, valid = dec.decode_clips_audio([(cg.streams()["32k"], cg.ref("32k")[0], 1000)], 8000, 16000, 1)
        assert tuple(out.shape) == (1, 1, 8000) and out.is_cuda
        _check("32k", 1000, cg.host(out)[0], int(valid[0]), 8000, 16000, 1)
        out, valid = dec.decode_clips_audio([], 100, 16000, 1)
        assert tuple(out.shape) == (0, 1, 100) and valid.size == 0
        out, valid = dec.decode_clips_audio([(cg.streams()["32k"], cg.ref("32k")[0], 1000)], 0, 16000, 1)
        assert tuple(out.shape) == (1, 1, 0) and valid[0] == 0
    finally:
        dec.close()
