"""Frame ranges of a stream on the host (include/pdmp3_bulk.h: pdmp3_amd_index_*, pdmp3_amd_bulk_parse_range; DESIGN.md
section 8).  No GPU.

A range's records are what the host stage gives for [first, b) by itself -- scanned from the index's nearest snapshot,
`first` started like a stream's first frame -- and must be byte for byte the whole stream's records for [s, b): spectra and
gc records with the merged scalefactors and count1, where s <= a is where the synthesis halo alone would start
(pdmp3_amd.sharding.halo_start, the Python twin of the node layer's rule): the PCM of [a, b) depends on the records of
[s, a) too.  With the scalefactor / count1 look-back of the halo rule turned off
(the synthesis halo alone) some ranges of the set must come out different: the set reaches the rule."""
import functools
import zlib

import numpy as np
import pytest

import clip_streams
from clip_streams import ISO_LSF
from pdmp3_amd.sharding import frame_flags_of, halo_start

SPACINGS = (16, 64)                               # snapshot spacings: no result may depend on them


def _streams():
    s = clip_streams.random_streams(range(1, 9), (200, 420))
    s += clip_streams.scfsi_streams(400) + clip_streams.h6_streams(400)
    s += clip_streams.corrupted_streams(range(3), 360) + clip_streams.mixed_streams(400)
    return s


STREAMS = _streams()


def _ranges(frames, seed):
    rs = np.random.RandomState(seed)
    out = [(int(rs.randint(0, frames)), int(rs.randint(1, 80))) for _ in range(20)]
    return out + [(0, 12), (frames - 1, 5), (frames + 3, 4), (frames // 2, 0)]


def _same(sp1, sd1, sp2, sd2):
    return sp1.shape == sp2.shape and np.array_equal(sp1, sp2) and np.array_equal(sd1.view(np.uint8), sd2.view(np.uint8))


def test_the_stream_families_reach_both_cases():
    """the streams do what they are there for: MPEG-1 and LSF among the random ones; a granule 1 that copies scalefactors
    (scfsi) behind a short granule 0 of its channel; granules coded empty (part2_3_length 0, H6) beside coded ones"""
    from pdmp3_amd import api
    kinds = set()
    for name, mp3, iso in STREAMS:
        if name.startswith("cfg"):
            kinds.add("lsf" if "lsf" in name else "mpeg1")
    assert kinds == {"lsf", "mpeg1"}
    for name, mp3, iso in clip_streams.scfsi_streams(400):
        bits, _, _ = api.parse_bits(mp3)
        gc = bits["gc"]
        hit = False
        for ch in (0, 1):
            short0 = (gc["flags"][:, ch] & 0x04).astype(bool) & (((gc["flags"][:, ch] >> 3) & 3) == 2)
            long1 = ~((gc["flags"][:, 2 + ch] & 0x04).astype(bool) & (((gc["flags"][:, 2 + ch] >> 3) & 3) == 2))
            hit |= bool((short0 & long1 & (bits["scfsi"][:, ch] != 0)).any())
        assert hit, name
    for name, mp3, iso in clip_streams.h6_streams(400):
        bits, _, _ = api.parse_bits(mp3)
        p23 = bits["gc"]["part2_3_length"]
        assert (p23 == 0).any() and (p23 != 0).any(), name


@functools.lru_cache(maxsize=None)
def _check(k):
    """every assertion on stream STREAMS[k]; -> how many of its ranges differ without the look-back"""
    from pdmp3_amd import api
    name, mp3, iso = STREAMS[k]
    total, frames = api.scan_buffer(mp3, iso)
    b = api.BulkDecoder(threads=2, window_frames=32, parse_only=True)
    ixs = []
    try:
        b.set_quirks(iso)
        sp, sd, nbytes = b.parse(mp3)
        assert sp.shape[0] == frames and nbytes == total
        fr = sd["frame"][:, 0, 0]
        flags = frame_flags_of(sd)
        per = np.where(((fr >> 2) & 3) == 3, 1, 2) * np.where(sd["lsf"][:, 0, 0] & 3, 1152, 2304)
        for spacing in SPACINGS:
            ix = api.StreamIndex(mp3, iso, spacing=spacing)
            ixs.append(ix)
            assert ix.frames == frames and ix.pcm_offsets[-1] == total, (ix.frames, frames)
            assert ix.pcm_offsets[0] == 0 and np.array_equal(np.diff(ix.pcm_offsets), per)
            if name.startswith("flipped") or iso & ISO_LSF:
                assert not ix.split, "%s: the one-thread scan builds this index (resync / LSF)" % name
            elif frames > spacing:
                assert ix.split, "%s: the pre-pass takes a clean MPEG-1 stream" % name
        differ = 0
        for a, c in _ranges(frames, zlib.crc32(name.encode())):
            e = min(a + c, frames) if a < frames else frames
            got = [b.parse_range(mp3, ix, a, c) for ix in ixs]
            for f0, rsp, rsd in got:
                assert f0 == got[0][0] and rsp.shape[0] == got[0][1].shape[0], (name, a, c)
                if a >= frames or c == 0:
                    assert rsp.shape[0] == 0 and f0 == min(a, frames)
                    continue
                # the records of the synthesis halo [s, a) -- what the PCM of [a, b) depends on besides its own -- included
                # (the decode's first frame carries PDMP3_FR_RESET, which the whole stream's frame f0 need not)
                s = halo_start(a, flags)
                assert 0 <= f0 <= s <= a and rsp.shape[0] == e - f0
                assert (rsd["frame"][0] & 0x40).all() and np.array_equal(rsd["frame"][0] & 0xbf, sd["frame"][f0] & 0xbf)
                rsd = rsd.copy()
                rsd["frame"][0] = sd["frame"][f0]
                assert _same(rsp[s - f0:], rsd[s - f0:], sp[s:e], sd[s:e]), "%s: range %d..%d (halo from %d) from %d" % (name, a, e, s, f0)
            if a < frames and c:
                g0, qsp, qsd = b.parse_range(mp3, ixs[0], a, c, lookback=False)
                differ += not _same(qsp[a - g0:], qsd[a - g0:], sp[a:e], sd[a:e])
        print("%s: %d frames, split %s, %d of the ranges differ without the look-back" % (name, frames, ixs[0].split, differ))
        return differ
    finally:
        for ix in ixs:
            ix.close()
        b.close()


@pytest.mark.parametrize("k", range(len(STREAMS)), ids=[s[0] for s in STREAMS])
def test_index_and_range_records(k):
    """the index is the scan's (frames, total, per-frame PCM sizes of the full parse); every range's records, with two
    snapshot spacings, are the full parse's for those frames, byte for byte"""
    _check(k)


def test_the_look_back_matters():
    """with the synthesis halo alone, ranges of the set decode to other records -- among them ranges of the streams made
    for the scfsi and H6 cases"""
    differ = {STREAMS[k][0]: _check(k) for k in range(len(STREAMS))}
    print(differ)
    assert sum(differ.values()) >= 1
    assert sum(v for n, v in differ.items() if n.startswith(("scfsi", "h6"))) >= 1


def test_ring_replay_index():
    from pdmp3_amd import api
    mp3 = clip_streams.replay_stream()
    ix = api.StreamIndex(mp3)
    b = api.BulkDecoder(threads=2, window_frames=32, parse_only=True)
    try:
        assert ix.frames == api.PDMP3_BULK_REPLAY and ix.replay and ix.pcm_offsets is None
        with pytest.raises(api.RingReplay):
            b.parse_range(mp3, ix, 10, 20)
    finally:
        ix.close()
        b.close()


def test_a_decoder_with_other_switches_is_refused():
    """the index of an LSF-enabled scan and a decoder without PDMP3_ISO_LSF (and the other way round): -1"""
    from pdmp3_amd import api
    name, mp3, iso = next(s for s in STREAMS if s[2] & ISO_LSF)
    ix = api.StreamIndex(mp3, iso)
    b = api.BulkDecoder(threads=2, window_frames=32, parse_only=True)
    try:
        with pytest.raises(RuntimeError):
            b.parse_range(mp3, ix, 3, 5)
        b.set_quirks(iso)
        f0, sp, sd = b.parse_range(mp3, ix, 3, 5)
        assert sp.shape[0] == 8 - f0
    finally:
        ix.close()
        b.close()
