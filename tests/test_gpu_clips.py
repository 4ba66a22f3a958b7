"""Clips on the GPU (include/pdmp3_bulk.h pdmp3_amd_bulk_decode_clips).

Every clip's PCM must be bit for bit the slice [pcm_offsets[a], pcm_offsets[b]) of BulkDecoder.decode(mp3) -- the whole
stream, same decoder settings -- and within +-1 LSB of the oracle's whole-stream output sliced the same way (the project's
bar; the oracle comparison alone is skipped for the two classes tests/fuzz_gpu.py exempts: a stream that makes the
reference's line counter wrap, and one whose synthesis is overloaded beyond 4 x full scale, within 64 LSB).  Destinations
are filled with the sentinel first: nothing past a clip's byte count, and nothing between the rows of a [K, stride]
destination, may change.

One batch of 69 clips from 18 streams -- the families of test_clip_host.py (fuzz_gpu.random_cfg configurations, MPEG-1 and
LSF; non-strict short-heavy streams for the scfsi case; low bit rates for H6; bit-flipped streams whose index the
one-thread scan builds; mono runs inside stereo; MPEG-1 and LSF frames in one stream) and one clip of 8400 frames, longer
than the decoder's 8192-frame window, from a stream of the C3 configuration (320 kbps joint stereo, 9600 frames: as long as
the oracle's restatement, 0.5 ms a frame on the host, can be run here) -- goes to pageable, pinned and device memory."""
import zlib

import numpy as np
import pytest

import clip_gpu as cg
import clip_streams
from clip_streams import ISO_LSF
from util import GUARD, SENTINEL

pytestmark = pytest.mark.gpu


_ORACLE = {}


def _oracle(oracle, k):
    """the oracle's whole-stream output of stream k and what to make of a difference (fuzz_gpu.py's exemptions)"""
    if k not in _ORACLE:
        name, mp3, _ = clip_streams.gpu_streams()[k]
        want = np.frombuffer(oracle.decode_buffer_like_cli_iso(mp3, ISO_LSF), dtype=np.int16)
        undefined = oracle.last_undefined
        peak = None
        ix, whole = cg.frames_ref(k)
        if not undefined and want.shape == whole.shape and np.abs(want.astype(np.int32) - whole.astype(np.int32)).max(initial=0) > 1:
            _, sp_t, sd_t = oracle.decode_buffer_like_cli_iso(mp3, ISO_LSF, tap_frames=ix.frames + 8)
            _, f32 = oracle.decode_f32(sp_t, sd_t)
            peak = float(np.abs(f32).max()) if f32.size else 0.0
        _ORACLE[k] = (want, undefined, peak)
    return _ORACLE[k]


def _clips():
    """(stream, first, count): four per stream -- two at random places, and at the start, at the last frame, past the end
    and empty ones spread over the streams -- and the long one"""
    out = []
    streams = clip_streams.gpu_streams()
    for k, (name, mp3, _) in enumerate(streams[:-1]):
        ix, _ = cg.frames_ref(k)
        rs = np.random.RandomState(zlib.crc32(name.encode()))
        edge = [(0, 30), (ix.frames - 1, 5), (ix.frames + 10, 5), (ix.frames // 3, 0)][k % 4]
        out += [(k, int(rs.randint(0, ix.frames)), int(rs.randint(1, 120))) for _ in range(3)] + [(k,) + edge]
    out.append((len(streams) - 1, 1000, 8400))
    return out


def _check_clip(oracle, k, first, count, got_bytes, seg, what):
    """seg: the clip's place and the guard behind it (int16 numpy)"""
    ix, whole = cg.frames_ref(k)
    a, b = ix.clamp(first, count)
    lo, hi = int(ix.pcm_offsets[a]) // 2, int(ix.pcm_offsets[b]) // 2
    assert got_bytes == 2 * (hi - lo), (what, k, first, count)
    n = hi - lo
    assert np.array_equal(seg[:n], whole[lo:hi]), "%s: stream %d clip %d+%d differs from the whole-stream decode" % (what, k, first, count)
    assert (seg[n:] == SENTINEL).all(), "%s: stream %d clip %d+%d: written past its byte count" % (what, k, first, count)
    want, undefined, peak = _oracle(oracle, k)
    if undefined or n == 0:
        return "undefined" if undefined else "empty"
    d = int(np.abs(seg[:n].astype(np.int32) - want[lo:hi].astype(np.int32)).max())
    if d > 1:
        assert peak is not None and peak > 4.0 and d <= 64, "%s: stream %d clip %d+%d: %d LSB from the oracle (peak %s)" % (what, k, first, count, d, peak)
        return "overloaded"
    return "ok"


def _sentinel_segments(kind, sizes):
    """one sentinel-filled int16 buffer with a place of size + GUARD per clip -> (owner, views, host view of the whole)"""
    from pdmp3_amd import api
    total = int(sum(sizes)) + GUARD * len(sizes)
    starts = np.concatenate([[0], np.cumsum(np.asarray(sizes) + GUARD)[:-1]]).astype(np.int64)
    if kind == "device":
        import torch
        flat = torch.full((total,), SENTINEL, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        return flat, [flat[s:s + n + GUARD] for s, n in zip(starts, sizes)], starts
    if kind == "pinned":
        pin = api.PinnedPCM(total)
        pin.array[:] = SENTINEL
        return pin, [pin.array[s:s + n + GUARD] for s, n in zip(starts, sizes)], starts
    flat = np.full(total, SENTINEL, dtype=np.int16)
    return flat, [flat[s:s + n + GUARD] for s, n in zip(starts, sizes)], starts


@pytest.mark.parametrize("kind", ["pageable", "pinned", "device"])
def test_a_batch_of_clips_is_the_whole_stream_sliced(oracle, kind):
    from pdmp3_amd import api
    streams = clip_streams.gpu_streams()
    clips = _clips()
    assert len(clips) >= 64 and len(set(k for k, _, _ in clips)) >= 16
    sizes = []
    for k, first, count in clips:
        ix, _ = cg.frames_ref(k)
        a, b = ix.clamp(first, count)
        sizes.append(int(ix.pcm_offsets[b] - ix.pcm_offsets[a]) // 2)
    assert max(b - a for (k, f, c) in clips for a, b in [cg.frames_ref(k)[0].clamp(f, c)]) > 8192
    owner, views, starts = _sentinel_segments(kind, sizes)
    dec = api.BulkDecoder(threads=2)
    try:
        dec.set_quirks(ISO_LSF)
        got = dec.decode_clips([(streams[k][1], cg.frames_ref(k)[0], first, count) for k, first, count in clips], views)
        stats = dec.clip_stats()
    finally:
        dec.close()
    if kind == "device":
        import torch
        torch.cuda.synchronize()
        host = owner.cpu().numpy()
    else:
        host = owner.array if kind == "pinned" else owner
    seen = {}
    for i, (k, first, count) in enumerate(clips):
        seg = host[starts[i]:starts[i] + sizes[i] + GUARD]
        r = _check_clip(oracle, k, first, count, int(got[i]), seg, kind)
        seen[r] = seen.get(r, 0) + 1
    kept = sum(b - a for (k, f, c) in clips for a, b in [cg.frames_ref(k)[0].clamp(f, c)])
    halo = sum(cg.frames_ref(k)[0].clamp(f, c)[0] - cg.halo(k, f, c) for k, f, c in clips if cg.frames_ref(k)[0].clamp(f, c)[1] > cg.frames_ref(k)[0].clamp(f, c)[0])
    print("%s: %d clips, %s; clip_stats %s, kept %d, halo %d" % (kind, len(clips), seen, stats, kept, halo))
    assert stats == (kept, halo)
    assert seen.get("ok", 0) >= 50
    if kind == "pinned":
        owner.free()


@pytest.mark.parametrize("kind", ["numpy", "device"])
def test_rows_of_one_array(oracle, kind):
    """out = one [K, stride] array whose rows are not 16-byte aligned (stride odd): the rows' gaps stay the sentinel"""
    from pdmp3_amd import api
    streams = clip_streams.gpu_streams()
    clips = _clips()[:-1]
    stride = 1 + GUARD + max(int(cg.frames_ref(k)[0].pcm_offsets[cg.frames_ref(k)[0].clamp(f, c)[1]] - cg.frames_ref(k)[0].pcm_offsets[cg.frames_ref(k)[0].clamp(f, c)[0]]) // 2
                             for k, f, c in clips)
    if kind == "device":
        import torch
        out = torch.full((len(clips), stride), SENTINEL, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
    else:
        out = np.full((len(clips), stride), SENTINEL, dtype=np.int16)
    dec = api.BulkDecoder(threads=2)
    try:
        dec.set_quirks(ISO_LSF)
        got = dec.decode_clips([(streams[k][1], cg.frames_ref(k)[0], first, count) for k, first, count in clips], out)
    finally:
        dec.close()
    host = out.cpu().numpy() if kind == "device" else out
    for i, (k, first, count) in enumerate(clips):
        _check_clip(oracle, k, first, count, int(got[i]), host[i], kind)


def test_short_destinations_take_what_fits():
    """dst_cap below a clip's bytes: exactly the first dst_cap bytes (an odd number of 16-byte units and a cut inside a
    frame), on the device and in host memory"""
    import torch
    from pdmp3_amd import api
    streams = clip_streams.gpu_streams()
    k = next(i for i, s in enumerate(streams) if s[0] == "mixed/mono-stereo")
    ix, whole = cg.frames_ref(k)
    dec = api.BulkDecoder(threads=2)
    try:
        dec.set_quirks(ISO_LSF)
        for n in (1001, 2304 * 3 + 7, 17):
            dev = torch.full((n,), SENTINEL, dtype=torch.int16, device="cuda")
            host = np.full(n, SENTINEL, dtype=np.int16)
            torch.cuda.synchronize()
            got = dec.decode_clips([(streams[k][1], ix, 70, 40)] * 2, [dev, host])
            lo = int(ix.pcm_offsets[70]) // 2
            assert list(got) == [int(ix.pcm_offsets[110] - ix.pcm_offsets[70])] * 2
            assert np.array_equal(dev.cpu().numpy(), whole[lo:lo + n]) and np.array_equal(host, whole[lo:lo + n])
    finally:
        dec.close()


def test_ring_replay_clips_fail_and_the_decoder_goes_on():
    from pdmp3_amd import api
    streams = clip_streams.gpu_streams()
    bad = clip_streams.replay_stream()
    bix = api.StreamIndex(bad, ISO_LSF)
    assert bix.replay
    k = 3
    ix, whole = cg.frames_ref(k)
    dec = api.BulkDecoder(threads=2)
    try:
        dec.set_quirks(ISO_LSF)
        for first in (0, 100, 4000):
            with pytest.raises(api.RingReplay):
                dec.decode_range(bad, bix, first, 50)
        out = [np.full(30 * 2304 + GUARD, SENTINEL, dtype=np.int16) for _ in range(2)]
        with pytest.raises(api.RingReplay) as e:
            dec.decode_clips([(bad, bix, 10, 20), (streams[k][1], ix, 20, 30)], out)
        assert e.value.pcm_bytes[0] == api.PDMP3_BULK_REPLAY and (out[0] == SENTINEL).all()
        n = int(ix.pcm_offsets[50] - ix.pcm_offsets[20]) // 2
        assert e.value.pcm_bytes[1] == 2 * n and (out[1][n:] == SENTINEL).all()
        assert np.array_equal(out[1][:n], whole[int(ix.pcm_offsets[20]) // 2:][:n])
        got = dec.decode_range(streams[k][1], ix, 5, 60)
        assert np.array_equal(got, whole[int(ix.pcm_offsets[5]) // 2:int(ix.pcm_offsets[65]) // 2])
    finally:
        dec.close()
        bix.close()


def test_switches_that_differ_from_the_index_are_refused():
    """an index built with PDMP3_ISO_LSF and a decoder without it: -1 (RuntimeError), nothing written; then right"""
    from pdmp3_amd import api
    streams = clip_streams.gpu_streams()
    k = next(i for i, s in enumerate(streams) if s[0] == "mixed/mpeg1-lsf")
    ix, whole = cg.frames_ref(k)
    dec = api.BulkDecoder(threads=2)
    try:
        out = np.full((1, 50000), SENTINEL, dtype=np.int16)
        with pytest.raises(RuntimeError):
            dec.decode_clips([(streams[k][1], ix, 60, 50)], out)
        assert (out == SENTINEL).all()
        dec.set_quirks(ISO_LSF)
        got = dec.decode_range(streams[k][1], ix, 60, 50)
        assert np.array_equal(got, whole[int(ix.pcm_offsets[60]) // 2:int(ix.pcm_offsets[110]) // 2])
    finally:
        dec.close()
