import functools
import hashlib

import numpy as np


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@functools.lru_cache(maxsize=None)
def ref_digests():
    """tests/golden/ref_digests.json: sha256 digests of the compiled reference's outputs on the inputs of the tests that
    compare against it (tools/make_golden.py), so that they check something where oracle/_ref is not built"""
    import json
    import os
    return json.load(open(os.path.join(os.path.dirname(__file__), "golden", "ref_digests.json")))


def cli_digest(pcm_bytes, sp, sd):
    """a CLI-style decode with tapped records, as stored in ref_digests.json: [PCM sha, record count, spectra sha, side sha]"""
    return [hashlib.sha256(pcm_bytes).hexdigest(), int(sp.shape[0]), sha(sp), sha(sd.view(np.uint8))]


def quad_list(q):
    """a Huffman quadruple result ((v, w, x, y), bits consumed, status) in JSON form"""
    return [[int(t) for t in q[0]], int(q[1]), int(q[2])]


def nch_of(side):
    return 1 if ((int(side["frame"][0, 0, 0]) >> 2) & 3) == 3 else 2


def pcm_tolerance_scaled(stage3):
    """ONLY for inputs that are not corpus cases with a literal tolerance (tests/corpus.py PCM_TOL_LSB): bit-flipped
    streams whose global_gain drives the synthesis 100x .. 4000x past full scale (test_gpu_bulk.py).  +-1 LSB, or the
    north-star float tolerance 1e-5 relative to the synthesis amplitude (an LSB is then far below the binary32
    resolution of the sums)."""
    amp = float(np.abs(stage3).max()) * 32.0       # bound of one matrixing output
    return max(1, int(np.ceil(1e-5 * 32767.0 * amp)))


def assert_pcm_close(got, want, tol=1, what=""):
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    assert d.max() <= tol, "%s PCM max-abs-diff %d LSB > %d (at %s)" % (
        what, d.max(), tol, np.unravel_index(d.argmax(), d.shape))
    return int(d.max()), int((d > 0).sum())


def oracle_decode_many(oracle, streams, threads=None):
    """the oracle's CLI-style decode of several byte streams on a thread pool (the ctypes call releases the GIL and the
    oracle's stream state is per call): int16 arrays, in order.  Test infrastructure only."""
    import os
    from concurrent.futures import ThreadPoolExecutor
    oracle.decode_buffer_like_cli(streams[0][:8192])         # the oracle's lazily built tables, once, on this thread
    if threads is None:
        threads = max(1, min(16, len(os.sched_getaffinity(0))))
    with ThreadPoolExecutor(threads) as ex:
        return [np.frombuffer(b, dtype=np.int16) for b in ex.map(oracle.decode_buffer_like_cli, streams)]


def level(pcm):
    """(median, 99th percentile, fraction clipped) of |PCM|, to print beside a parity result"""
    a = np.abs(np.asarray(pcm, dtype=np.int16).astype(np.int32)).ravel()
    if a.size == 0:
        return 0, 0, 0.0
    return int(np.median(a)), int(np.percentile(a, 99)), float((a >= 32767).mean())


# What a launch must leave alone: tests decode into buffers pre-filled with these (int16 / the bits of a float32) and look
SENTINEL = 0x5A5A
SENTINEL_F32_BITS = 0x5A5A5A5A
GUARD = 64                                        # values behind the last frame's place that belong to the buffer


def sentinel_buffer(n_frames, f32=False):
    """numpy buffer for n_frames frames of PCM plus the guard, every value the sentinel"""
    if f32:
        return np.full(n_frames * 2304 + GUARD, SENTINEL_F32_BITS, dtype=np.uint32).view(np.float32)
    return np.full(n_frames * 2304 + GUARD, SENTINEL, dtype=np.int16)


def check_launch_pcm(got_flat, want, side, what="", tol=None):
    """got_flat: what a decode of the records `side` left in a sentinel_buffer(); want: the oracle's [n][2304] (int16 or float32).
    Every sample the contract of include/pdmp3_hip.h has written (a mono frame: the first half of its place) is within
    +-1 LSB of the oracle's and at most 2 % of them differ at all (float: within tol absolute); everything else -- the second
    half of a mono frame's place, the guard -- still holds the sentinel.  -> (max difference, share of differing samples)"""
    n = want.shape[0]
    f32 = want.dtype == np.float32
    assert got_flat.size == n * 2304 + GUARD and got_flat.dtype == want.dtype
    bits = got_flat.view(np.uint32) if f32 else got_flat
    sent = SENTINEL_F32_BITS if f32 else SENTINEL
    assert (bits[n * 2304:] == sent).all(), "%s: written behind the last frame" % what
    fr = side["frame"].reshape(n, -1)[:, 0]
    written = np.ones((n, 2304), dtype=bool)
    written[((fr >> 2) & 3) == 3, 1152:] = False
    body = bits[:n * 2304].reshape(n, 2304)
    bad = np.flatnonzero((body != sent)[~written])
    assert bad.size == 0, "%s: %d values written into the unused half of mono frames' places" % (what, bad.size)
    got = got_flat[:n * 2304].reshape(n, 2304)
    if f32:
        d = np.abs(got[written].astype(np.float64) - want[written])
        assert not np.isnan(d).any() and d.max() <= tol, "%s: float PCM differs by %g > %g" % (what, d.max(), tol)
        return float(d.max()), float((d > 0).mean())
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    d[~written] = 0
    assert d.max() <= 1, "%s: PCM max-abs-diff %d LSB > 1 (at %s; a frame left at the sentinel reads %d)" % (
        what, d.max(), np.unravel_index(d.argmax(), d.shape), SENTINEL)
    share = float((d[written] > 0).mean())
    assert share <= 0.02, "%s: %.3f %% of the samples differ from the oracle's" % (what, 100 * share)
    return int(d.max()), share
