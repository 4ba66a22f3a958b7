"""What the clip tests on the GPU (tests/test_gpu_clip*.py) share, defined once: the sentinel and the guard, the named streams with
their indexes and whole-stream decodes, a decoder, sentinel-filled strided destinations, the binary32 signal a clip's frames read,
and `run`, the steps every feature call's test makes around the call.  tests/clip_gpu_calls.py holds what is particular to one
feature call and used by more than one test module.  No clip test module on the GPU imports another test module.

streams(), ref() and frames_ref() are cached here and nowhere else: a stream is indexed and decoded whole once a process."""
import functools

import numpy as np

import clip_audio_ref as aref
import clip_streams
from clip_streams import ISO_LSF

SENT = np.float32(-1234.5)                         # what every destination is filled with before a call
GUARD = 24                                         # floats behind every row's place that belong to the buffer


@functools.lru_cache(maxsize=None)
def streams():
    """name -> mp3: the streams of the frame-range tests (mono runs inside stereo, MPEG-1 and LSF in one stream, the 9600-frame C3
    configuration among them) plus one each at 48 and 32 kHz, a mono one and LSF ones at 22.05, 16 and 8 kHz"""
    from pdmp3_amd.packer import packer
    s = {name: mp3 for name, mp3, _ in clip_streams.gpu_streams()}
    s["48k"] = packer.generate(n_frames=300, seed=481, sfreq=1, mode=1, mode_ext=2, bitrate_index=10, block_pct=(40, 20, 20, 20))
    s["32k"] = packer.generate(n_frames=300, seed=321, sfreq=2, mode=0, bitrate_index=9, block_pct=(40, 20, 20, 20))
    s["44k-mono"] = packer.generate(n_frames=300, seed=441, sfreq=0, mode=3, bitrate_index=7)
    s["22k"] = packer.generate(n_frames=400, seed=221, version=1, sfreq=0, mode=1, mode_ext=2, bitrate_index=8, iso_strict=True)
    s["16k-mono"] = packer.generate(n_frames=400, seed=161, version=1, sfreq=2, mode=3, bitrate_index=6, iso_strict=True)
    s["8k"] = packer.generate(n_frames=400, seed=81, version=2, sfreq=2, mode=0, bitrate_index=6, iso_strict=True)
    return s


def _index_and_whole(mp3):
    from pdmp3_amd import api
    ix = api.StreamIndex(mp3, ISO_LSF)
    b = api.BulkDecoder(threads=2)
    try:
        b.set_quirks(ISO_LSF)
        whole = b.decode(mp3)
    finally:
        b.close()
    assert whole.nbytes == ix.pcm_offsets[-1]
    return ix, whole


@functools.lru_cache(maxsize=None)
def ref(name):
    """(index, the stream on its time line as int64 [Cs, N]) from the whole-stream decode"""
    ix, whole = _index_and_whole(streams()[name])
    if not ix.one_format:
        return ix, None
    return ix, aref.timeline(whole, ix.pcm_offsets, ix.frame_samples, ix.channels == 2)


@functools.lru_cache(maxsize=None)
def frames_ref(k):
    """(index, whole-stream decode as int16) of clip_streams.gpu_streams()[k], every switch but PDMP3_ISO_LSF off (one decoder
    takes a whole batch)"""
    return _index_and_whole(clip_streams.gpu_streams()[k][1])


@functools.lru_cache(maxsize=None)
def halo(k, first, count):
    """the first frame the host hook decodes a clip of frames from (pdmp3_amd_bulk_parse_range: the same index and halo rule)"""
    from pdmp3_amd import api
    b = api.BulkDecoder(threads=2, parse_only=True)
    try:
        b.set_quirks(ISO_LSF)
        f0, _, _ = b.parse_range(clip_streams.gpu_streams()[k][1], frames_ref(k)[0], first, count)
    finally:
        b.close()
    return f0


def decoder():
    from pdmp3_amd import api
    dec = api.BulkDecoder(threads=2)
    dec.set_quirks(ISO_LSF)
    return dec


# name -> maker of (mp3, index): the streams a test module makes for itself and adds here when it is imported.  A module uses only
# the names it adds itself (tests/test_gpu_clip_loud_long.py, which runs the loudness tests' helpers, adds its own two): a name
# resolves only where its module has been imported, and a name taken twice is a collision, so a new one says what it holds
STREAMS = {}


def source(name):
    """(mp3, index) of a stream of streams() or of STREAMS"""
    if name in STREAMS:
        return STREAMS[name]()
    return streams()[name], ref(name)[0]


def src(clips):
    """(name, start) -> (mp3, index, start): what the clip calls take"""
    return [source(n) + (s,) for n, s in clips]


def rate(p, name):
    """the rate a call with the arguments p works at on this stream: sample_rate 0 is the stream's own"""
    return p["sample_rate"] or source(name)[1].rate


def j_all(p, name):
    """the stream's length in samples at that rate"""
    ix = source(name)[1]
    return aref.out_length(ix.samples, ix.rate, rate(p, name))


def bits(a):
    """for bit-for-bit comparisons: binary32 as uint32, anything else as it is"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def host(big):
    if hasattr(big, "cpu"):
        import torch
        torch.cuda.synchronize()
        return big.cpu().numpy()
    return big


def filled(kind, shape):
    """a sentinel-filled binary32 array: a torch tensor on the GPU ("device") or a numpy array ("numpy")"""
    if kind == "device":
        import torch
        a = torch.full(shape, float(SENT), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        return a
    return np.full(shape, SENT, dtype=np.float32)


def destination(kind, k, c, inner, guard=GUARD, offset=0):
    """a sentinel-filled buffer of k * c rows of prod(inner) + guard floats, `offset` floats behind its start, and its dense
    [k, c] + inner view: rows and channels are strided, a trailing 2 in `inner` holds complex pairs.  -> (big, view); big is
    the buffer as [k, c, prod(inner) + guard], or with an offset the flat buffer, the offset's floats in front"""
    inner = tuple(inner)
    row = int(np.prod(inner)) + guard
    strides = (c * row, row) + tuple(int(np.prod(inner[i + 1:])) for i in range(len(inner)))
    big = filled(kind, (k * c * row + offset,))
    if kind == "device":
        view = big.as_strided((k, c) + inner, strides, offset)
    else:
        view = np.lib.stride_tricks.as_strided(big[offset:], (k, c) + inner, tuple(4 * s for s in strides))
    return (big if offset else big.reshape(k, c, row)), view


def run(dec, call, kind, clips, f, c, inner, offset=0, **kw):
    """dec.<call>(src(clips), f, out=<a destination of [k, c] + inner>, **kw) -> (host copy [k, c] + inner, valid); the guard
    behind every row and the offset's floats in front of the first are looked at"""
    k, inner = len(clips), tuple(inner)
    per = int(np.prod(inner))
    big, view = destination(kind, k, c, inner, offset=offset)
    out, valid = getattr(dec, call)(src(clips), f, out=view, **kw)
    assert out is view
    flat = host(big).reshape(-1)
    assert (flat[:offset] == SENT).all()
    rows = flat[offset:].reshape(k, c, per + GUARD)
    assert (rows[:, :, per:] == SENT).all(), "written behind a row's floats"
    return rows[:, :, :per].reshape((k, c) + inner), valid


def signal(dec, clips, f, p, front=0, back=0, centred=True):
    """the binary32 samples the clips' f frames read, `front` frames more in front and `back` behind, from the product's own
    audio call: per clip (s0, y [C, T]), y from sample s0 on.  centred: frames of n_fft (pitch: frame_length) samples centred on
    start + i hop, so s0 = max(0, start - front hop - n / 2); not centred (the Kaldi-style calls): frames of win_length samples
    from `start` on"""
    n = (p.get("n_fft") or p["frame_length"]) if centred else p["win_length"]
    lead = front * p["hop"] + (n // 2 if centred else 0)
    t = (f + front + back - 1) * p["hop"] + n
    s0 = [max(0, s - lead) for _, s in clips]
    y = np.full((len(clips), p["channels"], t), SENT, dtype=np.float32)
    dec.decode_clips_audio(src([(name, a) for (name, _), a in zip(clips, s0)]), t, rate(p, clips[0][0]), p["channels"], out=y)
    return list(zip(s0, y))
