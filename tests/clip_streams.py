"""The streams of the frame-range / clip tests (test_clip_host.py on the host, test_gpu_clips.py on the GPU): packer
configurations of fuzz_gpu.random_cfg with fixed seeds (MPEG-1 and LSF), streams made to reach the two cases of the halo
rule that look far back (granule 1 copying scalefactors that granule 0, a short block, did not
write -- non-strict streams, whose scfsi the packer draws at random; granules coded empty at low bit rates, H6), MPEG-1
streams with bit flips whose index the one-thread scan builds, and a stream the scan calls a ring replay."""
import functools
import random

from fuzz_gpu import random_cfg
from pdmp3_amd.packer import packer

ISO_LSF = 0x40
_BITRATE = [0, 32, 40, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320]
_RATE = [44100, 48000, 32000]


def frame_offsets(mp3):
    """where the frames of a clean MPEG-1 Layer III stream start (header fields alone)"""
    offs, x = [], 0
    while x + 4 <= len(mp3) and mp3[x] == 0xFF and (mp3[x + 1] & 0xE0) == 0xE0:
        offs.append(x)
        x += 144000 * _BITRATE[mp3[x + 2] >> 4] // _RATE[(mp3[x + 2] >> 2) & 3] + ((mp3[x + 2] >> 1) & 1)
    return offs


def flipped(mp3, seed):
    """1 .. 6 bit flips: one in the sync word of a frame header in the stream's middle (the scan resyncs there, which the
    split scan's pre-pass does not take), the others anywhere"""
    rng = random.Random(seed)
    b = bytearray(mp3)
    offs = frame_offsets(mp3)
    x = offs[len(offs) // 2 + rng.randrange(len(offs) // 4)]
    b[x + 1] ^= 1 << (5 + rng.randrange(3))
    for _ in range(rng.randrange(6)):
        b[rng.randrange(len(b))] ^= 1 << rng.randrange(8)
    return bytes(b)


def random_streams(seeds, frames):
    """(name, mp3, iso) from random_cfg(Random(seed)), each stream `frames[0] .. frames[1]` frames long"""
    out = []
    for s in seeds:
        rng = random.Random(s)
        kw = random_cfg(rng)
        kw["n_frames"] = rng.randint(*frames)
        iso = ISO_LSF if kw["version"] else rng.choice([0, 0, 0x3f])
        out.append(("cfg%d/%s" % (s, ("lsf%d" % kw["version"]) if kw["version"] else "mpeg1-mode%d" % kw["mode"]), packer.generate(**kw), iso))
    return out


def scfsi_streams(frames):
    """short-heavy, non-strict: granule 1 copies (scfsi) from a granule 0 that was a short block"""
    return [("scfsi/joint", packer.generate(n_frames=frames, seed=71, mode=1, mode_ext=2, bitrate_index=11, block_pct=(10, 10, 70, 10),
                                            mixed_pct=50, iso_strict=False), 0),
            ("scfsi/stereo", packer.generate(n_frames=frames, seed=72, mode=0, bitrate_index=9, vbr=True, vbr_lo=6, vbr_hi=12,
                                             block_pct=(10, 10, 70, 10), mixed_pct=0, iso_strict=False), 0)]


def h6_streams(frames):
    """32 .. 64 kbps VBR stereo: some granules' budgets drop under the packer's 160 bits and they are coded empty (count1 stays)"""
    return [("h6/stereo", packer.generate(n_frames=frames, seed=81, sfreq=1, mode=0, vbr=True, vbr_lo=1, vbr_hi=5,
                                          block_pct=(40, 20, 20, 20)), 0),
            ("h6/joint", packer.generate(n_frames=frames, seed=82, sfreq=0, mode=1, mode_ext=2, vbr=True, vbr_lo=1, vbr_hi=4,
                                         block_pct=(10, 10, 70, 10), iso_strict=False), 0)]


def corrupted_streams(seeds, frames):
    out = []
    for s in seeds:
        rng = random.Random(1000 + s)
        mp3 = packer.generate(n_frames=frames, seed=90 + s, sfreq=rng.randint(0, 1), mode=rng.choice([0, 1, 3]), mode_ext=2,
                              bitrate_index=rng.randint(6, 12), block_pct=(40, 10, 40, 10), mixed_pct=30)
        out.append(("flipped%d" % s, flipped(mp3, s), 0))
    return out


def replay_stream():
    """32 kHz / 256 kbps frames: the reference replays its input ring (test_bulk_host.test_ring_replay_is_reported_not_looped)"""
    return packer.generate(n_frames=4147, seed=435, sfreq=2, mode=0, mode_ext=0, vbr=True, vbr_lo=4, vbr_hi=13, bitrate_index=12,
                           block_pct=(40, 20, 20, 20), mixed_pct=50)


def mixed_streams(frames):
    """streams joined end to end (each part's first frame has main_data_begin 0): channel counts that change mid-stream --
    mono runs in stereo -- and, with PDMP3_ISO_LSF, MPEG-1 and LSF frames in one stream"""
    k = max(frames // 5, 8)
    parts = [packer.generate(n_frames=k, seed=61, mode=0, bitrate_index=10), packer.generate(n_frames=k, seed=62, mode=3, bitrate_index=8),
             packer.generate(n_frames=k, seed=63, mode=1, mode_ext=2, bitrate_index=11, block_pct=(20, 10, 60, 10), iso_strict=False),
             packer.generate(n_frames=3, seed=64, mode=3, bitrate_index=6),
             packer.generate(n_frames=k, seed=65, mode=2, mode_ext=0, bitrate_index=12)]
    mixed_mode = b"".join(parts)
    vparts = [packer.generate(n_frames=k, seed=66, mode=1, mode_ext=2, bitrate_index=12),
              packer.generate(n_frames=k, seed=67, version=1, sfreq=0, mode=1, mode_ext=2, bitrate_index=8, iso_strict=True),
              packer.generate(n_frames=k, seed=68, mode=3, bitrate_index=7),
              packer.generate(n_frames=k, seed=69, version=2, sfreq=1, mode=3, bitrate_index=6, iso_strict=True),
              packer.generate(n_frames=k, seed=70, version=1, sfreq=1, mode=0, bitrate_index=9, iso_strict=True)]
    return [("mixed/mono-stereo", mixed_mode, 0), ("mixed/mpeg1-lsf", b"".join(vparts), ISO_LSF)]


@functools.lru_cache(maxsize=None)
def gpu_streams():
    """(name, mp3, iso): the 18 streams of the clip tests on the GPU -- every family above and one of the C3 configuration (320 kbps
    joint stereo, 9600 frames: longer than the decoder's 8192-frame window)"""
    s = random_streams(range(1, 9), (200, 420))
    s += scfsi_streams(400) + h6_streams(400)
    s += corrupted_streams(range(3), 360) + mixed_streams(400)
    s.append(("c3-config", packer.generate(n_frames=9600, seed=0xC3, sfreq=0, mode=1, mode_ext=2, bitrate_index=14), 0))
    return s
