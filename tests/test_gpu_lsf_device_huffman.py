"""MPEG-2 LSF / MPEG-2.5 through the device Huffman stage on the GPU (PDMP3_ISO_LSF): the records k_unpack / k_merge_apply
build from the LSF form of pdmp3_frame_bits are the host stage's, byte for byte, and a device-Huffman whole-stream decoder
decodes LSF, MPEG-1 and mixed-version streams itself -- every frame's scalefactors and Huffman data on the device
(pdmp3_amd_bulk_huffman_frames), the same PCM as a host-Huffman decoder and the streaming API, FFmpeg's within the bars of
tests/iso_streams.py, to pageable, pinned and device memory.  The CPU half is tests/test_lsf_unpack_emul.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import iso_streams
from test_lsf_pin import ISO_LSF, ffmpeg_error, load_lsf_fixture

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(iso_streams.LSF_STREAMS)


def _mixed_streams():
    from pdmp3_amd.packer import packer
    m1 = packer.generate(n_frames=60, seed=81, mode=1, mode_ext=2, bitrate_index=9, block_pct=(60, 10, 20, 10))
    l1, _, _ = load_lsf_fixture("lsf_16k_msis")
    l2, _, _ = load_lsf_fixture("lsf_8k_mono")
    l3, _, _ = load_lsf_fixture("lsf_24k_stereo")
    tag = b"ID3\x03\x00\x00\x00\x00\x00\x21" + bytes(33)
    return {"lsf_16k_msis": l1, "mpeg1": m1, "tag + lsf_8k_mono": tag + l2, "mpeg1 + lsf + lsf + mpeg1": m1 + l1 + l2 + m1,
            "lsf + mpeg1 + lsf": l3 + m1 + l1, "lsf_24k_stereo": l3}


def test_device_unpack_builds_the_host_stage_records_of_lsf_windows(engine):
    """pdmp3_hip_stream_set_lsf + pdmp3_hip_stream_submit_bits on the LSF form of the side info: the records fetched back are
    api.parse_like_cli's (the host stage's), in windows of 13 frames and in windows cut where the version or an LSF stream's
    channel count changes, the scalefactor / count1 state carried over MPEG-1 and LSF windows alike"""
    from pdmp3_amd import api, hip
    lib = hip.load_library()
    vp = C.c_void_p
    lib.pdmp3_hip_stream_create_slots.argtypes = [vp, C.c_int, C.c_int, C.POINTER(vp)]
    for f in ("pdmp3_hip_stream_slot_bits", "pdmp3_hip_stream_slot_reservoir"):
        getattr(lib, f).restype = vp
        getattr(lib, f).argtypes = [vp, C.c_int]
    lib.pdmp3_hip_stream_submit_bits.argtypes = [vp, C.c_int, C.c_int]
    lib.pdmp3_hip_stream_set_lsf.argtypes = [vp, C.c_int]
    lib.pdmp3_hip_stream_wait.argtypes = [vp, C.c_int]
    lib.pdmp3_hip_stream_reset.argtypes = [vp]
    lib.pdmp3_hip_stream_fetch_records.argtypes = [vp, C.c_int, C.c_int, vp, vp]
    lib.pdmp3_hip_stream_destroy.argtypes = [vp]
    per = 64
    hs = vp()
    assert lib.pdmp3_hip_stream_create_slots(engine.h, per, 2, C.byref(hs)) == 0
    streams = {n: load_lsf_fixture(n)[0] for n in NAMES}
    streams.update(_mixed_streams())
    try:
        for name, mp3 in streams.items():
            bits, res, _ = api.parse_bits(mp3, ISO_LSF, lsf=True)
            n = bits.shape[0]
            sp_h, sd_h = api.parse_like_cli(mp3, n + 8, ISO_LSF)
            assert sp_h.shape[0] == n, name
            mono = ((bits["frame"] >> 2) & 3) == 3
            kind = bits["lsf"].astype(np.int32) * 2 + (mono & (bits["lsf"] != 0))
            changes = [int(i) for i in np.nonzero(kind[1:] != kind[:-1])[0] + 1]
            for step in (13, per):
                cuts = sorted(set([0, n] + changes + list(range(0, n, step))))
                assert lib.pdmp3_hip_stream_reset(hs) == 0
                sp = np.zeros_like(sp_h)
                sd = np.zeros_like(sd_h)
                for w, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
                    k, slot = b - a, w % 2
                    C.memmove(lib.pdmp3_hip_stream_slot_bits(hs, slot), bits[a:].ctypes.data, k * 80)
                    C.memmove(lib.pdmp3_hip_stream_slot_reservoir(hs, slot), res[a:].ctypes.data, k * 2064)
                    assert lib.pdmp3_hip_stream_set_lsf(hs, int(bits["lsf"][a] != 0)) == 0
                    assert lib.pdmp3_hip_stream_submit_bits(hs, slot, k) == 0
                    assert lib.pdmp3_hip_stream_wait(hs, slot) == 0
                    assert lib.pdmp3_hip_stream_fetch_records(hs, slot, k, sp[a:].ctypes.data, sd[a:].ctypes.data) == 0
                assert np.array_equal(sp, sp_h), (name, step)
                assert np.array_equal(sd.view(np.uint8), sd_h.view(np.uint8)), (name, step)
    finally:
        lib.pdmp3_hip_stream_destroy(hs)


@pytest.mark.parametrize("name", NAMES)
def test_device_huffman_decoder_decodes_lsf_itself(name):
    """every frame of the fixture through the device stage (none through the host pool), the PCM of a host-Huffman decoder and
    of the streaming API, FFmpeg's within the fixture's bar -- to pageable, pinned and device memory"""
    import torch
    from pdmp3_amd import api
    mp3, theirs, kw = load_lsf_fixture(name)
    nch = iso_streams.nch_of(kw)
    total, frames = api.scan_buffer(mp3, ISO_LSF)
    d = api.Decoder()
    try:
        d.set_quirks(ISO_LSF)
        stream = np.frombuffer(api.decode_like_cli(mp3, d), dtype=np.int16)
    finally:
        d.close()
    h = api.BulkDecoder(threads=2, window_frames=16, host_huffman=True)
    try:
        h.set_quirks(ISO_LSF)
        host = h.decode(mp3)
        assert h.huffman_frames() == (0, frames)
    finally:
        h.close()
    assert np.array_equal(host, stream)
    mx, _ = ffmpeg_error(host.reshape(-1, nch).astype(np.float64) * (32768.0 / 32767.0), theirs)
    assert mx <= iso_streams.LSF_TOL_S16_LSB[name], mx
    for window in (16, 0):
        b = api.BulkDecoder(threads=2, window_frames=window)
        try:
            b.set_quirks(ISO_LSF)
            assert np.array_equal(b.decode(mp3), host), window
            pinned = api.PinnedPCM(total // 2)
            try:
                got, rate, ch = b.decode_into(mp3, pinned.array)
                assert got == total and rate == iso_streams.lsf_rate_of(kw) and ch == nch
                assert np.array_equal(pinned.array[:total // 2], host), window
            finally:
                pinned.free()
            dev = torch.full((total // 2 + 64,), 0x5A5A, dtype=torch.int16, device="cuda")
            torch.cuda.synchronize()
            got, _, _ = b.decode_into_device(mp3, dev)
            assert got == total
            out = dev.cpu().numpy()
            assert np.array_equal(out[:total // 2], host), window
            assert (out[total // 2:] == 0x5A5A).all()                     # nothing written past the stream's PCM
            assert b.huffman_frames() == (3 * frames, 0)
        finally:
            b.close()


def test_decode_many_mixes_lsf_mpeg1_and_tagged_streams():
    """decode_many / decode_into_async over LSF, MPEG-1, tagged and mixed-version streams back to back: each stream's PCM is
    what it is decoded alone, and every frame went through the device stage"""
    from pdmp3_amd import api
    streams = list(_mixed_streams().values())
    alone = []
    for m in streams:
        b = api.BulkDecoder(threads=2, window_frames=16)
        try:
            b.set_quirks(ISO_LSF)
            alone.append(b.decode(m))
        finally:
            b.close()
    h = api.BulkDecoder(threads=2, window_frames=16, host_huffman=True)
    try:
        h.set_quirks(ISO_LSF)
        for m, a in zip(streams, alone):
            assert np.array_equal(h.decode(m), a)
    finally:
        h.close()
    frames = sum(api.scan_buffer(m, ISO_LSF)[1] for m in streams)
    for window in (16, 0):
        b = api.BulkDecoder(threads=2, window_frames=window)
        try:
            b.set_quirks(ISO_LSF)
            for rnd in range(2):
                outs = b.decode_many(streams + streams[::-1])
                for got, want in zip(outs, alone + alone[::-1]):
                    assert np.array_equal(got, want), (window, rnd)
            assert b.huffman_frames() == (4 * frames, 0)
        finally:
            b.close()


_CHILD = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
from pdmp3_amd import api
mp3 = open(sys.argv[2], "rb").read()
b = api.BulkDecoder(threads=2)
b.set_quirks(0x40)
total, frames = api.scan_buffer(mp3, 0x40)
dev = torch.zeros(total // 2, dtype=torch.int16, device="cuda")
torch.cuda.synchronize()
got, _, _ = b.decode_into_device(mp3, dev)
torch.cuda.synchronize()
np.save(sys.argv[3], dev.cpu().numpy())
print("RESULT", got, total, frames, *b.split_scans(), *b.huffman_frames())
b.close()
"""


def test_trailing_lsf_frames_on_the_split_scan(tmp_path):
    """the split scan (four scanners, PCM left on the device) meets LSF frames only at the stream's end: the stream is given
    up and decoded by the one-thread scan, LSF frames included -- the PCM and the frame count of a host-Huffman decoder"""
    from pdmp3_amd import api
    from pdmp3_amd.packer import packer
    lsf = packer.generate(**dict(iso_streams.LSF_STREAMS["lsf_22k_ms"], n_frames=10))
    mp3 = packer.generate(n_frames=4200, seed=91, mode=1, mode_ext=2, bitrate_index=9) + lsf
    total, frames = api.scan_buffer(mp3, ISO_LSF)
    assert frames > api.scan_buffer(mp3, 0)[1] and frames > 4200            # (the LSF frames that are not in the last 1152 bytes count)
    h = api.BulkDecoder(threads=2, host_huffman=True)
    try:
        h.set_quirks(ISO_LSF)
        want = h.decode(mp3)
    finally:
        h.close()
    assert want.size * 2 == total
    src, out = tmp_path / "s.mp3", tmp_path / "pcm.npy"
    src.write_bytes(mp3)
    env = dict(os.environ, PDMP3_BULK_SCAN_THREADS="4")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(src), str(out)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("RESULT")][0].split()[1:]
    got, tot, nf, taken, given_up, dev, host = (int(x) for x in line)
    assert got == tot == total and nf == frames
    assert given_up == 1 and taken == 0 and (dev, host) == (frames, 0)
    assert np.array_equal(np.load(out), want)
