"""MPEG-2 LSF / MPEG-2.5 through the device Huffman stage, without a GPU: the LSF-capable bits-mode scan
(pdmp3_amd_bulk_new_parse_bits_lsf, api.parse_bits(..., lsf=True)) hands the LSF form of pdmp3_frame_bits to
pdmp3_amd/csrc/unpack_core.h, compiled for the host (tests/host_emul), and the gc records that come out must be the
host stage's -- api.parse_like_cli(mp3, cap, ISO_LSF), itself pinned to FFmpeg by test_lsf_pin.py -- byte for byte:
for the 24 fixtures' streams, for version changes inside a stream, for any cut of the stream into windows, and for
corrupted streams.  The GPU half is tests/test_gpu_lsf_device_huffman.py."""
import ctypes as C

import numpy as np
import pytest

import iso_streams
from pdmp3_amd import api
from pdmp3_amd.packer import packer
from test_host_stage import _records_equal
from test_unpack_emul import emul_unpack

ISO_LSF = api.ISO_LSF
NAMES = list(iso_streams.LSF_STREAMS)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _lsf(name, **over):
    kw = dict(iso_streams.LSF_STREAMS[name])
    kw.update(over)
    return packer.generate(**kw)


def host_records(mp3, n):
    """the host stage's records of the stream's first n frames, and how many it built"""
    sp, sd = api.parse_like_cli(mp3, n + 8, ISO_LSF)
    return sp[:n], sd[:n], sp.shape[0]


def check_device_records(emul, mp3, cut_lists=()):
    """bits scan -> emulated device stage == host stage, whole and cut into the windows given (merge state carried)"""
    bits, res, nbytes = api.parse_bits(mp3, ISO_LSF, lsf=True)
    n = bits.shape[0]
    total, frames = api.scan_buffer(mp3, ISO_LSF)
    assert n == frames and nbytes == total
    sp_h, sd_h, n_h = host_records(mp3, n)
    assert n_h == n
    whole = emul_unpack(emul, bits, res)
    assert np.array_equal(whole[0], sp_h)
    assert np.array_equal(whole[1].view(np.uint8), sd_h.view(np.uint8))
    for cuts in cut_lists:
        cuts = sorted(set([0, n] + [c for c in cuts if 0 < c < n]))
        assert _records_equal(emul_unpack(emul, bits, res, cuts), whole), cuts
    return bits


def version_cuts(bits):
    """window boundaries where the engine's windows end: a change of version, or of an LSF stream's channel count"""
    mono = ((bits["frame"] >> 2) & 3) == 3
    kind = bits["lsf"].astype(np.int32) * 2 + (mono & (bits["lsf"] != 0))
    return [int(i) for i in np.nonzero(kind[1:] != kind[:-1])[0] + 1]


def test_legacy_bits_scan_still_stops_and_the_lsf_scan_does_not():
    mp3 = _lsf("lsf_22k_ms")
    old, _, _ = api.parse_bits(mp3, ISO_LSF)
    new, _, _ = api.parse_bits(mp3, ISO_LSF, lsf=True)
    assert old.shape[0] == 0 and new.shape[0] == api.scan_buffer(mp3, ISO_LSF)[1] > 0
    # without PDMP3_ISO_LSF an LSF stream is junk to either scan, as to the reference
    assert api.parse_bits(mp3, 0, lsf=True)[0].shape[0] == 0


@pytest.mark.parametrize("name", NAMES)
def test_lsf_fixture_device_records_are_the_host_stage_records(emul, name):
    mp3 = _lsf(name)
    bits = check_device_records(emul, mp3, [[1], list(range(0, 1000, 7)), list(range(0, 1000, 37))])
    ver = 1 if iso_streams.LSF_STREAMS[name]["version"] == 1 else 2
    assert (bits["lsf"] == ver).all() and not bits["gc"][:, 2:].view(np.uint8).any() and not bits["scfsi"].any()


@pytest.mark.parametrize("name", ["lsf_24k_msis", "lsf_8k_ms", "lsf_11k_mono"])
def test_long_lsf_streams_in_windows(emul, name):
    """a few hundred frames: scalefactor / count1 state carried over windows of 1, 7 and 37 frames"""
    mp3 = _lsf(name, n_frames=300, seed=iso_streams.LSF_STREAMS[name]["seed"] + 100)
    check_device_records(emul, mp3, [[1, 2, 3], list(range(0, 400, 7)), list(range(0, 400, 37))])


@pytest.mark.parametrize("order", ["mpeg1_lsf_mpeg1", "lsf_mpeg1_lsf"])
def test_version_changes_inside_a_stream(emul, order):
    """MPEG-1 -> LSF -> MPEG-1 and LSF -> MPEG-1 -> LSF in one stream (and a stereo LSF part next to a mono one), with the
    windows cut where the engine cuts them -- at every change of version or LSF channel count -- and elsewhere"""
    m1 = packer.generate(n_frames=40, seed=71, mode=1, mode_ext=2, bitrate_index=9, block_pct=(60, 10, 20, 10))
    m2 = packer.generate(n_frames=30, seed=72, mode=3, sfreq=1, bitrate_index=5)
    l1 = _lsf("lsf_16k_msis")
    l2 = _lsf("lsf_8k_mono")
    l3 = _lsf("lsf_24k_stereo")
    mp3 = m1 + l1 + l2 + m2 if order == "mpeg1_lsf_mpeg1" else l3 + m1 + l2 + l1
    bits, _, _ = api.parse_bits(mp3, ISO_LSF, lsf=True)
    vc = version_cuts(bits)
    assert len(vc) >= 3 and (bits["lsf"] == 0).any() and (bits["lsf"] != 0).any()
    check_device_records(emul, mp3, [vc, vc + [5, 11], sorted(set(vc + list(range(0, 300, 7))))])


def test_lsf_pool_rows_are_the_snapshot_rows(emul):
    """the compact input of LSF frames (8-bit main_data_begin, 9 / 17-byte side info, CRC): the rows rebuilt by the
    device's rule are byte for byte the reservoir snapshots, on clean, mixed-version, truncated and corrupted streams"""
    rs = np.random.RandomState(13)
    bases = [_lsf(n, n_frames=200, seed=iso_streams.LSF_STREAMS[n]["seed"] + 7) for n in
             ("lsf_22k_ms", "lsf_24k_mono", "lsf_16k_msis", "lsf_11k_stereo", "lsf_12k_mono", "lsf_8k_msis")]
    bases.append(packer.generate(n_frames=60, seed=73, bitrate_index=11) + bases[0] + bases[1])
    streams = [np.frombuffer(b, dtype=np.uint8) for b in bases] + [np.frombuffer(bases[2][:-300], dtype=np.uint8)]
    for it in range(40):
        m = np.frombuffer(bases[rs.randint(len(bases))], dtype=np.uint8).copy()
        for p in rs.randint(0, len(m), size=1 + rs.randint(0, 40)):
            m[p] ^= 1 << rs.randint(0, 8)
        streams.append(m)
    checked = 0
    for m in streams:
        try:
            bits, res, _ = api.parse_bits(m, ISO_LSF, lsf=True)
        except api.RingReplay:
            continue
        bits2, desc, pool = api.parse_pool(m, ISO_LSF, lsf=True)
        assert len(bits2) == len(bits) and np.array_equal(bits2.view(np.uint8), bits.view(np.uint8))
        if not len(bits):
            continue
        rows = np.zeros((len(bits), 2064), dtype=np.uint8)
        emul.emul_rows(_p(desc), _p(pool), len(bits), _p(rows))
        assert np.array_equal(rows, res)
        checked += len(bits)
    assert checked > 3000


def test_lsf_unpack_fuzz_matches_host_stage(emul):
    """bit flips, byte splats and truncation in LSF streams of all six rates and four channel modes (2 016 streams):
    whatever the host stage builds from a broken stream -- region counts past band 22, part2_3_length running off the
    reservoir, a 9-bit scalefac_compress in the intensity code, count1 wrapping below zero -- the device logic builds
    the same records, with random window cuts"""
    rs = np.random.RandomState(2024)
    streams = done = frames = 0
    for name in NAMES:
        kw = iso_streams.LSF_STREAMS[name]
        orig = np.frombuffer(_lsf(name, n_frames=40, seed=kw["seed"] + 500), dtype=np.uint8)
        for it in range(84):
            m = orig.copy()
            kind = it % 3
            for p in rs.randint(0, len(m), size=1 + rs.randint(0, 6 if kind == 0 else 60)):
                m[p] = rs.randint(0, 256) if kind == 2 else m[p] ^ (1 << rs.randint(0, 8))
            if it % 5 == 4:
                m = m[:rs.randint(1, len(m))]
            m = np.ascontiguousarray(m)
            streams += 1
            try:
                bits, res, _ = api.parse_bits(m, ISO_LSF, lsf=True)
            except api.RingReplay:
                continue
            n = bits.shape[0]
            sp_h, sd_h, n_h = host_records(m.tobytes(), n)
            assert n_h == n, (name, it)
            if not n:
                continue
            cuts = sorted(set([0, n] + rs.randint(0, n, size=rs.randint(0, 5)).tolist()))
            got = emul_unpack(emul, bits, res, cuts)
            assert np.array_equal(got[0], sp_h), (name, it)
            assert np.array_equal(got[1].view(np.uint8), sd_h.view(np.uint8)), (name, it)
            done += 1
            frames += n
    assert streams >= 2000 and done > 1500 and frames > 40000, (streams, done, frames)
