"""The destination check every decode_clips_* call shares (pdmp3_amd/api.py _clip_destination): which arrays it takes, and the
address of row 0, the bytes between rows and the floats between channels it hands to the library.  numpy only, no GPU, no
library: the expected values come from arr.ctypes.data and arr.strides."""
import numpy as np
import pytest

from pdmp3_amd.api import _clip_destination

K, C = 3, 2
# the three inner shapes: audio's (t,), mel's (n_mels, f), Kaldi's (f, d)
INNERS = [(19,), (5, 7), (7, 4)]


def _want(arr):
    return arr.ctypes.data, arr.strides[0], arr.strides[1] // 4


@pytest.mark.parametrize("inner", INNERS)
def test_dense(inner):
    a = np.zeros((K, C) + inner, np.float32)
    got = _clip_destination(a, K, C, inner)
    assert got == _want(a)
    n = int(np.prod(inner))
    assert got[1] == 4 * C * n and got[2] == n


@pytest.mark.parametrize("inner", INNERS)
def test_guard_row_between_rows(inner):
    """every other row of a [2 K] array: the rows are two rows' bytes apart"""
    big = np.zeros((2 * K, C) + inner, np.float32)
    a = big[::2]
    got = _clip_destination(a, K, C, inner)
    assert got == _want(a)
    assert got[0] == big.ctypes.data and got[1] == 2 * big.strides[0] and got[2] == int(np.prod(inner))


@pytest.mark.parametrize("inner", INNERS)
def test_padded_channel_stride(inner):
    """the channels of a row with three floats (audio: in the one dimension) or a whole line of padding between them"""
    if len(inner) == 1:
        big = np.zeros((K, C, inner[0] + 3), np.float32)
        a = big[:, :, :inner[0]]
        pad = 3
    else:
        big = np.zeros((K, C, inner[0] + 1, inner[1]), np.float32)
        a = big[:, :, :inner[0]]
        pad = inner[1]
    got = _clip_destination(a, K, C, inner)
    assert got == _want(a)
    assert got[2] == int(np.prod(inner)) + pad and got[1] == 4 * C * got[2]


@pytest.mark.parametrize("inner", INNERS)
def test_more_rows_than_clips(inner):
    a = np.zeros((K + 2, C) + inner, np.float32)
    assert _clip_destination(a, K, C, inner) == _want(a)
    with pytest.raises(AssertionError):
        _clip_destination(a, K + 3, C, inner)


def test_one_channel():
    a = np.zeros((K, 1, 5, 7), np.float32)
    assert _clip_destination(a, K, 1, (5, 7)) == _want(a)


def test_complex64_as_pairs():
    """complex64 [K, C, bins, F] is float32 [K, C, bins, F, 2]; so is the float32 array of that shape itself"""
    z = np.zeros((K, C, 5, 7), np.complex64)
    got = _clip_destination(z, K, C, (5, 7, 2), True)
    assert got == (z.ctypes.data, z.strides[0], z.strides[1] // 4)
    assert got[2] == 5 * 7 * 2
    f = np.zeros((K, C, 5, 7, 2), np.float32)
    assert _clip_destination(f, K, C, (5, 7, 2), True) == _want(f)
    zz = np.zeros((2 * K, C, 6, 7), np.complex64)[::2, :, :5]                      # guard rows and a padded channel stride
    got = _clip_destination(zz, K, C, (5, 7, 2), True)
    assert got == (zz.ctypes.data, zz.strides[0], zz.strides[1] // 4) and got[2] == 6 * 7 * 2


@pytest.mark.parametrize("k,inner", [(K, (0,)), (K, (5, 0)), (K, (0, 4)), (0, (19,)), (0, (5, 7)), (0, (7, 4)), (0, (5, 0))])
def test_zero_size(k, inner):
    a = np.zeros((k, C) + inner, np.float32)
    assert _clip_destination(a, k, C, inner) == _want(a)


def test_zero_size_complex():
    z = np.zeros((K, C, 5, 0), np.complex64)
    v = z.view(np.float32).reshape(z.shape + (2,))                                # (numpy gives an empty array's view strides of its own)
    assert v.ctypes.data == z.ctypes.data
    assert _clip_destination(z, K, C, (5, 0, 2), True) == _want(v)


@pytest.mark.parametrize("inner", INNERS)
def test_refused(inner):
    n = int(np.prod(inner))
    with pytest.raises(AssertionError):                                            # wrong inner shape
        _clip_destination(np.zeros((K, C) + inner[:-1] + (inner[-1] + 1,), np.float32), K, C, inner)
    with pytest.raises(AssertionError):                                            # wrong channel count
        _clip_destination(np.zeros((K, 1) + inner, np.float32), K, C, inner)
    with pytest.raises(AssertionError):                                            # a dimension too few
        _clip_destination(np.zeros((K, C * n), np.float32), K, C, inner)
    with pytest.raises(AssertionError):                                            # float64
        _clip_destination(np.zeros((K, C) + inner, np.float64), K, C, inner)
    with pytest.raises(AssertionError):                                            # int32: four bytes, but no floats
        _clip_destination(np.zeros((K, C) + inner, np.int32), K, C, inner)
    with pytest.raises(AssertionError):                                            # the innermost dimension not dense
        _clip_destination(np.zeros((K, C) + inner[:-1] + (2 * inner[-1],), np.float32)[..., ::2], K, C, inner)
    with pytest.raises(AssertionError):                                            # complex where the call writes floats
        _clip_destination(np.zeros((K, C) + inner, np.complex64), K, C, inner + (2,))
    with pytest.raises(AssertionError):
        _clip_destination(np.zeros((K, C) + inner, np.complex64), K, C, inner)


def test_refused_inner_lines_apart():
    """two-dimensional inner shapes: lines with padding between them are no dense row"""
    for inner in INNERS[1:]:
        a = np.zeros((K, C, inner[0], inner[1] + 2), np.float32)[..., :inner[1]]
        with pytest.raises(AssertionError):
            _clip_destination(a, K, C, inner)
    z = np.zeros((K, C, 5, 9), np.complex64)[..., :7]
    with pytest.raises(AssertionError):
        _clip_destination(z, K, C, (5, 7, 2), True)


def test_refused_misaligned_stride():
    """a float32 row at a stride that is no multiple of four bytes"""
    raw = np.zeros(K * (C * 19 * 4 + 2), np.uint8)
    a = np.lib.stride_tricks.as_strided(raw.view(np.uint8)[:4].view(np.float32), shape=(K, C, 19), strides=(C * 19 * 4 + 2, 19 * 4, 4))
    with pytest.raises(AssertionError):
        _clip_destination(a, K, C, (19,))
