"""Planted envelopes for the beat kernels, for the host tests on the emulated kernels
(tests/test_clip_beat_host.py) and the device tests (tests/test_gpu_clip_beat_forms.py) alike: they stand here because both read
them and no test imports a test.  Numpy alone.  A helper module: no test, no fixture."""
import numpy as np

import clip_beat_ref as bref


def tie_envelope(period, n, seed=None):
    """An envelope whose programme holds ties on real tables: impulses P + 1 .. 2 P + 1 frames apart and nothing between them.
    The local score's taps fall below binary32's smallest number 0.46 P frames from an impulse, so ls is exactly 0 between two
    impulses' reach, and with a flat transition cost cum stays at the last peak's value over such a stretch: equal candidates"""
    rng = np.random.default_rng(period if seed is None else seed)
    o = np.zeros(n, dtype=np.float32)
    i = period // 2
    while i < n:
        o[i] = float(rng.integers(1, 4))
        i += period + int(rng.integers(1, period + 2))
    return o


def tied_frames(cum, period):
    """the frames of a programme with a flat transition cost whose best candidate is not alone"""
    h = bref.half(period)
    return sum(1 for i in range(2 * period, cum.size) if np.sum(cum[i - 2 * period:i - h + 1] == cum[i - 2 * period:i - h + 1].max()) > 1)
