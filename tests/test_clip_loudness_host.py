"""The loudness of clips on the host, no GPU: the K-weighting's coefficients against the standard's
table, the tables of the blocked filter against the reference's restatement and the sample loop, the refusals of the planning
calls, and the kernels' own indexing and arithmetic (pdmp3_amd/csrc/loudness_core.h, compiled here with g++ into
tests/host_emul/loudness_emul.cpp's loops) against the binary64 definition within the derived bound -- every field of stats,
every momentary value, the audio times g bit for bit."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import clip_loudness_ref as ref
import test_clip_cqt_host as tch
from clip_host import build_emul, run_sanitizer_program

RATES = [8000, 22050, 48000]
MPEG_RATES = [8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000]
BS1770_48K = ([1.53512485958697, -2.69169618940638, 1.19839281085285], [1.0, -1.69065929318241, 0.73248077421585],
              [1.0, -2.0, 1.0], [1.0, -1.99004745483398, 0.99007225036621])


class LoudParams(C.Structure):                     # include/pdmp3_hip.h pdmp3_loud_params
    _fields_ = [("n_in", C.c_int64), ("channels", C.c_int32), ("q", C.c_int32), ("n_chunks", C.c_int32), ("n_sub", C.c_int32),
                ("n_mom", C.c_int32), ("dual_mono", C.c_int32), ("target", C.c_double), ("peak_limit", C.c_double)]


def _api():
    from pdmp3_amd import api
    return api


def _emul():
    lib = build_emul("loudness")
    lib.emul_clip_loudness.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    assert lib.emul_loudness_params_bytes() == C.sizeof(LoudParams)
    assert lib.emul_loudness_tables_bytes() == (70 * 16 + 4 * 64) * 8 + (64 * 64 + 64 * 4) * 4
    return lib


@functools.lru_cache(maxsize=None)
def _tables_blob(fs):
    hm, o, _, r, pw = _api().loudness_tables(fs)
    return np.frombuffer(pw.tobytes() + r.tobytes() + hm.tobytes() + o.tobytes(), dtype=np.uint8).copy()


def emulate(x, fs, dual_mono=False, target=None, peak_limit=0.0):
    """x float32 [C, T] -> (audio [C, T], stats [8], momentary [J]) of the emulated kernels"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    Cn, T = x.shape
    b, chunk, lds, q, nc, I, J = _api().loudness_plan(fs, T)
    P = LoudParams(T, Cn, q, nc, I, J, int(dual_mono), float("nan") if target is None else target, peak_limit)
    Ts = (T + 3) & ~3
    src = np.full((Cn, Ts), 7e29, dtype=np.float32)               # (the floats behind a row's end are not the kernel's to read)
    src[:, :T] = x
    out = np.full((Cn, T + 8), -5.0, dtype=np.float32)
    d = tch.MelDesc(src.ctypes.data, out.ctypes.data, Ts, T + 8, 0, 0)
    stats, mom = np.full(8 + 2, -5.0, dtype=np.float32), np.full(J + 2, -5.0, dtype=np.float32)
    tab = _tables_blob(fs)
    assert _emul().emul_clip_loudness(C.byref(d), 1, tab.ctypes.data, C.byref(P), stats.ctypes.data, mom.ctypes.data) == 0
    assert (out[:, T:] == -5.0).all() and (stats[8:] == -5.0).all() and (mom[J:] == -5.0).all()
    return out[:, :T].copy(), stats[:8].copy(), mom[:J].copy()


# ---- 1. coefficients ----
def test_coefficients_are_the_standards_table_at_48k():
    c = _api().loudness_coefficients(48000)
    want = np.array(BS1770_48K).reshape(2, 2, 3)
    assert np.abs(c - want).max() <= 1e-12
    assert np.abs(ref.coefficients(48000) - want).max() <= 1e-12
    for fs in MPEG_RATES + [96000]:
        assert np.abs(_api().loudness_coefficients(fs) - ref.coefficients(fs)).max() <= 1e-15


def test_a_full_scale_997_hz_sine_measures_minus_3_01():
    fs = 48000
    x = np.sin(2.0 * np.pi * 997.0 * np.arange(2 * fs) / fs)[None, :].astype(np.float32)
    m = ref.measure(x, fs)
    assert abs(m.L - (-3.0103)) <= 0.01 and abs(m.M - (-3.0103)) <= 0.01, (m.L, m.M)


@pytest.mark.parametrize("fs", MPEG_RATES + [96000])
def test_poles_lie_inside_the_unit_circle(fs):
    for f in _api().loudness_coefficients(fs):
        assert (np.abs(np.roots(f[1])) < 1.0).all()


# ---- 2. tables ----
@pytest.mark.parametrize("fs", RATES + [44100, 96000])
def test_tables_are_the_restatement_and_the_sample_loop(fs):
    hm, o, phi, r, pw = _api().loudness_tables(fs)
    Hm, O, Phi, R = ref.tables(fs)
    assert (hm == Hm.astype(np.float32)).all() and (o == O.astype(np.float32)).all()
    assert np.abs(phi - Phi).max() <= 1e-12 * max(1.0, np.abs(Phi).max()) and np.abs(r - R).max() <= 1e-12
    assert (hm[np.triu_indices(64, 1)] == 0).all()
    tol = 1e-12 * max(1.0, np.abs(Phi).max())           # (absolute: the powers decay, their roundings do not)
    want = ref.powers(fs, 128)
    assert np.abs(pw[:65] - want[:65]).max() <= tol and np.abs(pw[65] - want[128]).max() <= tol and (pw[1] == phi).all()
    for k in range(66, 70):                             # Phi^(64 2^(k - 64)): the square of the one before
        assert np.abs(pw[k] - pw[k - 1] @ pw[k - 1]).max() <= 1e-9 * max(1.0, np.abs(Phi).max())
    # Hm times an impulse train plus O times a state is the sample loop; the state behind the block too
    rng = np.random.default_rng(fs)
    u, s = rng.standard_normal(64), rng.standard_normal(4)
    y, st = ref.kweight(np.concatenate([u, [0.0]]), fs, state=s, states_every=64)
    assert np.abs(Hm @ u + O @ s - y[:64]).max() <= 1e-12 * np.abs(y).max()
    assert np.abs(Phi @ s + R @ u - st[1]).max() <= 1e-12 * max(1.0, np.abs(st[1]).max())


def test_the_plan_is_the_restatement():
    for fs in MPEG_RATES + [96000, 192000]:
        for T in (0, 1, 4095, 4096, 4097, 4 * ((fs + 5) // 10) - 1, 4 * ((fs + 5) // 10), 123457):
            got = _api().loudness_plan(fs, T)
            want = ref.plan(fs, T)
            assert got == (want["B"], want["chunk"], want["lds_bytes"], want["q"], want["n_chunks"], want["I"], want["J"])


# ---- 3. scipy ----
def test_the_sample_loop_is_scipys_lfilter():
    sig = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(3)
    for fs in RATES:
        x = rng.standard_normal((2, 3000))
        (b1, a1), (b2, a2) = ref.coefficients(fs)
        want = sig.lfilter(b2, a2, sig.lfilter(b1, a1, x, axis=-1), axis=-1)
        assert np.abs(ref.kweight(x, fs) - want).max() <= 1e-12 * np.abs(want).max()


# ---- 4., 5. the emulation within the bound ----
def _signal(kind, Cn, T, fs, seed):
    rng = np.random.default_rng(seed)
    n = 0.1 * rng.standard_normal((Cn, T))
    t = np.arange(T)
    if kind == "dc":
        n = 0.5 + n
    elif kind == "sine":
        n = np.stack([0.5 * np.sin(2.0 * np.pi * 440.0 * (c + 1) * t / fs) for c in range(Cn)])
    elif kind == "silence":
        n = np.zeros((Cn, T))
    elif kind == "step":
        n[:, T // 2:] *= 10.0 ** (-30.0 / 20.0)
    elif kind == "tail":
        n[:, T // 2:] = 0.0
    return n.astype(np.float32)


def _check(x, fs, **kw):
    m = ref.measure(x, fs, **kw)
    audio, stats, mom = emulate(x, fs, **kw)
    worst = ref.check_stats(m, stats, mom)
    assert (audio.view(np.uint32) == (x * np.float32(stats[3])).astype(np.float32).view(np.uint32)).all()
    return m, stats, worst


@pytest.mark.parametrize("kind", ["noise", "dc", "sine", "silence", "step", "tail"])
def test_signals_within_the_bound(kind):
    fs = 8000
    T = 12 * 800 + 37
    for Cn in (1, 2):
        x = _signal(kind, Cn, T, fs, 11 + Cn)
        m, stats, worst = _check(x, fs)
        assert not m.undecided
        print("%s C=%d: L %.4f worst error / bound %.3g, margin %.3g dB" % (kind, Cn, m.L, worst, m.margin))
        if kind == "silence":
            assert (stats == np.array([-np.inf, -np.inf, 0, 1, -np.inf, m.J, 0, 0], dtype=np.float32)).all() and worst == 0.0
        else:
            assert 0.0 < worst <= 1.0
        if kind == "step":
            assert m.nGt < m.nA == m.J
        if kind == "tail":
            assert m.nA < m.J


def _shapes(fs):
    q = (fs + 5) // 10
    b, chunk = _api().loudness_plan(fs, 1)[:2]
    big = max(3 * b * chunk + b + 5, 6 * q + 37)
    return [4 * q - 1, 4 * q, 4 * q + 1, 5 * q + b // 2 + 3, big]


@pytest.mark.parametrize("fs", RATES)
def test_shapes_within_the_bound(fs):
    for i, T in enumerate(_shapes(fs)):
        for Cn, dual in ((1, False), (1, True), (2, False)):
            x = _signal("noise", Cn, T, fs, 100 + i)
            m, stats, worst = _check(x, fs, dual_mono=dual)
            assert stats[5] == max(0, T // ((fs + 5) // 10) - 3)
            if m.J:
                assert 0.0 < worst <= 1.0 and not m.undecided
            else:
                assert (stats[[0, 1, 4]] == -np.inf).all() and stats[3] == 1.0 and stats[2] == np.abs(x).max()
            if dual and m.J:
                mono = ref.measure(x, fs)
                assert abs(float(stats[0]) - (mono.L + 10.0 * math.log10(2.0))) <= m.dL + 2e-6 * abs(m.L)


def chain_signal(T, fs, seed):
    """mono noise with two level steps inside: 0.1 rms over the first quarter, 30 dB less from there on, an offset of 0.25
    under the last two chunks in front of chunk 64 (it loads the high-pass's slow poles), and exact zeros from seven samples
    in front of chunk 64 on.  What the rows behind the 64th chunk hold is then the decay of the state that k_loud_chain
    carried out of lane 63, and nothing else: a wrong carry is wrong by the size of the values themselves"""
    x = _signal("noise", 1, T, fs, seed)
    x[:, T // 4:] *= np.float32(10.0 ** (-30.0 / 20.0))
    x[:, 62 * 4096:] += np.float32(0.25)
    x[:, 64 * 4096 - 7:] = 0.0
    return x


@pytest.mark.parametrize("fs,T", [(48000, 64 * 4096), (48000, 64 * 4096 + 1), (48000, 128 * 4096), (48000, 128 * 4096 + 1), (192000, 128 * 4096 + 1)])
def test_the_chain_at_the_edges_of_its_steps(fs, T):
    """k_loud_chain takes 64 chunks a step: exactly one step, one step and a chunk of a single sample (the guards of a step
    whose other lanes lie behind n_chunks), two steps, two and a sample.  The signal ends in front of chunk 64, so the first
    sub-blocks behind it are the carried state's decay.  At 48 000 Hz that state is gone a chunk later (4096 samples are 20
    time constants of the high-pass), and the carry's way into the step's other lanes, Phi^64 times it, moves nothing; at
    192 000 Hz a chunk is 5 time constants and sub-block 14, which begins inside chunk 65, is held by that path alone.
    L, Gamma, the counts and the whole momentary curve against the binary64 definition (its sample loop run by scipy's
    lfilter, which test_the_sample_loop_is_scipys_lfilter holds to 1e-12: the rows are half a million samples long)"""
    pytest.importorskip("scipy.signal")
    import clip_r128_ref
    q = (fs + 5) // 10
    n_chunks = _api().loudness_plan(fs, T)[4]
    assert n_chunks == (T + 4095) // 4096 and n_chunks in (64, 65, 128, 129)
    x = chain_signal(T, fs, 640 + n_chunks)
    m = clip_r128_ref._loudness_measure(x, fs)
    audio, stats, mom = emulate(x, fs)
    worst = ref.check_stats(m, stats, mom)
    print("fs %d T %d, %d chunks: L %.4f J %d |A| %d |Gt| %d worst error / bound %.3g, margin %.3g dB" % (fs, T, n_chunks, m.L, m.J, m.nA, m.nGt, worst, m.margin))
    assert not m.undecided and 0 < m.nGt < m.nA <= m.J and 0.0 < worst <= 1.0
    if n_chunks > 65:
        # the windows that begin behind the signal's end: the state's decay, well above the bound's floor, and held two-sidedly
        j = (64 * 4096 + q - 1) // q
        k = (65 * 4096 + q - 1) // q if fs == 192000 else j
        assert m.nA < m.J and np.isfinite(m.l[k]) and m.ez[k] < 1e-3 * m.z[k] and m.l[j - 4] > m.l[k] + 20.0
    assert (audio.view(np.uint32) == x.view(np.uint32)).all() and stats[3] == 1.0


# ---- 6. gain ----
def test_gain():
    fs = 8000
    x = _signal("noise", 2, 10 * 800, fs, 5)
    m, stats, _ = _check(x, fs)
    assert stats[3] == 1.0 and m.g == 1.0
    m, stats, _ = _check(x, fs, target=-14.0)
    assert stats[3] != 1.0 and not m.limited and abs(float(stats[3]) - m.g) <= m.dg + 2.0 ** -23 * m.g
    x[1, 4321] = -0.9                                   # (a click: g P exceeds the limit)
    m, stats, _ = _check(x, fs, target=-14.0, peak_limit=0.5)
    assert m.limited and np.float32(stats[3]) == np.float32(0.5 / float(np.abs(x).max()))
    m, stats, _ = _check(x, fs, target=-30.0, peak_limit=0.9)
    assert not m.limited and not m.undecided


# ---- 7. refusals ----
def test_refusals_of_the_planning_calls():
    api = _api()
    assert api.loudness_check(48000, 1) and api.loudness_check(8000, 2, target=-70.0) and api.loudness_check(192000, 1, target=0.0, dual_mono=True)
    assert api.loudness_check(44100, 2, peak_limit=0.5)
    for fs in (7999, 192001, 0, -1):
        assert not api.loudness_check(fs, 1)
        with pytest.raises(ValueError):
            api.loudness_coefficients(fs)
        with pytest.raises(ValueError):
            api.loudness_tables(fs)
        with pytest.raises(ValueError):
            api.loudness_plan(fs, 100)
    for kw in (dict(target=-70.1), dict(target=0.1), dict(target=float("inf")), dict(target=-float("inf")), dict(peak_limit=-0.1),
               dict(peak_limit=float("inf")), dict(peak_limit=float("nan")), dict(dual_mono=2), dict(dual_mono=-1)):
        assert not api.loudness_check(48000, 1, **kw), kw
    assert not api.loudness_check(48000, 2, dual_mono=True) and not api.loudness_check(48000, 0) and not api.loudness_check(48000, 3)
    for T in (-1, 2 ** 31 - 3, 2 ** 31):
        with pytest.raises(ValueError):
            api.loudness_plan(48000, T)
    # nothing is written where a call refuses
    lib = api.load_library()
    buf = np.full(12, 7.5)
    assert lib.pdmp3_amd_loudness_coefficients(100, buf.ctypes.data) == -1 and (buf == 7.5).all()
    assert lib.pdmp3_amd_loudness_tables(100, None, None, buf.ctypes.data, None, None) == -1 and (buf == 7.5).all()
    q = C.c_int(-9)
    assert lib.pdmp3_amd_loudness_plan(48000, -1, None, None, None, C.byref(q), None, None, None) == -1 and q.value == -9
    assert lib.pdmp3_amd_loudness_plan(48000, 48000, None, None, None, C.byref(q), None, None, None) == 0 and q.value == 4800


# ---- 8. the sanitizer program ----
def test_the_sanitizer_program_of_the_planning_calls(tmp_path):
    """tools/sanitize/loudness_plan.c: pdmp3_amd/host/clip_loudness.c's check, coefficients, tables and plan under AddressSanitizer
    and UBSan, a stand-alone program on the CPU"""
    run_sanitizer_program(tmp_path, "loudness_plan", ("clip_loudness.c",))
