"""pYIN pitch tracking of clips on the host, no GPU: the refusals of the check one by one, the tables against
the numpy restatement of librosa's construction, and the kernels' own phases (pdmp3_amd/csrc/pyin_core.h, compiled here with g++
into tests/host_emul/pyin_emul.cpp and run thread by thread on wave_emul.h's fibers over a poisoned LDS) against the definition
(tests/clip_pyin_ref.py): the candidate stage with 0, 1, 64, 65 and hundreds of troughs in a frame, two troughs in one bin, a
trough at or above 1, a minimum above every threshold, silence; the path at every size named in the issue, with an L0 jump, with
a switch of voicing; a glide, then noise, then silence through the emulated k_clip_pitch in front."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import clip_pyin_cases as pc
import clip_pyin_ref as ref
import test_clip_pitch_host as tph
from clip_host import build_emul, run_sanitizer_program


class PyinParams(C.Structure):                     # include/pdmp3_hip.h pdmp3_pyin_params
    _fields_ = [("no_trough", C.c_double), ("l_stay", C.c_double), ("l_sw", C.c_double), ("l0", C.c_double), ("lp0_u", C.c_double),
                ("fill", C.c_float), ("use_bin", C.c_int32), ("tmin", C.c_int32), ("tmax", C.c_int32), ("n_thr", C.c_int32),
                ("n_bins", C.c_int32), ("hb", C.c_int32), ("max_troughs", C.c_int32), ("n_frames", C.c_int32), ("frames_wg", C.c_int32),
                ("channels", C.c_int32), ("out_mode", C.c_int32), ("path_threads", C.c_int32), ("obs_lds_bytes", C.c_uint32),
                ("path_lds_bytes", C.c_uint32), ("reserved", C.c_uint32)]


def _api():
    from pdmp3_amd import api
    return api


def _emul():
    lib = build_emul("pyin")
    lib.emul_pyin_obs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.emul_pyin_path.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.emul_pyin_table_bytes.argtypes = [C.c_void_p]
    assert lib.emul_pyin_params_bytes() == C.sizeof(PyinParams)
    return lib


def _kw(a):
    return {k: v for k, v in a.items() if k != "sample_rate"}


@functools.lru_cache(maxsize=None)
def _tables_cached(key):
    a = dict(key)
    return _api().pyin_tables(a["sample_rate"], **_kw(a))


def tables(a):
    return _tables_cached(tuple(sorted(a.items())))


def params_of(a, f, mode, fill=float("nan"), use_bin=0):
    api = _api()
    t, k = tables(a), ref.numbers(a)
    plan = api.pyin_plan(a["sample_rate"], n_frames=f, out_mode=mode, **_kw(a))
    assert (plan["n_bins"], plan["n_s"], plan["msf"], plan["band"], plan["hb"]) == (k["n_b"], k["n_s"], k["msf"], k["Wd"], k["hb"]), (plan, k)
    assert plan["states"] == 2 * k["n_b"] and plan["path_threads"] == min(1024, (k["n_b"] + 63) & ~63)
    assert plan["curve_bytes"] == 4 * f * (k["tmax"] + 1)
    assert (plan["obs_bytes"], plan["bp_bytes"]) == ((4 * f * (k["n_b"] + 1), 4 * f * k["n_b"]) if mode == 0 else (0, 0))
    p = PyinParams(a["no_trough_prob"], t["l_stay"], t["l_sw"], t["L0"], t["lp0_u"], fill, use_bin, k["tmin"], k["tmax"], t["n_thresholds"],
                   t["n_bins"], t["hb"], t["max_troughs"], f, plan["obs_frames"], 1, mode, plan["path_threads"], plan["obs_lds"], plan["path_lds"], 0)
    assert _emul().emul_pyin_table_bytes(C.byref(p)) <= t["block"].nbytes < _emul().emul_pyin_table_bytes(C.byref(p)) + 8
    return p


def emul_obs(curve, a):
    """curve: float32 [tmax + 1, F] -> mode 1's [n_b + 1, F]; mode 0's stage [F, n_b + 1] holds the same values"""
    curve = np.ascontiguousarray(curve, dtype=np.float32)
    f = curve.shape[1]
    t = tables(a)
    nb = t["n_bins"]
    outs = []
    for mode in (1, 0):
        p = params_of(a, f, mode)
        out = np.full((nb + 1) * f + 8, -5.0, dtype=np.float32)
        assert _emul().emul_pyin_obs(curve.ctypes.data, out.ctypes.data, t["block"].ctypes.data, C.byref(p)) == 0, "the emulated kernel read LDS it must not read"
        assert (out[(nb + 1) * f:] == -5.0).all() and not (out[:(nb + 1) * f] == -5.0).any()
        outs.append(out[:(nb + 1) * f].reshape((nb + 1, f) if mode == 1 else (f, nb + 1)).copy())
    assert np.array_equal(outs[0].view(np.uint32), outs[1].T.view(np.uint32))
    return outs[0]


def emul_path(obs, a, fill=float("nan"), use_bin=0):
    """obs: float32 [n_b + 1, F] -> the four planes [4, F]"""
    t = tables(a)
    nb, f = t["n_bins"], obs.shape[1]
    p = params_of(a, f, 0, fill, use_bin)
    stage = np.ascontiguousarray(obs.T, dtype=np.float32)
    bp = np.full(f * 2 * nb + 8, 0xeeee, dtype=np.uint16)
    out = np.full(4 * f + 8, -5.0, dtype=np.float32)
    assert _emul().emul_pyin_path(stage.ctypes.data, bp.ctypes.data, out.ctypes.data, t["block"].ctypes.data, C.byref(p)) == 0
    assert (out[4 * f:] == -5.0).all() and (bp[f * 2 * nb:] == 0xeeee).all()
    return out[:4 * f].reshape(4, f).copy()


WIDE = ref.args(sample_rate=16000, frame_length=2048, win_length=512, hop=256, fmin=10.5, fmax=21.0, resolution=0.5)      # lags 761 .. 1524, 25 bins


# ---- 1. the check ----
def test_the_checks_refusals_one_by_one():
    api = _api()
    ok = _kw(ref.args())
    assert api.pyin_check(22050, **ok) and api.pyin_check(22050) and api.pyin_check(16000, **_kw(WIDE))
    for bad in (dict(frame_length=2047), dict(frame_length=4096), dict(win_length=3), dict(hop=2049), dict(fmin=0.0), dict(fmax=65.406),
                dict(fmax=11025.1), dict(n_thresholds=0), dict(n_thresholds=257), dict(boltzmann=0.0), dict(boltzmann=-1.0),
                dict(boltzmann=float("nan")), dict(switch_prob=0.0), dict(switch_prob=1.0), dict(no_trough_prob=0.0), dict(no_trough_prob=1.0),
                dict(no_trough_prob=float("nan")), dict(resolution=0.04), dict(resolution=0.0), dict(resolution=-0.1), dict(fmin=20.0, fmax=11000.0, resolution=0.05),
                dict(fmax=65.5), dict(max_transition_rate=300.0), dict(max_transition_rate=-1.0), dict(beta=(2.5, 18)), dict(beta=(2, 65)),
                dict(beta=(0, 18)), dict(threshold_weights=[0.5] * 99), dict(threshold_weights=[-0.1] + [0.5] * 99),
                dict(threshold_weights=[float("inf")] + [0.5] * 99), dict(out_mode=2), dict(out_mode=-1), dict(out_mode="curve"),
                dict(n_frames=-1), dict(n_frames=2 ** 31 // 339 + 1), dict(resolution=1.0 / (3.0 + 1e-12)),
                dict(fmin=100.0, fmax=200.0 * (1 + 1e-13)), dict(max_transition_rate=10.5 * 22050 / (12 * 512) * (1 + 1e-13))):
        assert not api.pyin_check(22050, **dict(ok, **bad)), bad
    # n_s at its limits, a non-integer beta with weights of the caller's, quotients that are the boundary itself
    assert api.pyin_check(22050, **dict(ok, resolution=0.05)) and api.pyin_check(22050, **dict(ok, resolution=1.0))
    assert api.pyin_check(22050, **dict(ok, beta=(2.5, 18), threshold_weights=[0.01] * 100))
    assert api.pyin_plan(22050, **dict(ok, fmin=100.0, fmax=200.0))["n_bins"] == 121
    assert api.pyin_plan(16000, **dict(_kw(WIDE), max_transition_rate=62.5))["band"] == 25                   # Wd = n_b
    assert not api.pyin_check(16000, **dict(_kw(WIDE), max_transition_rate=62.5, hop=512))                    # Wd = 49 > n_b = 25
    assert api.pyin_plan(22050, **dict(ok, max_transition_rate=0.0))["band"] == 1
    # a tie of msf rounds to even, as Python's round does: 10.5 -> 10, 11.5 -> 12
    for want, msf in ((10, 10.5), (12, 11.5)):
        got = api.pyin_plan(16000, **dict(ok, hop=256, fmax=2000.0, max_transition_rate=msf * 16000 / (12 * 256)))
        assert msf * 16000 / (12 * 256) * 12 * 256 / 16000 == msf and got["msf"] == want, got


# ---- 2. the tables ----
@pytest.mark.parametrize("a", [ref.args(), WIDE, ref.args(hop=256, resolution=1.0), ref.args(hop=256, resolution=1.0, fmax=2000.0),
                               ref.args(sample_rate=16000, fmin=100.0, fmax=108.0, resolution=1.0, max_transition_rate=0.0)],
                         ids=["defaults", "wide-25-bins", "even-band-even-bins", "even-band-odd-bins", "two-bins"])
def test_tables_against_librosas_construction(a):
    t, k = tables(a), ref.numbers(a)
    nb = k["n_b"]
    assert (t["n_bins"], t["hb"], t["n_thresholds"]) == (nb, k["Wd"] // 2, 100) and t["max_troughs"] == (k["tmax"] - 1 - k["tmin"]) // 2 + 1
    want = np.log(ref.transition(nb, k["Wd"], a["switch_prob"]) + ref.TINY)
    got = ref.log_transition(t)
    pos = want > ref.L0 + 1.0
    assert np.abs(got - want)[pos].max() <= 1e-12 and (got[~pos] == ref.L0).all() and abs(t["L0"] - ref.L0) == 0.0
    assert np.array_equal(t["theta"], np.arange(1, 101) / 100.0)
    assert np.abs(t["w"] - ref.beta_weights(100, 2, 18)).max() <= 1e-16 and np.array_equal(t["wsum"], np.concatenate([[0.0], np.cumsum(t["w"])]))
    for n in (1, 2, 5, t["max_troughs"]):
        assert np.abs(t["G"][:n] * t["cN"][n] - ref.boltzmann_pmf(np.arange(n), 2.0, n)).max() <= 1e-15
    sr, ns = a["sample_rate"], k["n_s"]
    q = np.arange(1, nb + 1)
    assert np.abs(t["T"] / (sr / (a["fmin"] * 2.0 ** ((q - 0.5) / (12 * ns)))) - 1).max() <= 4 * ref.E and (np.diff(t["T"]) < 0).all()
    assert np.array_equal(t["f0"], (a["fmin"] * 2.0 ** (np.arange(nb) / (12 * ns))).astype(np.float32))
    assert t["lp0_u"] == -math.log(nb) and t["l_sw"] == math.log(a["switch_prob"]) and t["l_stay"] == math.log(1 - a["switch_prob"])


def test_tables_against_scipy():
    st = pytest.importorskip("scipy.stats")
    for beta in ((2, 18), (1, 1), (64, 64), (1, 18), (5, 3)):
        t = tables(ref.args(beta=beta))
        assert np.abs(t["w"] - np.diff(st.beta.cdf(np.arange(101) / 100.0, *beta))).max() <= 1e-14, beta
    t = tables(ref.args(boltzmann=0.7))
    for n in (1, 3, 40, t["max_troughs"]):
        assert np.abs(t["G"][:n] * t["cN"][n] - st.boltzmann.pmf(np.arange(n), 0.7, n)).max() <= 1e-14
    w = np.linspace(0.0, 1.0, 100) ** 2
    assert np.array_equal(tables(ref.args(beta=(2.5, 3.5), threshold_weights=tuple(w)))["w"], w)


# ---- 3. the candidate stage ----
def run_obs(curve, a):
    k, t = ref.numbers(a), tables(a)
    got = emul_obs(curve, a)
    worst, most = ref.check_observation(curve, got, t, k["tmin"], k["tmax"], a["no_trough_prob"])
    return got, worst, most


def _spaced(a, n, seed):
    """n troughs exactly two lags apart somewhere, the rest of the curve 1"""
    k = ref.numbers(a)
    rng = np.random.default_rng(seed)
    c = np.ones(k["tmax"] + 1, dtype=np.float32)
    first = k["tmin"] + int(rng.integers(0, k["tmax"] - k["tmin"] - 2 * n + 1))
    c[first:first + 2 * n:2] = (0.02 + 0.95 * rng.random(n)).astype(np.float32)
    return c


@pytest.mark.parametrize("f", [1, 7, 8, 9, 17])
def test_the_candidate_stage_by_the_number_of_troughs(f):
    a = WIDE
    counts = [0, 1, 64, 65, 129, 300, 381, 2, 63, 127, 128, 200, 33, 5, 250, 64, 65][:f]
    curve = np.stack([_spaced(a, n, 100 * f + i) for i, n in enumerate(counts)], axis=1)
    if f > 1:
        curve[ref.numbers(a)["tmin"], -1] = 0.5       # (a trough at tmin in the last frame: the one-sided test)
    got, worst, most = run_obs(curve, a)
    print("F %d: troughs up to %d a frame, worst error / bound %.3f" % (f, most, worst))
    assert most >= max(counts) and worst <= 1.0
    assert (got[:, 0] == 0).all()                       # no trough: O = 0 and v = 0


def test_the_candidate_stage_at_the_defaults_and_passes_of_64():
    a = ref.args()
    k = ref.numbers(a)
    assert (k["tmin"], k["tmax"], k["n_b"]) == (10, 338, 601)
    rng = np.random.default_rng(9)
    # curves as noise gives them: a random walk around 1 with a trough every few lags
    curve = (1.0 + 0.3 * rng.standard_normal((339, 9))).astype(np.float32).clip(0.01, 2.0)
    curve[:, 3] *= 0.3
    got, worst, most = run_obs(curve, a)
    print("defaults: troughs up to %d a frame, worst error / bound %.3f, v %s" % (most, worst, got[-1]))
    assert most > 64 and worst <= 1.0 and (got[-1] > 0).all()


@pytest.mark.parametrize("f", [3, 9])
@pytest.mark.parametrize("case", ["nb2048-obs4", "nb2048-nt256-obs2", "nb2048-tmax2000-obs2"])
def test_the_candidate_stage_at_four_and_two_frames_a_workgroup(case, f):
    """lags up to 1600 or 2000, or 256 thresholds: a workgroup's curves, rows and counts leave room for 4 or 2 frames only (asserted
    on the plan); F = 3 leaves the last workgroup's waves without a frame, F = 9 ends on a workgroup of one"""
    a, frames_wg = pc.MANY[case]
    k = ref.numbers(a)
    assert _api().pyin_plan(a["sample_rate"], n_frames=f, **_kw(a))["obs_frames"] == frames_wg and k["n_b"] == 2048
    rng = np.random.default_rng(k["tmax"] + f)
    curve = (1.0 + 0.3 * rng.standard_normal((k["tmax"] + 1, f))).astype(np.float32).clip(0.01, 2.0)
    curve[:, 1] *= 0.3
    got, worst, most = run_obs(curve, a)
    print("%s, F %d: troughs up to %d a frame, worst error / bound %.3f, entries at bins >= 1024: %d" % (case, f, most, worst, np.count_nonzero(got[1024:-1])))
    assert most > 300 and worst <= 1.0 and np.count_nonzero(got[1024:-1]) > f


def test_two_troughs_in_one_bin_the_larger_lag_stands():
    a = WIDE
    k, t = ref.numbers(a), tables(a)
    c = np.ones((k["tmax"] + 1, 2), dtype=np.float32)
    # lags 1010 and 1014 fall into one bin of a half-semitone grid; 1014's height is the larger, so its P is the smaller
    b = lambda tau: int((tau <= t["T"]).sum())
    assert b(1010) == b(1014) and b(1010) != b(1100)
    c[[1009, 1010, 1011], 0] = (0.5, 0.1, 0.5)
    c[[1013, 1014, 1015], 0] = (0.6, 0.3, 0.6)
    c[[1100], 1] = 0.2
    c[[1000], 1] = 0.4
    got, worst, _ = run_obs(c, a)
    o0, _, p64, n = ref.observe(c[:, 0], k["tmin"], k["tmax"], t, a["no_trough_prob"])
    assert n == 2 and np.count_nonzero(got[:-1, 0]) == 1 and got[b(1014), 0] == o0[b(1014)]
    alone = c[:, 0].copy()
    alone[[1009, 1010, 1011]] = 1.0
    lone = emul_obs(alone[:, None], a)[:, 0]
    assert 0 < got[b(1014), 0] < lone[b(1014)], "the entry is not the larger lag's own probability"
    assert np.count_nonzero(got[:-1, 1]) == 2


def test_a_trough_at_or_above_one_and_a_minimum_above_every_threshold():
    a = WIDE
    k, t = ref.numbers(a), tables(a)
    c = np.full((k["tmax"] + 1, 3), 3.0, dtype=np.float32)
    c[1000, 0] = 0.2
    c[1200, 0] = 1.0                                    # h = 1: under no threshold, and not the minimum: P = 0, dropped
    c[1200, 1] = 1.5                                    # the only trough, above every threshold: no_trough_prob (w_1 + .. + w_nt) alone
    c[1200, 2] = np.float32(0.995)                      # under the last threshold only
    got, worst, _ = run_obs(c, a)
    b = lambda tau: int((tau <= t["T"]).sum())
    assert np.count_nonzero(got[:-1, 0]) == 1 and got[b(1000), 0] > 0
    assert np.count_nonzero(got[:-1, 1]) == 1 and got[b(1200), 1] == np.float32(a["no_trough_prob"] * t["wsum"][-1]) == got[-1, 1]
    want = t["w"][-1] * (t["G"][0] * t["cN"][1]) + a["no_trough_prob"] * t["wsum"][99]
    assert got[b(1200), 2] == np.float32(want)


def test_silence_is_exactly_zero_and_unvoiced():
    for a in (WIDE, ref.args()):
        k, t = ref.numbers(a), tables(a)
        curve = np.ones((k["tmax"] + 1, 9), dtype=np.float32)
        got = emul_obs(curve, a)
        assert (got.view(np.uint32) == 0).all()
        planes = emul_path(got, a)
        assert np.isnan(planes[0]).all() and (planes[1] == 0).all() and (planes[2].view(np.uint32) == 0).all()
        assert ref.check_path(got, planes, t)[0] >= 0
        planes = emul_path(got, a, fill=-1.0)
        assert (planes[0] == -1.0).all()
        planes = emul_path(got, a, use_bin=1)
        assert np.array_equal(planes[0], t["f0"][planes[3].astype(int)])


# ---- 4. the path ----
TWO = ref.args(sample_rate=16000, fmin=100.0, fmax=108.0, resolution=1.0, max_transition_rate=0.0)                   # n_b 2, Wd 1
SIZES = {"nb2-wd1": TWO, "nb25-wd25": dict(WIDE, max_transition_rate=62.5), "nb25-wd15": WIDE, "nb601-wd101": ref.args(),
         "nb601-wd1": ref.args(max_transition_rate=0.0), "nb61-wd6": ref.args(hop=256, resolution=1.0),
         "nb60-wd6": ref.args(hop=256, resolution=1.0, fmax=2000.0),
         # one bin a thread at the thread limit, the first bin of a second turn, and two bins a thread: all of them more states than
         # a dynamic LDS request holds (k_clip_pyin_path_big on the device)
         "nb1024-wd141": pc.BINS_1024, "nb1025-wd141": pc.BINS_1025, "nb1201-wd201": pc.BINS_1201, "nb2048-wd101": pc.BINS_2048}


def random_obs(nb, f, rng, density=3):
    """observations as the candidate stage leaves them: a few entries a frame, some frames empty, v their clipped sum"""
    obs = np.zeros((nb + 1, f), dtype=np.float32)
    for i in range(f):
        n = int(rng.integers(0, density + 1))
        at = rng.choice(nb, size=min(n, nb), replace=False)
        obs[at, i] = (rng.random(at.size) ** 3 * (0.9 / max(n, 1))).astype(np.float32)
        s = 0.0
        for x in obs[:nb, i][obs[:nb, i] != 0]:
            s += float(x)
        obs[nb, i] = np.float32(min(1.0, s))
    return obs


@pytest.mark.parametrize("size", sorted(SIZES))
def test_the_path_at_every_size(size):
    a = SIZES[size]
    t, k = tables(a), ref.numbers(a)
    nb = k["n_b"]
    assert "nb%d-wd%d" % (nb, k["Wd"]) == size
    rng = np.random.default_rng(nb + k["Wd"])
    open_frames, frames = 0, 0
    for f in (1, 2, 7, 8, 9, 17):
        obs = random_obs(nb, f, rng)
        planes = emul_path(obs, a)
        und, s, best = ref.check_path(obs, planes, t)
        open_frames, frames = open_frames + und, frames + f
    print("%s: %d of %d frames without the margin" % (size, open_frames, frames))


def test_the_optimum_takes_an_l0_jump():
    a = ref.args()
    t = tables(a)
    nb, f = 601, 9
    obs = np.zeros((nb + 1, f), dtype=np.float32)
    obs[100, :4] = 1.0                                  # v = 1: the unvoiced states observe 0, and only bin 100 is left ...
    obs[400, 4:] = 1.0                                  # ... then only bin 400, 300 bins away: six bands
    obs[nb] = 1.0
    planes = emul_path(obs, a)
    und, s, best = ref.check_path(obs, planes, t)
    assert und == 0 and planes[3].tolist() == [100.0] * 4 + [400.0] * 5 and (planes[1] == 1).all()
    assert abs(s - (2 * ref.L0 + 7 * (t["ltri"][50] - t["lZ"][300] + t["l_stay"]))) < 1e-9      # lp0 of a voiced state, and the jump


def test_the_optimum_switches_voicing():
    a = ref.args()
    t = tables(a)
    nb, f = 601, 17
    obs = np.zeros((nb + 1, f), dtype=np.float32)
    obs[300, 5:11] = 0.9
    obs[302, 8] = 0.05
    obs[nb, 5:11] = 0.9
    obs[nb, 8] = np.float32(np.float64(np.float32(0.9)) + np.float64(np.float32(0.05)))
    planes = emul_path(obs, a)
    und, s, best = ref.check_path(obs, planes, t)
    assert planes[1].tolist() == [0.0] * 5 + [1.0] * 6 + [0.0] * 6 and (planes[3, 5:11] == 300).all()
    assert np.isnan(planes[0, :5]).all() and (planes[0, 5:11] == t["f0"][300]).all()


def test_the_optimum_switches_voicing_on_a_planted_curve():
    """test_the_optimum_switches_voicing from a curve, as the device test hands it to the kernels: no trough, six frames of one
    trough (a second one in the middle frame), no trough.  The definition alone first: the voicing of every frame and the bin of
    every voiced frame are decided; the unvoiced frames' bins are not (equal states), and are left to check_path's score rule"""
    a = ref.args()
    t = tables(a)
    nb, f = 601, 17
    curve, b = pc.voiced_stretch(a, t, f, 5, 11, 300)
    o64 = pc.observation(curve, a, t)
    assert np.count_nonzero(o64[:nb, 8]) == 2 and np.count_nonzero(o64[:nb]) == 7
    voiced, sure_v = pc.voicing(o64, t)
    want, sure = pc.decided(o64, t)
    assert voiced.tolist() == [False] * 5 + [True] * 6 + [False] * 6 and sure_v.all() and (want[5:11] == b).all() and sure[5:11].all()
    obs = emul_obs(curve, a)
    planes = emul_path(obs, a)
    ref.check_path(obs, planes, t)
    assert np.array_equal(planes[1] == 1, voiced) and (planes[3, 5:11] == b).all()
    assert np.isnan(planes[0, ~voiced]).all() and (planes[0, 5:11] == t["f0"][b]).all()


def test_a_planted_trough_in_the_1025th_bin():
    """1025 bins on 1024 threads: bin 1024 is thread 0's second and narrower than a lag (0.06 lags), so streams hardly ever put an
    entry there.  A trough whose parabola's vertex lies in its middle does: the observation's one entry is at bin 1024 with
    P = v = 1, and the path is voiced there in every frame, decided (the definition alone first)"""
    a = pc.BINS_1025
    t = tables(a)
    curve, b = pc.top_bin(a, t, 9)
    o64 = pc.observation(curve, a, t)
    want, sure = pc.decided(o64, t)
    assert b == 1024 and (np.flatnonzero(o64[:-1, 0]) == [b]).all() and (want == b).all() and sure.all()
    obs, worst, most = run_obs(curve, a)
    planes = emul_path(obs, a)
    und, s, best = ref.check_path(obs, planes, t)
    assert und == 0 and (planes[3] == b).all() and (planes[1] == 1).all() and (obs[b] == 1.0).all() and np.count_nonzero(obs[:-1]) == 9


def test_a_planted_glide_through_the_second_bin_of_a_thread():
    """2048 bins on 1024 threads: noise never steers the path above bin 800 or so (its lowest trough sits at long lags), so the
    second turn of the step's loop decides nothing there.  One shallow trough a frame whose lag falls from 120 to 42 does: the
    bin rises through 1024 by no more than hb a frame.  First the definition alone on its own observation: voiced at the planted
    bin in every frame but the first (a voiced state starts at L0), decided; then the emulated kernels."""
    a = pc.BINS_2048
    t, k = tables(a), ref.numbers(a)
    f = 17
    curve, bins = pc.glide(a, t, f, 900, 23)
    assert (np.abs(np.diff(bins)) <= k["hb"]).all() and (bins >= 1024).sum() >= 5 and (bins < 1024).sum() >= 5
    want, sure = pc.decided(pc.observation(curve, a, t), t)
    assert np.array_equal(want[1:], bins[1:]) and sure.all(), "the reference's own decode does not follow the planted bins"
    obs = emul_obs(curve, a)
    planes = emul_path(obs, a)
    und, s, best = ref.check_path(obs, planes, t)
    print("planted glide: bins %s, v %s" % (planes[3].astype(int).tolist(), planes[2, :2]))
    assert und == 0 and np.array_equal(planes[3, 1:], bins[1:]) and (planes[1, 1:] == 1).all() and planes[1, 0] == 0
    assert (planes[3] >= 1024).sum() >= 5


def test_the_optimum_takes_an_l0_jump_between_two_upper_bins():
    """test_the_optimum_takes_an_l0_jump at 2048 bins, from a curve: a trough under every threshold has P = 1 and v = 1, so only
    its bin is left; both bins are a thread's second, 500 bins (ten bands) apart"""
    a = pc.BINS_2048
    t = tables(a)
    nb, f, hb = 2048, 9, 50
    curve, bins = pc.jump(a, t, f, 4, 1200, 1700)
    assert bins[0] >= 1024 and bins[-1] - bins[0] > 8 * hb and bins[-1] < nb - hb
    want, sure = pc.decided(pc.observation(curve, a, t), t)
    assert np.array_equal(want, bins) and sure.all(), "the reference's own decode does not take the jump"
    obs = emul_obs(curve, a)
    assert (obs[nb] == 1.0).all() and np.count_nonzero(obs[:nb]) == f
    planes = emul_path(obs, a)
    und, s, best = ref.check_path(obs, planes, t)
    assert und == 0 and np.array_equal(planes[3], bins) and (planes[1] == 1).all()
    assert abs(s - (2 * ref.L0 + 7 * (t["ltri"][hb] - t["lZ"][bins[0]] + t["l_stay"]))) < 1e-9 and t["lZ"][bins[0]] == t["lZ"][bins[-1]]


# ---- 5. the whole chain on the emulated kernels ----
STEADY = ref.args(sample_rate=16000, frame_length=256, win_length=128, hop=64, fmin=16000 / 137.5, fmax=16000 / 2.5)     # lags 2 .. 127


def steady_tone(n, period=50.3):
    """a sine whose period's multiples lie away from the half lags, where a trough's two neighbours would tie"""
    return (0.5 * np.sin(2.0 * np.pi * np.arange(n) / period)).astype(np.float32)


def test_a_steady_tone_against_the_binary64_chain():
    """N 256, W 128: the chain of 128 additions keeps section 20's intervals narrow, and the reference alone decides every frame
    of this tone (asserted); the decided frames' troughs are then the binary64 curve's, and check_observation holds the rest"""
    a = STEADY
    k, t = ref.numbers(a), tables(a)
    assert (k["tmin"], k["tmax"], k["n_b"], k["Wd"]) == (2, 127, 694, 21)
    g = dict(sample_rate=16000, frame_length=256, win_length=128, hop=64, fmin=a["fmin"], fmax=a["fmax"], threshold=0.1)
    f = 17
    y = steady_tone(40 * 64)
    row, lead = tph.row_of(y, 500, 256, 64, f)
    _, curve = tph.emulate(row, lead, g, f)
    obs, worst, most = run_obs(curve, a)
    und = ref.undecided_frames(row, lead, a, f, curve, t)
    print("steady tone: %d of %d frames undecided against the binary64 chain, worst error / bound %.3f" % (und.sum(), f, worst))
    assert und.sum() <= ref.CAP * f
    planes = emul_path(obs, a)
    open_frames, s, best = ref.check_path(obs, planes, t)
    want = int(round(120 * math.log2(16000 / 50.3 / a["fmin"])))
    print("  the path: %d of %d frames without the margin, bins %s (the tone's: %d)" % (open_frames, f, sorted(set(planes[3].astype(int))), want))
    assert (planes[1] == 1).all() and (np.abs(planes[3] - want) <= 1).all()


def test_a_glide_then_noise_then_silence():
    sr = 22050
    a = ref.args()
    k, t = ref.numbers(a), tables(a)
    g = dict(sample_rate=sr, frame_length=2048, win_length=None, hop=512, fmin=65.406, fmax=2093.0, threshold=0.1)
    y = tph.glide()[sr:]                                # the glide from 110 to 440 Hz ...
    rng = np.random.default_rng(4)
    y = np.concatenate([y, (0.1 * rng.standard_normal(12 * 512)).astype(np.float32), np.zeros(12 * 512, dtype=np.float32)])
    f = y.size // 512 - 2
    row, lead = tph.row_of(y, 1024, 2048, 512, f)
    _, curve = tph.emulate(row, lead, g, f)
    obs, worst, most = run_obs(curve, a)
    und = ref.undecided_frames(row, lead, a, f, curve, t)
    glide_frames = (y.size - 24 * 512) // 512 - 2
    print("glide, noise, silence: %d frames, troughs up to %d, worst error / bound %.3f; undecided against the binary64 chain: %d of %d "
          "glide frames, %d of the rest" % (f, most, worst, und[:glide_frames].sum(), glide_frames, und[glide_frames:].sum()))
    # (not capped here: the glide's curve has shallow troughs between its harmonics' lags, which section 20's intervals -- the
    # worst case of a chain of 1024 binary32 additions -- cannot decide; test_a_steady_tone_against_the_binary64_chain holds the cap)
    planes = emul_path(obs, a)
    open_frames, s, best = ref.check_path(obs, planes, t)
    print("  the path: %d of %d frames without the margin; S %.6f, max S %.6f" % (open_frames, f, s, best))
    voiced = planes[1] == 1
    assert voiced[2:glide_frames - 2].all() and not voiced[glide_frames + 3:].any()
    assert (planes[2, -8:] == 0).all()
    # bins within one of the glide's: frame i reads the samples [512 i, 512 i + 2048), over which the glide's frequency rises
    # from f_lo to f_hi; whatever period the frame shows lies between theirs, so the bin lies within one of that range of bins
    t_lo, t_hi = 512 * np.arange(f) / sr, (512 * np.arange(f) + 2048) / sr
    bin_of = lambda tt: 12 * k["n_s"] * np.log2(110.0 * 4.0 ** np.clip(tt / 1.1, 0.0, 1.0) / a["fmin"])
    inner = slice(2, glide_frames - 2)
    b = planes[3, inner]
    assert (b >= np.floor(bin_of(t_lo))[inner] - 1).all() and (b <= np.ceil(bin_of(t_hi))[inner] + 1).all(), (b, bin_of(t_lo)[inner], bin_of(t_hi)[inner])


# ---- 6. the sanitizer program ----
def test_the_sanitizer_program_of_the_planning_calls(tmp_path):
    """tools/sanitize/pyin_plan.c: pdmp3_amd/host/clip_pyin.c's check, tables and plan over the refusals and the edge cases under
    AddressSanitizer and UBSan, a stand-alone program on the CPU"""
    run_sanitizer_program(tmp_path, "pyin_plan", ("clip_pyin.c", "clip_pitch.c"))
