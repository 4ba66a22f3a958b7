"""pdmp3_hip_clip_pyin and pdmp3_hip_clip_beat called through the engine's C-ABI (include/pdmp3_hip.h) with torch device tensors as
memory: the kernels take device addresses of the curve, the stages, the envelope and the tables, so a test can hand them the same
planted inputs the emulated kernels get (tests/test_clip_pyin_host.py, tests/test_clip_beat_host.py).  The parameters are the
plans' (api.pyin_plan / pyin_tables, api.beat_plan / beat_tables), as pdmp3_amd/host/clip_features.c fills them.  Every buffer a
kernel writes is filled with a sentinel first and has guard elements behind it, which are looked at.  A helper module: no test, no
fixture."""
import contextlib
import ctypes as C

import numpy as np

import clip_beat_ref as bref
import clip_pyin_ref as yref
from clip_host import build_emul

SENT = np.float32(-1234.5)
GUARD = 24


class PyinDesc(C.Structure):                       # include/pdmp3_hip.h pdmp3_pyin_desc
    _fields_ = [("curve", C.c_uint64), ("obs", C.c_uint64), ("bp", C.c_uint64), ("dst", C.c_uint64), ("dst_chan_stride", C.c_uint64)]


class PyinParams(C.Structure):                     # include/pdmp3_hip.h pdmp3_pyin_params
    _fields_ = [("no_trough", C.c_double), ("l_stay", C.c_double), ("l_sw", C.c_double), ("l0", C.c_double), ("lp0_u", C.c_double),
                ("fill", C.c_float), ("use_bin", C.c_int32), ("tmin", C.c_int32), ("tmax", C.c_int32), ("n_thr", C.c_int32),
                ("n_bins", C.c_int32), ("hb", C.c_int32), ("max_troughs", C.c_int32), ("n_frames", C.c_int32), ("frames_wg", C.c_int32),
                ("channels", C.c_int32), ("out_mode", C.c_int32), ("path_threads", C.c_int32), ("obs_lds_bytes", C.c_uint32),
                ("path_lds_bytes", C.c_uint32), ("reserved", C.c_uint32)]


class BeatDesc(C.Structure):                       # include/pdmp3_hip.h pdmp3_beat_desc
    _fields_ = [("env", C.c_uint64), ("stats", C.c_uint64), ("dst", C.c_uint64), ("dst_chan_stride", C.c_uint64), ("n", C.c_uint32),
                ("reserved", C.c_uint32)]


class BeatParams(C.Structure):                     # include/pdmp3_hip.h pdmp3_beat_params
    _fields_ = [("tightness", C.c_double), ("bpm", C.c_float), ("period", C.c_int32), ("p_min", C.c_int32), ("p_max", C.c_int32),
                ("n_frames", C.c_int32), ("channels", C.c_int32), ("trim", C.c_int32), ("out_mode", C.c_int32), ("env_stride", C.c_uint32),
                ("work_stride", C.c_uint32), ("score_lds_bytes", C.c_uint32), ("dp_lds_bytes", C.c_uint32)]


def check_sizes():
    """the mirrors above against the structs the kernels' own source is compiled with"""
    assert build_emul("pyin").emul_pyin_params_bytes() == C.sizeof(PyinParams) and C.sizeof(PyinDesc) == 40
    assert build_emul("beat").emul_beat_params_bytes() == C.sizeof(BeatParams) and C.sizeof(BeatDesc) == 40


@contextlib.contextmanager
def stream(engine, max_frames=64):
    """(the engine's library, a stream of two slots on the engine's context); destroyed on leaving"""
    from pdmp3_amd import hip
    lib = hip.load_library()
    vp = C.c_void_p
    lib.pdmp3_hip_stream_create_slots.argtypes = [vp, C.c_int, C.c_int, C.POINTER(vp)]
    lib.pdmp3_hip_stream_destroy.argtypes = [vp]
    lib.pdmp3_hip_clip_pyin.argtypes = [vp, C.c_int, vp, C.c_int, vp, vp]
    lib.pdmp3_hip_clip_beat.argtypes = [vp, C.c_int, vp, C.c_int, vp, vp, vp]
    hs = vp()
    assert lib.pdmp3_hip_stream_create_slots(engine.h, max_frames, 2, C.byref(hs)) == 0
    try:
        yield lib, hs
    finally:
        lib.pdmp3_hip_stream_destroy(hs)


def _device(a):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return d


def _host(d):
    import torch
    torch.cuda.synchronize()
    return d.cpu().numpy()


def pyin_params(a, t, f, mode, fill=float("nan"), use_bin=0):
    """pdmp3_pyin_params of the arguments a (clip_pyin_ref.args) and their tables t (api.pyin_tables) for F frames, one channel"""
    from pdmp3_amd import api
    k = yref.numbers(a)
    plan = api.pyin_plan(a["sample_rate"], n_frames=f, out_mode=mode, **{x: v for x, v in a.items() if x != "sample_rate"})
    assert (plan["n_bins"], plan["hb"]) == (k["n_b"], k["hb"]) == (t["n_bins"], t["hb"])
    return PyinParams(a["no_trough_prob"], t["l_stay"], t["l_sw"], t["L0"], t["lp0_u"], fill, use_bin, k["tmin"], k["tmax"], t["n_thresholds"],
                      t["n_bins"], t["hb"], t["max_troughs"], f, plan["obs_frames"], 1, mode, plan["path_threads"], plan["obs_lds"], plan["path_lds"], 0), plan


def pyin_path(lib, hs, curve, a, t):
    """one clip, one channel, mode 0 on a curve float32 [tmax + 1, F] of the caller's: k_clip_pyin_obs into the stage, then
    k_clip_pyin_path -> (the stage as mode 1 lays it out [n_b + 1, F], the four planes [4, F], the plan); nothing is written
    behind the stage's [F][n_b + 1], the back-pointers' [F][2 n_b] or the planes' [4][F], and every element of them is written"""
    curve = np.ascontiguousarray(curve, dtype=np.float32)
    nb, f = t["n_bins"], curve.shape[1]
    p, plan = pyin_params(a, t, f, 0)
    assert curve.shape[0] == p.tmax + 1
    d_curve = _device(curve)
    d_obs = _device(np.full(f * (nb + 1) + GUARD, SENT, dtype=np.float32))
    d_bp = _device(np.full(f * 2 * nb + GUARD, -4370, dtype=np.int16))          # 0xeeee
    d_out = _device(np.full(4 * f + GUARD, SENT, dtype=np.float32))
    desc = PyinDesc(d_curve.data_ptr(), d_obs.data_ptr(), d_bp.data_ptr(), d_out.data_ptr(), 4 * f)
    block = np.ascontiguousarray(t["block"])
    assert lib.pdmp3_hip_clip_pyin(hs, 0, C.byref(desc), 1, block.ctypes.data, C.byref(p)) == 0
    obs, bp, out = _host(d_obs), _host(d_bp), _host(d_out)
    assert (obs[f * (nb + 1):] == SENT).all() and (bp[f * 2 * nb:] == -4370).all() and (out[4 * f:] == SENT).all(), "written behind a stage or the planes"
    assert not (obs[:f * (nb + 1)] == SENT).any() and not (out[:4 * f] == SENT).any()
    return obs[:f * (nb + 1)].reshape(f, nb + 1).T.copy(), out[:4 * f].reshape(4, f).copy(), plan


def beat_params(period, f, mode, trim, tightness=100.0, sample_rate=22050, hop=512):
    """pdmp3_beat_params of a given period for F frames, one channel -> (params, plan)"""
    from pdmp3_amd import api
    bpm = 60.0 * sample_rate / (hop * period)
    plan = api.beat_plan(sample_rate, n_frames=f, bpm=bpm, hop=hop, tightness=tightness)
    assert plan["period"] == period == bref.period_of(bpm, sample_rate, hop) and plan["work_bytes"] % 8 == 0
    return BeatParams(tightness, bpm, period, period, period, f, 1, 1 if trim else 0, mode, f, plan["work_bytes"] // 8, plan["score_lds"],
                      plan["dp_lds"]), plan


def beat_track(lib, hs, env, f, period, g, tx, mode, trim=True):
    """one clip, one channel on an envelope float32 [n <= F] and tables g [P + 1], tx [2 P + 1] of the caller's, out_mode 0 .. 2 ->
    (the row [F] or rows [2, F], stats [8], the plan); nothing is written behind the rows, the stats or the clip's scratch"""
    env = np.ascontiguousarray(env, dtype=np.float32)
    n, rows = env.size, 1 if mode == 0 else 2
    assert 2 <= n <= f and g.shape == (period + 1,) and tx.shape == (2 * period + 1,)
    p, plan = beat_params(period, f, mode, trim)
    d_env = _device(np.concatenate([env, np.full(f - n + GUARD, SENT, dtype=np.float32)]))
    d_out = _device(np.full(rows * f + GUARD, SENT, dtype=np.float32))
    d_stats = _device(np.full(8 + GUARD, SENT, dtype=np.float32))
    d_work = _device(np.full(p.work_stride + GUARD, -7.25))
    desc = BeatDesc(d_env.data_ptr(), d_stats.data_ptr(), d_out.data_ptr(), rows * f, n, 0)
    block = np.ascontiguousarray(np.concatenate([g, tx]), dtype=np.float64)
    assert lib.pdmp3_hip_clip_beat(hs, 0, C.byref(desc), 1, block.ctypes.data, d_work.data_ptr(), C.byref(p)) == 0
    out, stats, work = _host(d_out), _host(d_stats), _host(d_work)
    assert (out[rows * f:] == SENT).all() and (stats[8:] == SENT).all() and (work[p.work_stride:] == -7.25).all(), "written behind the rows, the stats or the scratch"
    assert not (out[:rows * f] == SENT).any() and not (stats[:8] == SENT).any()
    return (out[:f].copy() if mode == 0 else out[:2 * f].reshape(2, f).copy()), stats[:8].copy(), plan


def beat_track_many(lib, hs, envs, which, f, period, g, tx, mode=2, trim=True):
    """len(which) clips of one channel in one call, clip i on the envelope envs[which[i]] (float32 [E, F], every frame of which
    enters) -> (rows [K, 2, F] (mode 0: [K, F]), stats [K, 8], the scratch [K, work_stride] as doubles, params, plan).  More than
    32 768 clips make the engine launch twice, the second time with `first` = 32 768: clip i's scratch must lie at row i
    whichever launch runs it.  Nothing is written behind the last row of the rows, the stats or the scratch"""
    envs = np.ascontiguousarray(envs, dtype=np.float32)
    k, rows = len(which), 1 if mode == 0 else 2
    assert envs.ndim == 2 and envs.shape[1] == f and g.shape == (period + 1,) and tx.shape == (2 * period + 1,)
    p, plan = beat_params(period, f, mode, trim)
    d_env = _device(np.concatenate([envs.reshape(-1), np.full(GUARD, SENT, dtype=np.float32)]))
    d_out = _device(np.full(k * rows * f + GUARD, SENT, dtype=np.float32))
    d_stats = _device(np.full(k * 8 + GUARD, SENT, dtype=np.float32))
    d_work = _device(np.full(k * p.work_stride + GUARD, -7.25))
    descs = (BeatDesc * k)()
    for i, e in enumerate(which):
        descs[i] = BeatDesc(d_env.data_ptr() + 4 * f * int(e), d_stats.data_ptr() + 32 * i, d_out.data_ptr() + 4 * rows * f * i, rows * f, f, 0)
    block = np.ascontiguousarray(np.concatenate([g, tx]), dtype=np.float64)
    assert lib.pdmp3_hip_clip_beat(hs, 0, descs, k, block.ctypes.data, d_work.data_ptr(), C.byref(p)) == 0
    out, stats, work = _host(d_out), _host(d_stats), _host(d_work)
    assert (out[k * rows * f:] == SENT).all() and (stats[k * 8:] == SENT).all() and (work[k * p.work_stride:] == -7.25).all(), "written behind the rows, the stats or the scratch"
    shape = (k, f) if mode == 0 else (k, 2, f)
    return out[:k * rows * f].reshape(shape).copy(), stats[:k * 8].reshape(k, 8).copy(), work[:k * p.work_stride].reshape(k, p.work_stride), p, plan
