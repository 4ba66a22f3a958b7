"""The loudness of clips (include/pdmp3_bulk.h pdmp3_amd_bulk_decode_clips_loudness) in binary64 with
numpy: the definition as a plain sample loop, the error bound of the device's blocked binary32 product evaluated from the
reference's own quantities, the rule for clips whose gates are undecided, and a restatement of pdmp3_amd_loudness_tables and
pdmp3_amd_loudness_plan.  Shared by tests/test_clip_loudness_host.py and tests/test_gpu_clip_loudness.py."""
import math

import numpy as np

B = 64                     # samples of a block
CHUNK = 64                 # blocks of a scan chunk
WAVE = 1024                # samples whose squares one wave of k_loud_blocks adds
LDS_BYTES = 64 * 68 * 4
U = 2.0 ** -24             # unit roundoff of binary32
K_EXTENT = B + 8           # terms of an output sample's chain: 64 columns of Hm, the state as high and low parts


def coefficients(fs):
    """-> [2, 2, 3]: [H1 / H2][b / a][3], libebur128's parametrisation"""
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / fs)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    b1 = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0]
    a1 = [1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    return np.array([[b1, a1], [[1.0, -2.0, 1.0], [1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]]])


def kweight(x, fs, state=None, states_every=0):
    """y = H2(H1(x)) along the last axis by a plain sample loop (transposed direct form II), every leading index a row of its
    own, from rest or from state [..., 4] = (z1, z2 of H1, z1, z2 of H2).  -> y, or (y, the states in front of samples 0,
    states_every, 2 states_every, ... [..., n, 4]) when states_every"""
    (b1, a1), (b2, a2) = coefficients(fs)
    x = np.asarray(x, dtype=np.float64)
    lead = x.shape[:-1]
    s = np.zeros(lead + (4,)) if state is None else np.array(state, dtype=np.float64).reshape(lead + (4,))
    s0, s1, s2, s3 = (s[..., i].copy() for i in range(4))
    y = np.empty_like(x)
    kept = []
    for t in range(x.shape[-1]):
        if states_every and t % states_every == 0:
            kept.append(np.stack([s0, s1, s2, s3], axis=-1))
        xt = x[..., t]
        v = b1[0] * xt + s0
        s0 = b1[1] * xt - a1[1] * v + s1
        s1 = b1[2] * xt - a1[2] * v
        yt = b2[0] * v + s2
        s2 = b2[1] * v - a2[1] * yt + s3
        s3 = b2[2] * v - a2[2] * yt
        y[..., t] = yt
    if states_every:
        return y, (np.stack(kept, axis=-2) if kept else np.zeros(lead + (0, 4)))
    return y


_TABLES = {}


def tables(fs):
    """pdmp3_amd_loudness_tables restated, all in binary64: Hm [64, 64], O [64, 4], Phi [4, 4], R [4, 64] with
    y_block = Hm u + O s_in, s_out = Phi s_in + R u"""
    if fs not in _TABLES:
        imp = np.zeros(B)
        imp[0] = 1.0
        h = kweight(imp, fs)
        Hm = np.zeros((B, B))
        for i in range(B):
            Hm[i, :i + 1] = h[i::-1]
        O, st = kweight(np.zeros((4, B + 1)), fs, state=np.eye(4), states_every=B)      # row m: from unit state m
        Phi = st[:, 1, :].T                                                              # column m: the state 64 samples on
        _, st = kweight(np.concatenate([np.eye(B), np.zeros((B, 1))], axis=1), fs, states_every=B)
        R = st[:, 1, :].T
        _TABLES[fs] = (Hm, O[:, :B].T.copy(), Phi, R)
    return _TABLES[fs]


def powers(fs, n=CHUNK + 1):
    """Phi^k, k = 0 .. n, as the recurrence itself gives them: the states 64 k samples behind each unit state, no input"""
    _, st = kweight(np.zeros((4, n * B + 1)), fs, state=np.eye(4), states_every=B)
    return np.transpose(st, (1, 2, 0))                 # [k][row r][column m]


def plan(fs, n_samples):
    q = (fs + 5) // 10
    I = n_samples // q
    return dict(B=B, chunk=CHUNK, lds_bytes=LDS_BYTES, q=q, n_chunks=(n_samples + B * CHUNK - 1) // (B * CHUNK), I=I, J=max(0, I - 3))


def _l(z):
    z = np.asarray(z, dtype=np.float64)
    with np.errstate(divide="ignore"):
        return np.where(z > 0, -0.691 + 10.0 * np.log10(np.where(z > 0, z, 1.0)), -np.inf)


def _dl(z, e):
    """how far the loudness of z may move when z moves by e: 10 log10(z / (z - e)), inf where e >= z"""
    z, e = np.asarray(z, dtype=np.float64), np.asarray(e, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(e < z, 10.0 * np.log10(np.where(e < z, z / np.where(e < z, z - e, 1.0), 1.0)), np.inf)


class Measured:
    pass


def measure(x, fs, dual_mono=False, target=None, peak_limit=0.0):
    """x [C, T]: binary32 values -> the definition's numbers in binary64 and the bounds of the device's.

    Bound.  An output sample is one chain of K_EXTENT fused multiply-adds over binary32 operands: with u = 2^-24,
    |y^ - y| <= e_t = ((K_EXTENT u) / (1 - K_EXTENT u) + 2 u) A_t + 2^-28 max(1, (fs / 48000)^2) max|x|,
    A_t = sum_j |h_(i-j)| |u_j| + sum_m |O_im| |s_m|; the 2 u are the roundings of Hm and O, the last term the binary64 chain of
    the states through |O| (it does not grow with T: the powers of Phi decay; DESIGN.md section 18 has the estimate).  A sub-block sum: sum (2 |y| e + e^2), plus D u / (1 - D u) sum (|y| + e)^2 for the square and the
    D - 1 additions a term passes: 16 in a lane, 6 in the wave, q / 1024 + 2 across the waves."""
    x = np.asarray(x)
    assert x.ndim == 2 and x.shape[0] in (1, 2)
    C, T = x.shape
    x64 = x.astype(np.float64)
    m = Measured()
    p = plan(fs, T)
    q, I, J = p["q"], p["I"], p["J"]
    m.q, m.I, m.J = q, I, J
    y, st = kweight(x64, fs, states_every=B) if T else (np.zeros((C, 0)), np.zeros((C, 0, 4)))
    m.y = y
    Hm, O, _, _ = tables(fs)
    nb = (T + B - 1) // B
    ux = np.zeros((C, nb * B))
    ux[:, :T] = np.abs(x64)
    A = (ux.reshape(C, nb, B) @ np.abs(Hm).T + np.abs(st) @ np.abs(O).T).reshape(C, nb * B)[:, :T]
    peak = float(np.abs(x64).max()) if T else 0.0
    e = (K_EXTENT * U / (1.0 - K_EXTENT * U) + 2.0 * U) * A + 2.0 ** -28 * max(1.0, (fs / 48000.0) ** 2) * peak
    D = 16 + 6 + q // WAVE + 2 + 1
    s = (y[:, :I * q] ** 2).reshape(C, I, q).sum(axis=2)
    es = ((2.0 * np.abs(y) * e + e * e)[:, :I * q]).reshape(C, I, q).sum(axis=2) + \
        D * U / (1.0 - D * U) * (((np.abs(y) + e) ** 2)[:, :I * q]).reshape(C, I, q).sum(axis=2)
    G = np.ones(C)
    if dual_mono:
        assert C == 1
        G[0] = 2.0
    z = np.array([(G[:, None] * s[:, j:j + 4]).sum() for j in range(J)]) / (4.0 * q)
    ez = np.array([(G[:, None] * es[:, j:j + 4]).sum() for j in range(J)]) / (4.0 * q)
    m.s, m.es, m.z, m.ez = s, es, z, ez
    m.l, m.dl = _l(z), _dl(z, ez)
    inA = m.l > -70.0
    m.nA = int(inA.sum())
    m.P = peak
    margins = [np.inf]
    undecided = False
    lo, hi = _l(np.maximum(z - ez, 0.0)), _l(z + ez)          # where the device's l_j may lie
    if J:
        undecided |= bool(((lo <= -70.0) & (hi > -70.0)).any())
        margins.append(float(np.minimum(np.abs(lo + 70.0), np.abs(hi + 70.0)).min()))
    if m.nA:
        m.gamma = float(_l(z[inA].mean()) - 10.0)
        m.dgamma = float(_dl(z[inA].mean(), ez[inA].mean()))
        inG = inA & (m.l > m.gamma)
        undecided |= bool(((lo[inA] <= m.gamma + m.dgamma) & (hi[inA] >= m.gamma - m.dgamma)).any())
        margins.append(float(np.minimum(np.abs(lo[inA] - m.gamma), np.abs(hi[inA] - m.gamma)).min() - m.dgamma))
        m.nGt = int(inG.sum())
        m.L = float(_l(z[inG].mean()))
        m.dL = float(_dl(z[inG].mean(), ez[inG].mean()))
    else:
        m.gamma, m.dgamma, m.nGt, m.L, m.dL = -np.inf, 0.0, 0, -np.inf, 0.0
    m.M = float(m.l.max()) if J else -np.inf
    if J and np.isfinite(m.M):
        jm = int(np.argmax(m.l))
        near = m.l + m.dl >= m.M - m.dl[jm]
        m.dM = float(m.dl[near].max())
    else:
        m.dM = 0.0
    # the gain
    m.limited = False
    if target is None or not np.isfinite(m.L):
        m.g, m.dg = 1.0, 0.0
    else:
        g = 10.0 ** ((target - m.L) / 20.0)
        dg = g * (10.0 ** (m.dL / 20.0) - 1.0) + 2.0 * U * g
        if peak_limit > 0.0:
            if abs(g * peak - peak_limit) <= dg * peak:
                undecided = True
            margins.append(abs(20.0 * math.log10(g * peak / peak_limit)) - m.dL if peak > 0 else np.inf)
            if g * peak > peak_limit:
                m.limited = True
                g = float(np.float32(peak_limit / peak))
                dg = 0.0
        m.g, m.dg = g, dg
    m.undecided = bool(undecided)
    m.margin = float(min(margins))
    return m


def check_stats(m, stats, momentary=None):
    """the device's stats row (and momentary row) against the reference m -> the worst error / bound met (0 where every bound is
    0 and every value exact); AssertionError on a miss.  An undecided clip: M, P, J and the momentary curve alone."""
    stats = np.asarray(stats, dtype=np.float64)
    worst = 0.0

    def near(got, want, bound, what):
        nonlocal worst
        if not np.isfinite(want):
            assert got == want, (what, got, want)
            return
        b = bound + abs(want) * 2.0 ** -23            # (the value's own rounding to binary32)
        assert abs(got - want) <= b, (what, got, want, b)
        worst = max(worst, abs(got - want) / b)

    assert stats[5] == m.J, ("J", stats[5], m.J)
    assert np.float32(stats[2]) == np.float32(m.P), ("P", stats[2], m.P)
    near(stats[1], m.M, m.dM, "M")
    if momentary is not None:
        mom = np.asarray(momentary, dtype=np.float64)
        assert mom.shape == (m.J,)
        for j in range(m.J):
            if m.ez[j] < 0.5 * m.z[j]:
                near(mom[j], m.l[j], m.dl[j], "l[%d]" % j)
            else:                                      # (next to silence: no more than the bound allows)
                assert mom[j] <= float(_l(m.z[j] + m.ez[j])) + 1e-5, ("l[%d]" % j, mom[j], m.z[j], m.ez[j])
    if m.undecided:
        return worst
    assert stats[6] == m.nA and stats[7] == m.nGt, ("counts", stats[6:8], m.nA, m.nGt)
    near(stats[0], m.L, m.dL, "L")
    near(stats[4], m.gamma, m.dgamma, "Gamma")
    if m.limited or m.dg == 0.0:
        assert np.float32(stats[3]) == np.float32(m.g), ("g", stats[3], m.g)
    else:
        near(stats[3], m.g, m.dg, "g")
    return worst


def curve_gates(row, every=1, relative=-10.0):
    """The two gates on a curve as a call stores it: row holds binary32 values l'_j = fl32(l_j) in dB (-inf: silence) of which
    every `every`-th takes part; the absolute gate is -70, the relative one `relative` dB under the level of the mean of what
    passes the absolute one.  All in binary64 -> a Measured with n_abs, gamma / dgamma, n_rel, level / dlevel (the level of the
    mean of what passes both), inside (the mask of those, over row[::every]), dv (the bound of each of row[::every]),
    undecided and margin_bounds.

    Bounds, from the row's own rounding alone.  The call gates and sums its binary64 l_j and z_j and stores fl32(l_j), so
    |l'_j - l_j| <= d_j = 2^-24 |l'_j| / (1 - 2^-24) (round to nearest, |l_j| <= |l'_j| / (1 - 2^-24)).  The power behind a
    value is z = 10^((l + 0.691) / 10), so dz / z = (ln 10 / 10) dl to first order and, without dropping a term,
    |z'_j / z_j - 1| <= r_j = exp((ln 10 / 10) d_j) - 1.  A mean of positive z_j over a fixed set moves by no more than the
    largest r_j of the set, relatively, so its level moves by no more than 10 log10(1 / (1 - r)) dB: that is dgamma (r over
    the set behind the absolute gate) and dlevel (r over the set behind both).  The sets are fixed only where no value lies
    within its rounding of a gate: |l'_j + 70| <= d_j, or |l'_j - gamma| <= d_j + dgamma for a value behind the absolute
    gate, makes the clip undecided, as in measure().  margin_bounds is the smallest such distance over its bound."""
    v = np.asarray(row, dtype=np.float64)[::every]
    g = Measured()
    d = np.where(np.isfinite(v), U * np.abs(np.where(np.isfinite(v), v, 0.0)) / (1.0 - U), 0.0)
    r = np.expm1(math.log(10.0) / 10.0 * d)
    z = np.where(np.isfinite(v), 10.0 ** ((np.where(np.isfinite(v), v, 0.0) + 0.691) / 10.0), 0.0)
    g.dv = d
    in_a = v > -70.0
    g.n_abs = int(in_a.sum())
    near = np.isfinite(v) & (np.abs(v + 70.0) <= d)
    with np.errstate(divide="ignore", invalid="ignore"):
        bounds = [np.inf] + list(np.abs(v + 70.0)[np.isfinite(v)] / np.maximum(d[np.isfinite(v)], 1e-300))
    g.undecided = bool(near.any())
    g.inside = np.zeros(v.shape, dtype=bool)
    g.n_rel, g.gamma, g.dgamma, g.level, g.dlevel = 0, -np.inf, 0.0, -np.inf, 0.0
    if g.n_abs:
        g.gamma = float(_l(z[in_a].mean()) + relative)
        g.dgamma = float(-10.0 * np.log10(1.0 - r[in_a].max()))
        g.undecided |= bool((np.abs(v[in_a] - g.gamma) <= d[in_a] + g.dgamma).any())
        bounds += list(np.abs(v[in_a] - g.gamma) / (d[in_a] + g.dgamma))
        g.inside = in_a & (v > g.gamma)
        g.n_rel = int(g.inside.sum())
        if g.n_rel:
            g.level = float(_l(z[g.inside].mean()))
            g.dlevel = float(-10.0 * np.log10(1.0 - r[g.inside].max()))
    g.values = v
    g.margin_bounds = float(min(bounds))
    return g
