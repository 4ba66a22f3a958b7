"""Chroma features of clips (include/pdmp3_bulk.h) restated with numpy alone: the class of a bin, the
kernel's plan, the definition in binary64 on top of tests/clip_cqt_ref.py -- and the binary32 error bound the tests hold the
product to.  Nothing here is the product's code.

Definition.
  1. Q_k[f] is section 16's magnitude (quantity 1) or power (2) of bin k of frame f: clip_cqt_ref.cqt.
  2. class(k) = ((k + r // 2) // r + base_class) mod n_chroma, r = bins_per_octave // n_chroma.
  3. C_p[f] = sum of Q_k[f] over the bins of class p (0 without a bin).
  4. D[f] over the classes: L1 sum_p C_p; L2 sqrt(sum_p C_p^2); max max_p C_p.
  5. Out_p[f] = C_p / max(D, floor), floor rounded to binary32 first; C_p itself at chroma_norm 0.

The product (lower case) computes q_k as decode_clips_cqt does, c_p as the binary32 sum of its bins in ascending k from the
first term on, d as ((c_0 + c_1) + ..), as sqrtf of s = c_0 c_0, s = fma(c_p, c_p, s), or as the exact maximum, and
c_p / max(d, floor) by one division.  The build's binary32 division and sqrtf are the correctly rounded ones (the HIP compiler's
default, no flag of the project's touches it; the host test and the GPU test hold L1 and max against numpy's binary32
division bit for bit), so the quotient's rounding is one u.

The bound (u = 2^-24; e_k is clip_cqt_ref's bound on q_k, taken from there and not restated):
  class of n bins:  |dc_p| <= sum e_k + n u sum (Q_k + e_k) for n >= 2, sum e_k for n <= 1.  The chain commits n - 1 roundings,
    each at most u times a partial sum, which is at most sum q_k (1 + u)^(n - 2): (1 + u)^(n - 1) - 1 <= n u covers them with
    the second-order terms, the project's convention (clip_cqt_ref: N_k + 2 in the place of N_k + 1), and q_k <= Q_k + e_k.
  L1:  the same rule over the n_chroma classes: |dd| <= sum dc_p + n_chroma u sum (C_p + dc_p).
  max: |dd| <= max_p dc_p (the maximum is 1-Lipschitz in the maximum norm, and exact).
  L2:  the Euclidean norm is 1-Lipschitz: | ||c|| - ||C|| | <= g = sqrt(sum dc_p^2).  The chain's n_chroma roundings give
    s = ||c||^2 (1 + t), |t| <= T = (1 + u)^n_chroma - 1, plus at most 2^-150 of underflow a step; sqrtf adds one u:
    |dd| <= g + (||C|| + g) SQRT_CN + 2 sqrt(n_chroma 2^-150), SQRT_CN = (1 + T / (2 - T)) (1 + u) - 1: clip_stft_ref's
    SQRT_C with T in the place of its T2.
  max(d, floor) is 1-Lipschitz: the divisors differ by at most dd.
  quotient:  c / m - C / M = (c - C) / m + (C / M) (M - m) / m, so with d' = max(M - dd, floor) <= m and rho =
    (C_p + dc_p) / d' >= |c_p / m|:  |dOut_p| <= (dc_p + rho dd) / d' + u rho + 2^-150 (the last: a quotient below the normal
    range).  No new measured constant."""
import numpy as np

import clip_cqt_ref as cref

U = cref.U
T2 = cref.T2
FMIN_C1 = cref.FMIN_C1
FMIN_C2 = 2.0 * FMIN_C1
FMIN_C3 = 4.0 * FMIN_C1
NORMS = {None: 0, "l1": 1, "l2": 2, "max": 3}
QUANTITIES = {"magnitude": 1, "power": 2}
PART_FLOATS = cref.PART_FLOATS
LDS_SOFT, LDS_MAX = cref.LDS_SOFT, cref.LDS_MAX
TINY = 2.0 ** -150

valid = cref.valid


def class_map(n_bins, bins_per_octave, n_chroma, base_class):
    """-> (class of every bin int64 [n_bins], bins of every class int64 [n_chroma])"""
    r = bins_per_octave // n_chroma
    k = np.arange(n_bins, dtype=np.int64)
    cls = ((k + r // 2) // r + base_class) % n_chroma
    return cls, np.bincount(cls, minlength=n_chroma)


def plan(sr, hop, **geo):
    """the plan of a workgroup of k_clip_chroma restated: (tile, row_pad, lds_bytes, split rows, segments, split tiles, floats in
    front of the q plane, floats in front of the class plane, launch path), None where no tile fits the LDS or the constant-Q
    transform's own plan finds none.  The LDS: the span | 8 x 2 x 16 x 17 partial sums, the class plane [n_chroma][17] over them |
    the q plane [n_bins rounded up to 16][17]."""
    if cref.plan(sr, hop, **geo) is None:
        return None
    rows, _ = cref.tiles(sr, **geo)
    pad = (2 - hop) % 32
    n_split = int((rows >= cref.SPLIT_ROWS).sum())
    q_floats = len(rows) * 16 * 17
    for tile in (16, 8, 4):
        span = (tile - 1) * hop + int(rows[0])
        span_floats = (-(-span // hop) * (hop + pad) + 3) // 4 * 4
        lds = (span_floats + PART_FLOATS + q_floats) * 4
        if lds <= LDS_MAX:
            return (tile, pad, lds, cref.SPLIT_ROWS, cref.SEGMENTS, n_split, span_floats + PART_FLOATS, span_floats,
                    "tile%d-%s" % (tile, "dyn" if lds <= LDS_SOFT else "static"))
    return None


def fold32(q, cls, n_chroma):
    """q: binary32 [..., n_bins, F] -> the binary32 sequential fold [..., n_chroma, F]: a class's bins in ascending k, from the
    first term on by plain additions; +0 without a bin"""
    q = np.asarray(q, dtype=np.float32)
    out = np.zeros(q.shape[:-2] + (n_chroma, q.shape[-1]), dtype=np.float32)
    seen = np.zeros(n_chroma, dtype=bool)
    for k, p in enumerate(cls):
        out[..., p, :] = out[..., p, :] + q[..., k, :] if seen[p] else q[..., k, :]
        seen[p] = True
    return out


def normalise32(c, norm, floor):
    """c: binary32 [..., n_chroma, F] -> the product's quotient in binary32 for norm 1 (L1) and 3 (max), bit for bit where the
    build's division is the correctly rounded one"""
    c = np.asarray(c, dtype=np.float32)
    if norm == 3:
        d = c.max(axis=-2)
    else:
        assert norm == 1
        d = c[..., 0, :].copy()
        for p in range(1, c.shape[-2]):
            d = d + c[..., p, :]
    return c / np.maximum(d, np.float32(floor))[..., None, :]


def chroma(y, pos0, start, n_frames, sr, hop, quantity, n_chroma=12, base_class=0, chroma_norm=3, norm_floor=1e-10, **kw):
    """y: [C, T] binary32 values of the signal from position pos0 on -> (out, bound), binary64 [C, n_chroma, F]: the definition
    on those values, and what the product's binary32 evaluation may differ from it by (the module's docstring)"""
    q, e = cref.cqt(y, pos0, start, n_frames, sr, hop, quantity, **kw)
    return from_cqt(q, e, kw.get("bins_per_octave", 12), n_chroma, base_class, chroma_norm, norm_floor)


def from_cqt(q, e, bins_per_octave, n_chroma, base_class, chroma_norm, norm_floor=1e-10):
    """q, e: clip_cqt_ref.cqt's values and bounds at mode 1 or 2, [C, n_bins, F] -> (out, bound) as chroma()"""
    n_bins, n_frames = q.shape[1], q.shape[2]
    cls, count = class_map(n_bins, bins_per_octave, n_chroma, base_class)
    c = np.zeros((q.shape[0], n_chroma, n_frames))
    dc = np.zeros_like(c)
    for p in range(n_chroma):
        mine = cls == p
        n = int(count[p])
        c[:, p] = q[:, mine].sum(axis=1)
        dc[:, p] = e[:, mine].sum(axis=1) + (n * U * (q[:, mine] + e[:, mine]).sum(axis=1) if n >= 2 else 0.0)
    if chroma_norm == 0:
        return c, dc
    floor = float(np.float32(norm_floor))
    if chroma_norm == 1:
        d = c.sum(axis=1)
        dd = dc.sum(axis=1) + n_chroma * U * (c + dc).sum(axis=1)
    elif chroma_norm == 3:
        d = c.max(axis=1)
        dd = dc.max(axis=1)
    else:
        assert chroma_norm == 2
        d = np.sqrt((c * c).sum(axis=1))
        g = np.sqrt((dc * dc).sum(axis=1))
        t = (1.0 + U) ** n_chroma - 1.0
        sqrt_cn = (1.0 + t / (2.0 - t)) * (1.0 + U) - 1.0
        dd = g + (d + g) * sqrt_cn + np.where(d + g > 0.0, 2.0 * np.sqrt(n_chroma * TINY), 0.0)
    m = np.maximum(d, floor)[:, None]
    low = np.maximum(m - dd[:, None], floor)
    rho = (c + dc) / low
    bound = (dc + rho * dd[:, None]) / low + U * rho + np.where(rho > 0.0, TINY, 0.0)
    return c / m, bound
