"""The definition of beat tracking of clips (include/pdmp3_bulk.h pdmp3_amd_bulk_decode_clips_beats)
restated in numpy: binary64 throughout, every operation rounded once, in the stated order.  Nothing of the product's code.

The two blocked sums use reshape and cumsum (numpy's cumsum adds one element after the other); the local score adds one tap
after the other over all frames at once; the programme, the walk and the trim are plain loops."""
import numpy as np

BLOCK = 64


def half(P):
    """h = max(1, round-half-even(P / 2))"""
    return max(1, int(round(P / 2)))            # (Python rounds halves to even)


def period_of(bpm, sample_rate, hop):
    return int(round(60.0 * sample_rate / (hop * bpm)))


def tables(P, tightness):
    """g[0 .. P], tx[0 .. 2 P] (0 below h)"""
    k = np.arange(P + 1, dtype=np.float64)
    g = np.exp(-0.5 * (32.0 * k / P) ** 2)
    h = half(P)
    d = np.arange(2 * P + 1, dtype=np.float64)
    tx = np.zeros(2 * P + 1)
    tx[h:] = -tightness * (np.log(d[h:]) - np.log(float(P))) ** 2
    return g, tx


def blocked_sum(x):
    """blocks of 64 ascending from 0.0, then the blocks' sums ascending from 0.0 (a trailing +0.0 changes no sum)"""
    x = np.asarray(x, dtype=np.float64)
    pad = (-x.size) % BLOCK
    blocks = np.concatenate([x, np.zeros(pad)]).reshape(-1, BLOCK)
    sums = np.cumsum(np.concatenate([np.zeros((blocks.shape[0], 1)), blocks], axis=1), axis=1)[:, -1]
    return float(np.cumsum(np.concatenate([[0.0], sums]))[-1])


def normalise(o):
    """-> (m, norm) of the n = len(o) frames that enter"""
    o = np.asarray(o, dtype=np.float32).astype(np.float64)
    n = o.size
    m = blocked_sum(o) / n
    d = o - m
    with np.errstate(all="ignore"):
        return m, float(np.sqrt(np.float64(blocked_sum(d * d)) / np.float64(n - 1)))


def runs(o):
    """item 8's first two cases"""
    if len(o) < 2:
        return False
    norm = normalise(o)[1]
    return bool(norm > 0.0 and np.isfinite(norm))


def local_score(o, P, g):
    """-> (the sums in binary64, ls as binary32)"""
    o = np.asarray(o, dtype=np.float32).astype(np.float64)
    n = o.size
    z = np.concatenate([np.zeros(P), o / normalise(o)[1], np.zeros(P)])
    s = np.zeros(n)
    for k in range(2 * P + 1):                   # j = i - P + k ascending
        s = s + z[k:k + n] * g[abs(k - P)]
    return s, s.astype(np.float32)


def programme(ls, P, tx):
    """-> (cum float64 [n], back int [n])"""
    ls = np.asarray(ls, dtype=np.float32)
    n, h = ls.size, half(P)
    l64 = ls.astype(np.float64)
    hit = np.nonzero(l64 >= 0.01 * l64.max())[0]
    i0 = int(hit[0]) if hit.size else n
    cum, back = np.zeros(n), np.full(n, -1, dtype=np.int64)
    for i in range(n):
        hi = min(2 * P, i)
        best, at = -np.inf, 0
        if hi >= h:
            d = np.arange(h, hi + 1)
            v = cum[i - d] + tx[d]
            a = int(np.argmax(v))                # (the first of equal ones: the smallest d)
            if v[a] > -np.inf:
                best, at = float(v[a]), int(d[a])
        cum[i] = l64[i] + best if at else l64[i]
        back[i] = i - at if at and i >= i0 else -1
    return cum, back


def local_maxima(cum):
    n = cum.size
    lm = np.zeros(n, dtype=bool)
    if n >= 2:
        lm[1:-1] = (cum[1:-1] > cum[:-2]) & (cum[1:-1] >= cum[2:])
        lm[-1] = cum[-1] > cum[-2]
    return lm


def pick(ls, cum, back, trim):
    """-> dict: beats (the kept ones), q (before the trim), tail, thr, maxima; -1 where not reached"""
    l64 = np.asarray(ls, dtype=np.float32).astype(np.float64)
    res = dict(beats=np.zeros(0, dtype=np.int64), q=-1, tail=-1, thr=-1.0, maxima=0)
    lm = local_maxima(cum)
    vals = np.sort(cum[lm])
    M = res["maxima"] = int(vals.size)
    if not M:
        return res
    med = vals[M // 2] if M & 1 else 0.5 * (vals[M // 2 - 1] + vals[M // 2])
    tails = np.nonzero(lm & (cum >= 0.5 * med))[0]
    if not tails.size:
        res["q"] = 0
        return res
    res["tail"] = i = int(tails[-1])
    b = []
    while i >= 0:
        b.append(i)
        i = int(back[i])
    b = np.array(b[::-1], dtype=np.int64)
    q = res["q"] = b.size
    lb = np.concatenate([[0.0], l64[b], [0.0]])
    s = (0.5 * lb[:-2] + lb[1:-1]) + 0.5 * lb[2:]
    ss = 0.0
    for v in s:
        ss = ss + v * v
    thr = res["thr"] = 0.5 * float(np.sqrt(np.float64(ss) / np.float64(q))) if trim else 0.0
    keep = np.nonzero(s > thr)[0]
    if keep.size:
        res["beats"] = b[keep[0]:keep[-1] + 1]
    return res


def track(o, n_frames, P, g, tx, trim=True):
    """the whole chain on the envelope of the n = len(o) frames that enter -> dict: score [F], dp [2, F], beats [2, F] (float32) and
    stats[2:8] (kept, beats, tail, norm, thr, n)"""
    F, n = int(n_frames), len(o)
    score = np.zeros(F, dtype=np.float32)
    dp = np.stack([np.zeros(F, dtype=np.float32), np.full(F, -1.0, dtype=np.float32)])
    rows = np.stack([np.zeros(F, dtype=np.float32), np.full(F, -1.0, dtype=np.float32)])
    stats = [0.0, -1.0, -1.0, -1.0, -1.0, float(n)]
    if runs(o):
        stats[3] = np.float32(normalise(o)[1])
        score[:n] = local_score(o, P, g)[1]
        cum, back = programme(score[:n], P, tx)
        with np.errstate(over="ignore"):
            dp[0, :n], dp[1, :n] = cum.astype(np.float32), back.astype(np.float32)
        r = pick(score[:n], cum, back, trim)
        b = r["beats"]
        rows[0, b], rows[1, :b.size] = 1.0, b
        if r["maxima"]:
            stats[0], stats[1], stats[2], stats[4] = float(b.size), float(r["q"]), float(r["tail"]), np.float32(r["thr"])
    return dict(score=score, dp=dp, beats=rows, stats=np.array(stats, dtype=np.float32))
