"""The contract of dynamics (include/grail_hip.h, "levels, continued: dynamics" and "... of streams") in numpy: a Python loop
over time, vectorised over rows as a wave is.  numpy's float64 is IEEE binary64, every operation rounded by itself, nothing
fused: the operations below are the header's, in the header's order.  The lookup takes the envelope's exponent and mantissa
fields as the header names them, and f as the integer's exact conversion times 2^-48.  Beside it the designer's and the
ballistics' formulas in Python floats."""
import math

import numpy as np

FLT_MAX = np.float32(3.4028234663852886e38)
REFUSED = 0xFFFFFFFF
STEPS, LOG2_LO, LOG2_HI, POINTS, CURVES_MAX = 16, -32, 8, 641, 16
PEAK, SQUARE = 0, 1
COMPRESS, EXPAND = 0, 1


def level(k):
    """lev[k], exact"""
    return math.ldexp(1.0 + (k % STEPS) / STEPS, LOG2_LO + k // STEPS)


LEVELS = np.array([level(k) for k in range(POINTS)], np.float64)


def clean(x):
    """(the samples as binary64 with +0.0 in place of the non-finite ones, the count of those)"""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        finite = np.abs(x) <= FLT_MAX
    return np.where(finite, x, np.float32(0.0)).astype(np.float64), int(np.count_nonzero(~finite))


def index(e):
    """(k int [..], f float64 [..], inside bool [..]) of e float64 [..] (finite, >= 0): the header's E, m, k and f; k = 0 where
    e is not inside [2^LO, 2^HI)"""
    e = np.ascontiguousarray(e, np.float64)
    bits = e.view(np.uint64)
    E = (bits >> np.uint64(52)).astype(np.int64) & 0x7FF
    m = bits & np.uint64((1 << 52) - 1)
    inside = (e >= 2.0 ** LOG2_LO) & (e < 2.0 ** LOG2_HI)
    k = np.where(inside, (E - (1023 + LOG2_LO)) * STEPS + (m >> np.uint64(48)).astype(np.int64), 0)
    f = (m & np.uint64((1 << 48) - 1)).astype(np.float64) * 2.0 ** -48
    return k, f, inside


def lookup(G, e):
    """curve(e) for e float64 [R] (finite, >= 0) on the rows' curves G float64 [R][641]"""
    rows = np.arange(len(e))
    k, f, inside = index(e)
    lo, hi = G[rows, k], G[rows, np.minimum(k + 1, POINTS - 1)]
    g = lo + f * (hi - lo)
    return np.where(e < 2.0 ** LOG2_LO, G[:, 0], np.where(inside, g, G[:, POINTS - 1]))


def lookup_one(gain, e):
    """curve(e) for many e on one curve gain float64 [641]"""
    gain = np.asarray(gain, np.float64)
    k, f, inside = index(e)
    lo, hi = gain[k], gain[np.minimum(k + 1, POINTS - 1)]
    g = lo + f * (hi - lo)
    return np.where(np.asarray(e) < 2.0 ** LOG2_LO, gain[0], np.where(inside, g, gain[POINTS - 1]))


def run(v, w, steps, G, attack, release, square, e, min_gain):
    """v, w: float64 [R][T], the rows' samples and their keys' (+0.0 where there are none); steps: int [R], a row's own
    samples.  e, min_gain: float64 [R], updated in place up to each row's steps (min_gain from +inf: the caller says 1.0 for a
    row of no samples).  Returns g * v, float64 [R][T] (garbage past
    a row's steps)."""
    R, T = v.shape
    out = np.zeros((R, T), np.float64)
    for t in range(T):
        live = steps > t
        wt = w[:, t]
        a = np.where(square, wt * wt, np.abs(wt))
        alpha = np.where(a > e, attack, release)
        en = a + alpha * (e - a)
        e[:] = np.where(live, en, e)
        g = lookup(G, en)
        min_gain[:] = np.where(live & (g < min_gain), g, min_gain)
        out[:, t] = g * v[:, t]
    return out


def to_f32(y):
    with np.errstate(all="ignore"):
        return np.asarray(y, np.float64).astype(np.float32)


def bind(curves, which):
    """(G [R][641], attack [R], release [R], square [R]) for rows bound to curves[which[r]]; a curve is (gain [641], (alpha_attack,
    alpha_release), detector)"""
    G = np.array([np.asarray(curves[c][0], np.float64) for c in which]).reshape(len(which), POINTS)
    attack = np.array([curves[c][1][0] for c in which], np.float64)
    release = np.array([curves[c][1][1] for c in which], np.float64)
    square = np.array([curves[c][2] == SQUARE for c in which], bool)
    return G, attack, release, square


def dyn_model(rows, curves, which=None, keys=None, key_row=None, key_lens=None, out_stride=None, lens=None):
    """grail_dyn_async on rows (a list of float32 arrays), row r on curves[which[r]] (None: curve 0), keyed by keys[key_row[r]]
    (keys None: self-keyed; key_row None: row r listens to key r): a list of (out float32 [n_out], n_out, nonfinite, min_gain),
    or (None, REFUSED, 0, nan) for a row whose curve or key index is outside.  lens / key_lens: what len_dev / key_len_dev
    hold, where they are not the arrays' own lengths."""
    which = [0] * len(rows) if which is None else list(which)
    if keys is not None:
        key_row = list(range(len(rows))) if key_row is None else list(key_row)
    ok = [r for r in range(len(rows)) if which[r] < len(curves) and (keys is None or key_row[r] < len(keys))]
    result = [(None, REFUSED, 0, float("nan"))] * len(rows)
    if not ok:
        return result
    xs = [np.asarray(rows[r], np.float32)[:None if lens is None else min(int(lens[r]), len(rows[r]))] for r in ok]
    n = np.array([len(x) for x in xs], np.int64)
    T = int(n.max())
    v = np.zeros((len(ok), max(T, 1)), np.float64)
    bad = []
    for i, x in enumerate(xs):
        v[i, :len(x)], b = clean(x)
        bad.append(b)
    if keys is None:
        w = v
    else:
        w = np.zeros_like(v)
        for i, r in enumerate(ok):
            kx = np.asarray(keys[key_row[r]], np.float32)
            if key_lens is not None:
                kx = kx[:min(int(key_lens[key_row[r]]), len(kx))]
            kx = kx[:T]
            w[i, :len(kx)] = clean(kx)[0]
    G, attack, release, square = bind(curves, [which[r] for r in ok])
    e, mg = np.zeros(len(ok)), np.full(len(ok), np.inf)
    y = run(v[:, :T], w[:, :T], n, G, attack, release, square, e, mg)
    for i, r in enumerate(ok):
        n_out = int(n[i]) if out_stride is None else min(int(n[i]), out_stride)
        result[r] = (to_f32(y[i, :n_out]), n_out, bad[i], float(mg[i]) if n[i] else 1.0)
    return result


class DynStreamModel:
    """grail_dyn_stream_*: n_rows rows, row r bound to curves[which[r]] (and, keyed, to the key key_row[r] of each call); e
    carried between calls"""

    def __init__(self, curves, which, key_row=None):
        self.bound = bind(curves, which)
        self.key_row = key_row
        self.e = np.zeros(len(which))
        self.fed = np.zeros(len(which), np.int64)

    def next(self, chunks, keys=None):
        """chunks[r]: the float32 samples row r is fed; keys: the call's key rows (a keyed stream), of which row r reads
        the first len(chunks[r]) -> [(out float32 [n], n, nonfinite, min_gain)]"""
        R = len(chunks)
        n = np.array([len(x) for x in chunks], np.int64)
        T = int(n.max()) if R else 0
        v = np.zeros((R, max(T, 1)), np.float64)
        bad = [0] * R
        for r, x in enumerate(chunks):
            if n[r]:
                v[r, :n[r]], bad[r] = clean(x)
        if self.key_row is None:
            w = v
        else:
            w = np.zeros_like(v)
            for r in range(R):
                if n[r]:
                    w[r, :n[r]] = clean(np.asarray(keys[self.key_row[r]], np.float32)[:n[r]])[0]
        mg = np.full(R, np.inf)
        y = run(v[:, :T], w[:, :T], n, *self.bound, self.e, mg)
        self.fed += n
        return [(to_f32(y[r, :n[r]]), int(n[r]), bad[r], float(mg[r]) if n[r] else 1.0) for r in range(R)]


# ---- the designer and the ballistics, in Python floats, in the header's order ----------------------------------------------------
def level_db(lev, detector):
    return (20.0 if detector == PEAK else 10.0) * math.log10(lev)


def reduction_db(kind, x, T, R, W, range_db):
    """r of the header: y - x of the static curve at the level x dB"""
    d, h = x - T, W / 2.0
    if kind == COMPRESS:
        if d <= -h:
            return 0.0
        if d >= h:
            return (T + d / R) - x
        q = d + h
        return ((1.0 / R - 1.0) * (q * q)) / (2.0 * W)
    if d >= h:
        r = 0.0
    elif d <= -h:
        r = (T + d * R) - x
    else:
        q = d - h
        r = ((1.0 - R) * (q * q)) / (2.0 * W)
    return -range_db if r < -range_db else r


def design_model(kind, detector, T, R, W, range_db, makeup_db):
    return np.array([math.pow(10.0, (reduction_db(kind, level_db(level(k), detector), T, R, W, range_db) + makeup_db) / 20.0)
                     for k in range(POINTS)], np.float64)


def ideal_gain_db(kind, detector, e, T, R, W, range_db, makeup_db):
    """the curve the table samples, at any level e > 0, in dB"""
    return reduction_db(kind, level_db(e, detector), T, R, W, range_db) + makeup_db


def ballistics_model(rate, attack_ms, release_ms):
    return np.array([0.0 if ms == 0.0 else math.exp(-1000.0 / (ms * float(rate))) for ms in (attack_ms, release_ms)], np.float64)
