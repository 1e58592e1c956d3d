"""The contract of recursive filtering (include/grail_hip.h, "levels, continued: recursive filtering" and "... of streams") in
numpy: a Python loop over time and over sections, vectorised over rows.  numpy's float64 is IEEE binary64, every operation
rounded by itself, nothing fused: the operations below are the header's, in the header's order.  A row with fewer sections
than another takes the longer one's further sections' results by no route: they are computed and dropped (np.where), never
run as identities."""
import numpy as np

FLT_MAX = np.float32(3.4028234663852886e38)
REFUSED = 0xFFFFFFFF
SECTIONS_MAX = 8


def clean(x):
    """(the samples as binary64 with +0.0 in place of the non-finite ones, the count of those)"""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        finite = np.abs(x) <= FLT_MAX
    return np.where(finite, x, np.float32(0.0)).astype(np.float64), int(np.count_nonzero(~finite))


def table(filters, which):
    """(c float64 [R][8][5], S int [R]) for rows bound to filters[which[r]]; a filter is float64 [S][5] or flat [5 S]"""
    c = np.zeros((len(which), SECTIONS_MAX, 5), np.float64)
    S = np.zeros(len(which), np.int64)
    for r, f in enumerate(which):
        sec = np.asarray(filters[f], np.float64).reshape(-1, 5)
        assert 1 <= len(sec) <= SECTIONS_MAX
        c[r, :len(sec)] = sec
        S[r] = len(sec)
    return c, S


def run(v, steps, c, S, s1, s2):
    """v: float64 [R][T], row r's inputs (+0.0 where it has none); steps: int [R], a row's state stops at its steps-th input.
    s1, s2: float64 [R][8], updated in place.  Returns float64 [R][T], what leaves the rows' last sections before the one
    rounding to binary32 (garbage past a row's steps)."""
    R, T = v.shape
    out = np.zeros((R, T), np.float64)
    most = int(S.max()) if R else 0
    with np.errstate(all="ignore"):
        for t in range(T):
            live = steps > t
            x = v[:, t].copy()
            for j in range(most):
                has = S > j
                y = c[:, j, 0] * x + s1[:, j]
                n1 = (c[:, j, 1] * x - c[:, j, 3] * y) + s2[:, j]
                n2 = c[:, j, 2] * x - c[:, j, 4] * y
                s1[:, j] = np.where(live & has, n1, s1[:, j])
                s2[:, j] = np.where(live & has, n2, s2[:, j])
                x = np.where(has, y, x)
            out[:, t] = x
    return out


def to_f32(y):
    with np.errstate(all="ignore"):
        return np.asarray(y, np.float64).astype(np.float32)


def iir_model(rows, filters, which=None, tail=0, out_stride=None, lens=None, exact=False):
    """grail_iir_async on rows (a list of float32 arrays), row r through filters[which[r]] (None: filter 0): a list of
    (out float32 [n_out], n_out, nonfinite), or (None, REFUSED, 0) for a row whose index is outside the set.  lens: what
    len_dev holds, where it is not the rows' own lengths (a row is min(len, its samples) long).  exact: out is the float64
    before the one rounding."""
    which = [0] * len(rows) if which is None else list(which)
    ok = [r for r in range(len(rows)) if which[r] < len(filters)]
    result = [(None, REFUSED, 0)] * len(rows)
    if not ok:
        return result
    xs = [np.asarray(rows[r], np.float32)[:None if lens is None else min(int(lens[r]), len(rows[r]))] for r in ok]
    n = np.array([len(x) for x in xs], np.int64)
    n_out = np.where(n == 0, 0, n + tail)
    if out_stride is not None:
        n_out = np.minimum(n_out, out_stride)
    T = int(n_out.max())
    v = np.zeros((len(ok), max(T, 1)), np.float64)
    bad = []
    for k, x in enumerate(xs):
        vx, b = clean(x)
        v[k, :min(len(x), T)] = vx[:T]
        bad.append(b)                                          # (over all n samples, also where out_stride cut the output)
    c, S = table(filters, [which[r] for r in ok])
    s1, s2 = np.zeros((len(ok), SECTIONS_MAX)), np.zeros((len(ok), SECTIONS_MAX))
    y = run(v[:, :T], n_out, c, S, s1, s2)
    for k, r in enumerate(ok):
        yk = y[k, :n_out[k]]
        result[r] = (yk.copy() if exact else to_f32(yk), int(n_out[k]), bad[k])
    return result


class IirStreamModel:
    """grail_iir_stream_*: n_rows rows, row r bound to filters[which[r]], one tail for all; the state carried between calls"""

    def __init__(self, filters, which, tail):
        self.c, self.S = table(filters, which)
        self.tail = tail
        R = len(which)
        self.s1, self.s2 = np.zeros((R, SECTIONS_MAX)), np.zeros((R, SECTIONS_MAX))
        self.fed = np.zeros(R, np.int64)
        self.ended = np.zeros(R, bool)

    def next(self, chunks):
        """chunks[r]: the float32 samples row r is fed -> [(out float32 [n], n, nonfinite)]; (None, REFUSED, 0) for a row
        that has ended and is fed, its state as it was"""
        R = len(chunks)
        n = np.array([len(x) for x in chunks], np.int64)
        refused = self.ended & (n > 0)
        take = np.where(self.ended, 0, n)
        T = int(take.max()) if R else 0
        v = np.zeros((R, max(T, 1)), np.float64)
        bad = [0] * R
        for r, x in enumerate(chunks):
            if take[r]:
                v[r, :take[r]], bad[r] = clean(x)
        y = run(v[:, :T], take, self.c, self.S, self.s1, self.s2)
        self.fed += take
        return [(None, REFUSED, 0) if refused[r] else (to_f32(y[r, :take[r]]), int(take[r]), bad[r]) for r in range(R)]

    def finish(self, marks=None):
        """the rows marked (None: all) that have not ended ring out and end -> [tail float32 [0 or tail]]"""
        R = len(self.fed)
        marks = np.ones(R, bool) if marks is None else np.asarray(marks).astype(bool)
        takes = marks & ~self.ended
        count = np.where(takes & (self.fed > 0), self.tail, 0)
        T = int(count.max()) if R else 0
        y = run(np.zeros((R, T), np.float64), count, self.c, self.S, self.s1, self.s2)
        self.ended |= takes
        return [to_f32(y[r, :count[r]]) for r in range(R)]


def stream_len(fed_before, n, tail, finishing):
    """grail_iir_stream_len"""
    return (tail if fed_before else 0) if finishing else n


def response(coef, w):
    """|H(e^jw)| of sections float64 [S][5], in numpy's complex128"""
    z1 = np.exp(-1j * np.asarray(w, np.float64))
    h = np.ones_like(z1)
    for b0, b1, b2, a1, a2 in np.asarray(coef, np.float64).reshape(-1, 5):
        h = h * (b0 + b1 * z1 + b2 * z1 * z1) / (1.0 + a1 * z1 + a2 * z1 * z1)
    return np.abs(h)
