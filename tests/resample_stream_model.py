"""The contract of resample streams (include/grail_hip.h, "levels, continued: sample-rate conversion of streams") in numpy,
on top of tests/resample_model.py: a row's samples are fed in calls; one-shot output m reads the samples i0 - h + 1 .. i0 + h
with i0 = floor(m D / U) and h = P / 2, so after N samples the outputs E(N) = 0 for N <= h, else ceil((N - h) U / D) are
known; a call that feeds n samples writes outputs E(N) .. E(N + n) - 1 of the one-shot contract applied to everything fed so
far, and finish writes the rest, E(N) .. ceil(N U / D) - 1.  All lengths are Python integers: no width to overflow."""
import numpy as np

from resample_model import resample_model


def ceil_div(a, b):
    return -(-a // b)


def known(N, U, D, P):
    """E(N): the outputs that can be known after N samples (output m needs sample floor(m D / U) + P / 2)"""
    h = P // 2
    return 0 if N <= h else ceil_div((N - h) * U, D)


def stream_len(fed_before, n, U, D, P, finishing=False):
    """the count a call writes for a row that was fed fed_before samples before it"""
    if finishing:
        assert n == 0
        return ceil_div(fed_before * U, D) - known(fed_before, U, D, P)
    return known(fed_before + n, U, D, P) - known(fed_before, U, D, P)


def advance(i, p, N, n, U, D, P, finishing=False):
    """The incremental form the device keeps instead of E(N) (N U outgrows 64 bits long before N does): i = floor(M D / U)
    and p = M D mod U of the next output M.  -> (count, i, p) of a call that feeds n samples to a row fed N before it:
    the outputs whose i0 <= T, T = N + n - 1 - h (finishing: T = N - 1, the samples to come being +0.0)."""
    T = N - 1 if finishing else N + n - 1 - P // 2
    c = 0 if T < i else ceil_div((T - i + 1) * U - p, D)
    assert (T - i + 1) * U < 2 ** 44 or T < i
    return c, i + (p + c * D) // U, (p + c * D) % U


def stream_model(x, num, D, split):
    """x: all the samples a row is fed, num int32[U, P] the pair's table, split: how many each `next` call feeds (zeros
    allowed, sum = len(x)) -> ([(y float32, nonfinite) per call], tail float32).  Every call's outputs come from the one-shot
    model on the samples fed up to and including that call: later samples cannot have changed them."""
    x = np.asarray(x, np.float32)
    (U, P), D = num.shape, int(D)
    h = P // 2
    assert sum(split) == len(x) and all(n >= 0 for n in split)
    calls, N, i, p = [], 0, 0, 0
    for n in split:
        lo, hi = known(N, U, D, P), known(N + n, U, D, P)
        y, _, _ = resample_model(x[:N + n], num, D, m_lo=lo, m_hi=hi)
        assert len(y) == stream_len(N, n, U, D, P) <= ceil_div(n * U, D)
        # no sample before N - (P - 1) is needed: the first new output's lowest tap
        assert hi == lo or lo * D // U - h + 1 >= N - (P - 1)
        c, i, p = advance(i, p, N, n, U, D, P)
        assert c == len(y) and (i, p) == (hi * D // U, hi * D % U)
        calls.append((y, int(np.count_nonzero(~np.isfinite(x[N:N + n])))))
        N += n
    tail, n_out, _ = resample_model(x, num, D, m_lo=known(N, U, D, P))
    assert len(tail) == stream_len(N, 0, U, D, P, finishing=True) == n_out - known(N, U, D, P) <= ceil_div(h * U, D)
    assert advance(i, p, N, 0, U, D, P, finishing=True)[0] == len(tail) and (N or len(tail) == 0)
    return calls, tail


def splits(N, P, Ci, rng):
    """the issue's splits of N samples: all at once; [1, h, h + 1, 0, rest]; cuts either side of Ci, the input samples of one
    output chunk; a seeded random split with zeros.  Parts that do not fit are cut to what is left, so every split sums to N."""
    def fit(parts):
        out, left = [], N
        for p in parts:
            p = min(p, left)
            out.append(p)
            left -= p
        return out + [left]

    h = P // 2
    random = []
    left = N
    while left:
        p = 0 if rng.random() < 0.25 else int(min(left, rng.integers(1, max(2, N // 3 + 1))))
        random.append(p)
        left -= p
    return [[N], fit([1, h, h + 1, 0]), fit([Ci - 1, 2]), random + [0]]
