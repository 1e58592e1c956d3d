"""The contract of filter streams (include/grail_hip.h, "levels, continued: FIR filtering of streams") in numpy, on top of
tests/fir_model.py: a row's samples are fed in calls; after N samples the outputs E(N) = max(0, N - origin) are known, a call
that feeds n samples writes outputs E(N) .. E(N + n) - 1 of the one-shot contract applied to everything fed so far, and
finish writes the rest, E(N) .. N + K - 1 - origin - 1."""
import numpy as np

from fir_model import fir_model


def known(N, origin):
    """E(N): the outputs that can be known after N samples (output m needs sample m + origin)"""
    return max(0, N - origin)


def stream_len(fed_before, n, K, origin, finishing=False):
    """the count a call writes for a row that was fed fed_before samples before it"""
    if finishing:
        return 0 if fed_before == 0 else fed_before + K - 1 - origin - known(fed_before, origin)
    return known(fed_before + n, origin) - known(fed_before, origin)


def stream_model(x, h, origin, split):
    """x: all the samples a row is fed, split: how many each `next` call feeds (zeros allowed, sum = len(x)) ->
    ([(y float32, nonfinite) per call], tail float32).  Every call's outputs come from the one-shot model on the samples fed
    up to and including that call: later samples cannot have changed them."""
    x = np.asarray(x, np.float32)
    assert sum(split) == len(x) and all(n >= 0 for n in split)
    calls, N = [], 0
    for n in split:
        fed = x[:N + n]
        y, _, _ = fir_model(fed, h, origin, m_lo=known(N, origin), m_hi=known(N + n, origin))
        assert len(y) == stream_len(N, n, len(h), origin)
        calls.append((y, int(np.count_nonzero(~np.isfinite(x[N:N + n])))))
        N += n
    tail, n_out, _ = fir_model(x, h, origin, m_lo=known(N, origin))
    assert len(tail) == stream_len(N, 0, len(h), origin, finishing=True) == n_out - min(known(N, origin), n_out)
    return calls, tail


def splits(N, K, chunk, rng):
    """the issue's splits of N samples: all at once; [1, K - 1, K, 0, rest]; cuts at chunk - 1 and chunk + 1; a seeded random
    split with zeros.  Parts that do not fit are cut to what is left, so every split sums to N."""
    def fit(parts):
        out, left = [], N
        for p in parts:
            p = min(p, left)
            out.append(p)
            left -= p
        return out + [left]

    cuts = fit([chunk - 1, 2])                          # cuts at chunk - 1 and chunk + 1
    random = []
    left = N
    while left:
        p = 0 if rng.random() < 0.25 else int(min(left, rng.integers(1, max(2, N // 3 + 1))))
        random.append(p)
        left -= p
    return [[N], fit([1, K - 1, K, 0]), cuts, random + [0]]
