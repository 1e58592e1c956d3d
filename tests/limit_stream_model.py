"""The contract of limit streams (include/grail_hip.h, "levels, continued: the limiter on streams") in numpy, on top of
limiter_model of tests/test_limiter_host.py: a group's samples are fed in calls; z[t] needs q up to t + L - 1 and q[s] needs x
up to s + 11, so after N samples the outputs E(N) = max(0, N - LAMBDA), LAMBDA = L + 10, are final; a call that feeds n
samples writes outputs E(N) .. E(N + n) - 1 of the one-shot contract applied to everything fed so far, and finish writes the
rest, E(N) .. N - 1, from the whole row.  All lengths are Python integers: no width to overflow."""
import numpy as np

from test_limiter_host import Q, limiter_model
from test_true_peak_host import FLT_MAX

LIMIT_CHUNK = 4096      # GRAIL_LIMIT_CHUNK


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def delay(ell):
    """LAMBDA = GRAIL_LIMIT_STREAM_DELAY(ell)"""
    return (1 << ell) + 10


def known(N, ell):
    """E(N): the outputs that are final after N samples"""
    return max(0, N - delay(ell))


def stream_len(fed_before, n, ell, finishing=False):
    """the count a call writes for a group that was fed fed_before samples before it"""
    if finishing:
        assert n == 0
        return fed_before - known(fed_before, ell)
    return known(fed_before + n, ell) - known(fed_before, ell)


def ring_capacity(ell):
    """the samples of a row's ring: 3 L + 19 rounded up to a power of two"""
    cap = 32
    while cap < 3 * (1 << ell) + 19:
        cap *= 2
    return cap


def nonfinite(x):
    with np.errstate(invalid="ignore"):
        return int(np.count_nonzero(~(np.abs(np.asarray(x, np.float32)) <= FLT_MAX)))


def _stretch(members, c, ell, lo, hi):
    """outputs lo .. hi - 1 of the one-shot model of a group -> ([z per member], min_gain float32, n_limited)"""
    L = 1 << ell
    out, _, _, _, ((q, S, g),) = limiter_model(members, c, ell, group=len(members), curves=True)
    if hi == lo:
        return [np.zeros(0, np.float32) for _ in members], np.float32(1.0), 0
    return [z[lo:hi] for z in out], g[lo:hi].min(), int(np.count_nonzero(S[lo:hi] < L * Q))


def stream_model(members, c, ell, split):
    """members: the float32 rows of one group (equal lengths), all the samples they are fed; split: how many each `next` call
    feeds every member (zeros allowed, sum = the rows' length)
    -> ([([z per member], min_gain, n_limited, nonfinite) per call], ([z per member], min_gain, n_limited) of the tail).
    Every call's outputs come from the one-shot model on the samples fed up to and including that call: later samples cannot
    have changed them.  Asserts, per call, that no sample before N - 3 L - 19 is needed: the same outputs come from the rows
    with everything before it cut away."""
    members = [np.asarray(x, np.float32) for x in members]
    total, L = len(members[0]), 1 << ell
    assert all(len(x) == total for x in members) and sum(split) == total and all(n >= 0 for n in split)
    calls, N = [], 0
    for n in split:
        lo, hi = known(N, ell), known(N + n, ell)
        z, min_gain, n_limited = _stretch([x[:N + n] for x in members], c, ell, lo, hi)
        assert len(z[0]) == stream_len(N, n, ell) <= n
        oldest = max(0, N - 3 * L - 19)
        if hi > lo and oldest > 0:
            cut = _stretch([x[oldest:N + n] for x in members], c, ell, lo - oldest, hi - oldest)
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(z, cut[0])) and cut[1:] == (min_gain, n_limited)
        calls.append((z, min_gain, n_limited, sum(nonfinite(x[N:N + n]) for x in members)))
        N += n
    tail = _stretch(members, c, ell, known(N, ell), N)
    assert len(tail[0][0]) == stream_len(N, 0, ell, finishing=True) == min(N, delay(ell))
    return calls, tail


def combined(calls, tail):
    """what the contract says the per-call results combine to: ([z per member] end to end, min of min_gain, sum of n_limited,
    sum of nonfinite)"""
    parts = [c[0] for c in calls] + [tail[0]]
    joined = [np.concatenate([p[j] for p in parts]) for j in range(len(tail[0]))]
    return (joined, min([c[1] for c in calls] + [tail[1]]), sum(c[2] for c in calls) + tail[2], sum(c[3] for c in calls))


def check_against_one_shot(members, c, ell, split):
    """stream_model's calls and tail concatenate to the one-shot result and their results combine to its results -> them"""
    calls, tail = stream_model(members, c, ell, split)
    joined, min_gain, n_limited, bad = combined(calls, tail)
    out, g1, l1, b1 = limiter_model(members, c, ell, group=len(members))
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(joined, out)), (ell, split)
    assert bits(min_gain) == bits(g1[0]) and n_limited == l1[0] and bad == b1[0], (ell, split)
    return calls, tail


def splits(N, L, rng):
    """the issue's splits of N samples: all at once; [1, LAMBDA, LAMBDA + 1, 0, rest]; cuts one sample either side of a chunk
    of GRAIL_LIMIT_CHUNK outputs; a seeded random split with zeros.  Parts that do not fit are cut to what is left, so every
    split sums to N."""
    def fit(parts):
        out, left = [], N
        for p in parts:
            p = min(p, left)
            out.append(p)
            left -= p
        return out + [left]

    lam = L + 10
    random = []
    left = N
    while left:
        p = 0 if rng.random() < 0.25 else int(min(left, rng.integers(1, max(2, N // 3 + 1))))
        random.append(p)
        left -= p
    # the first call of the third writes LIMIT_CHUNK - 1 outputs and the second takes the stream one output past the chunk;
    # the first call of the fourth writes LIMIT_CHUNK + 1
    return [[N], fit([1, lam, lam + 1, 0]), fit([LIMIT_CHUNK + lam - 1, 2]), fit([LIMIT_CHUNK + lam + 1]), random + [0]]
