"""The contract of meter streams (include/grail_hip.h, "levels, continued: the meters on streams") in numpy and Python floats,
beside the one-shot models of tests/test_loudness_host.py (kweight_hops_model, gate_model) and tests/test_true_peak_host.py
(true_peak_model): a row's state is carried from call to call (N, s1 .. s4, acc, the running peak, the ledger, the last eleven
samples), every call gives what the header says it gives, and check_against_one_shot holds every clause of THE CONTRACT
between the two.  All counts are Python integers: no width to overflow."""
import math

import numpy as np

from test_loudness_host import _clean, gate_model, kweight_hops_model
from test_true_peak_host import TAPS, true_peak_model

REFUSED = 0xFFFFFFFF
TAIL = 11               # the outputs after a row's last sample: taps - 1


def bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def hops_of_call(fed_before, n, H):
    """grail_meter_stream_hops in integers"""
    return (fed_before + n) // H - fed_before // H


def momentary_model(hops, H):
    """the gate's last z_j: +0.0 below four hops"""
    h = [float(v) for v in hops]
    if len(h) < 4:
        return 0.0
    j = len(h) - 4
    return (((h[j] + h[j + 1]) + h[j + 2]) + h[j + 3]) / (4.0 * H)


def short_term_model(hops, H):
    """the left fold of the last 30 hops from the oldest over (30.0 * H): +0.0 below 30 hops"""
    h = [float(v) for v in hops]
    if len(h) < 30:
        return 0.0
    s = h[len(h) - 30]
    for v in h[len(h) - 29:]:
        s = s + v
    return s / (30.0 * H)


def peak_of_outputs(history, v):
    """the largest |y[p][t]| over the len(v) output times whose newest samples are v (binary64), `history` the eleven samples
    before them: the header's left fold over ascending k from +0.0, vectorised over t as true_peak_model is"""
    n = len(v)
    if n == 0:
        return 0.0
    padded = np.concatenate([np.asarray(history, np.float64), np.asarray(v, np.float64)])
    assert len(padded) == n + TAIL
    best = 0.0
    for p in range(4):
        acc = np.zeros(n)
        for k in range(12):
            acc = acc + TAPS[p, k] * padded[TAIL - k:TAIL - k + n]
        best = max(best, float(np.abs(acc).max()))
    return best


class RowModel:
    """one row of a meter stream"""

    def __init__(self, rate, coef, max_hops=None):
        self.H = int(rate) // 10
        self.coef = [float(c) for c in coef]
        self.max_hops = max_hops
        self.N = 0
        self.ended = False
        self.s = [0.0, 0.0, 0.0, 0.0]
        self.acc = 0.0
        self.peak = 0.0
        self.ledger = []
        self.history = [0.0] * TAIL         # the last eleven samples fed, +0.0 where they were not finite (and before the row)

    def next(self, chunk):
        """-> (the hop sums the call completes float64 [n_hops], true_peak, nonfinite), or None: refused, nothing changed"""
        chunk = np.asarray(chunk, np.float32)
        n = len(chunk)
        new_hops = hops_of_call(self.N, n, self.H)
        if (self.ended and n) or (self.max_hops is not None and len(self.ledger) + new_hops > self.max_hops):
            return None
        if self.ended:
            return np.zeros(0), 0.0, 0
        v, bad = _clean(chunk)
        b0, b1, b2, a1, a2, d0, d1, d2, e1, e2 = self.coef
        s1, s2, s3, s4 = self.s
        acc, pos, done = self.acc, self.N % self.H, []
        for x in v.tolist():
            y = b0 * x + s1
            s1 = (b1 * x - a1 * y) + s2
            s2 = b2 * x - a2 * y
            z = d0 * y + s3
            s3 = (d1 * y - e1 * z) + s4
            s4 = d2 * y - e2 * z
            acc = acc + z * z
            pos += 1
            if pos == self.H:
                done.append(acc)
                acc, pos = 0.0, 0
        assert len(done) == new_hops
        self.s, self.acc = [s1, s2, s3, s4], acc
        peak = peak_of_outputs(self.history, v)
        self.history = (self.history + v.tolist())[-TAIL:]
        self.peak = max(self.peak, peak)
        self.ledger += done
        self.N += n
        return np.array(done, np.float64), peak, bad

    def finish(self):
        """-> the largest of the eleven outputs after the row's last sample; +0.0 for a row that had ended"""
        if self.ended:
            return 0.0
        peak = peak_of_outputs(self.history, np.zeros(TAIL))
        self.peak = max(self.peak, peak)
        self.ended = True
        return peak

    def read(self):
        """-> (integrated_ms, momentary_ms, short_term_ms, true_peak, hops)"""
        return (float(gate_model(self.ledger, self.H)), momentary_model(self.ledger, self.H), short_term_model(self.ledger, self.H),
                self.peak, len(self.ledger))


def same_read(a, b):
    return all(bits(x) == bits(y) for x, y in zip(a[:4], b[:4])) and int(a[4]) == int(b[4])


def stream_model(row, split, rate, coef, max_hops=None):
    """row fed as `split` says (zeros allowed, sum = len(row)), then finished
    -> ([(hops, true_peak, nonfinite) per call], [read after each call], the finish's true_peak, the read after it)"""
    row = np.asarray(row, np.float32)
    assert sum(split) == len(row) and all(n >= 0 for n in split)
    m = RowModel(rate, coef, max_hops)
    calls, reads, at = [], [], 0
    for n in split:
        calls.append(m.next(row[at:at + n]))
        assert calls[-1] is not None
        reads.append(m.read())
        at += n
    tail = m.finish()
    return calls, reads, tail, m.read()


def check_against_one_shot(row, split, rate, coef):
    """every clause of THE CONTRACT between stream_model and the one-shot models -> stream_model's result"""
    row = np.asarray(row, np.float32)
    H = int(rate) // 10
    calls, reads, tail, last = stream_model(row, split, rate, coef)
    (hops, bad), = kweight_hops_model([row], rate, coef)
    joined = np.concatenate([c[0] for c in calls] + [np.zeros(0)])
    assert np.array_equal(bits(joined), bits(hops)), ("hops end to end", split)
    peak, bad_tp = true_peak_model(row)
    assert bits(max([c[1] for c in calls] + [tail])) == bits(peak), ("the largest of the true peaks", split)
    assert sum(c[2] for c in calls) == bad == bad_tp, ("the counts", split)
    N = 0
    for k, (n, c, r) in enumerate(zip(split, calls, reads)):
        assert len(c[0]) == hops_of_call(N, n, H)
        N += n
        # a row that holds exactly the N samples fed so far: its hops are the whole row's first N // H (the filter is causal)
        prefix = hops[:N // H]
        want = (float(gate_model(prefix, H)), momentary_model(prefix, H), short_term_model(prefix, H))
        assert all(bits(a) == bits(b) for a, b in zip(r[:3], want)) and r[4] == N // H, ("read", split, k)
        # the running peak before `finish`: the one-shot number of the prefix without the eleven outputs after its last sample
        assert bits(r[3]) == bits(peak_of_outputs(np.zeros(TAIL), _clean(row[:N])[0])), ("running peak", split, k)
        if n == 0:
            assert len(c[0]) == 0 and bits(c[1]) == bits(0.0) and c[2] == 0
    assert bits(last[3]) == bits(peak) and last[4] == len(row) // H
    assert not math.isnan(last[0])
    return calls, reads, tail, last


def random_split(N, rng, zeros=0.25, most=None):
    """a seeded split of N samples with calls of no samples"""
    out, left = [], N
    most = most or max(2, N // 3 + 1)
    while left:
        p = 0 if rng.random() < zeros else int(min(left, rng.integers(1, most)))
        out.append(p)
        left -= p
    return out + [0]
