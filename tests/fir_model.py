"""The FIR contract of include/grail_hip.h ("levels, continued: FIR filtering") in numpy: a loop over the taps, vectorised
over the outputs, every step acc = acc + (double)h[k] * v[m + o - k] in binary64, one rounding to binary32 at the end."""
import numpy as np


def fir_model(x, h, origin, out_stride=None, m_lo=0, m_hi=None):
    """x: the row's samples (float32), h: the taps (float32), origin: o -> (y float32[m_lo .. min(m_hi, n_out)), n_out,
    nonfinite).  out_stride clamps n_out; the count is that of the whole row whatever is cut."""
    x = np.asarray(x, np.float32)
    h = np.asarray(h, np.float32)
    n, K = len(x), len(h)
    assert 1 <= K and 0 <= origin <= K - 1
    finite = np.isfinite(x)
    bad = int(n - np.count_nonzero(finite))
    n_out = 0 if n == 0 else n + K - 1 - origin
    if out_stride is not None:
        n_out = min(n_out, out_stride)
    m_hi = n_out if m_hi is None else min(m_hi, n_out)
    m_lo = min(m_lo, m_hi)
    v = np.zeros(n + 2 * K, np.float64)             # v[t] lies at index t + K: +0.0 outside the row and where not finite
    v[K:K + n] = np.where(finite, x, np.float32(0.0)).astype(np.float64)
    acc = np.zeros(m_hi - m_lo, np.float64)
    for k in range(K):
        at = K + m_lo + origin - k
        acc = acc + np.float64(h[k]) * v[at:at + m_hi - m_lo]
    with np.errstate(over="ignore"):
        return acc.astype(np.float32), n_out, bad


def cancelling_taps(K, rng):
    """h[0] = 2^30, h[K - 1] = -2^30, the rest uniform in +-1: over steps of equal samples the two large products cancel,
    and what the small ones left behind in the low bits depends on the order they were added in"""
    h = rng.uniform(-1.0, 1.0, K).astype(np.float32)
    h[0] = np.float32(2.0 ** 30)
    h[K - 1] = np.float32(-2.0 ** 30)
    return h


def steps(n, rng):
    """the "cancelling" content: steps of 100 equal samples"""
    return np.repeat(rng.uniform(-1.0, 1.0, n // 100 + 1).astype(np.float32), 100)[:n]
