"""The resampling contract (include/grail_hip.h, "levels, continued: sample-rate conversion") in numpy's binary64, as the
header states it: v[t] = (double)x[t] for 0 <= t < n and +0.0 outside, a non-finite sample counted once and entering as
+0.0; n_out = min(ceil(n U / D), out_stride); for output m: a = m D, p = a mod U, i0 = a div U, acc = +0.0, for k = 0 ..
P - 1 ascending acc = acc + C[p][k] * v[i0 + P/2 - k], y[m] = (float)acc; C[p][k] = N / 2^26 with N the library's table."""
import numpy as np


def resample_model(x, num, down, out_stride=None, m_lo=0, m_hi=None):
    """x float32[n], num int32[U, P] (grail_resample_coefficients) -> (y[m_lo:m_hi] float32, n_out, nonfinite); any range of
    m is computed without the outputs before it"""
    x = np.asarray(x, np.float32)
    (U, P), D, n = num.shape, int(down), len(x)
    n_out = -(-n * U // D) if out_stride is None else min(-(-n * U // D), int(out_stride))
    m = np.arange(m_lo, n_out if m_hi is None else min(m_hi, n_out), dtype=np.int64)
    finite = np.isfinite(x)
    if n == 0 or len(m) == 0:
        return np.zeros(0, np.float32), n_out, int(n - finite.sum())
    C = num.astype(np.float64) / 2.0 ** 26
    a = m * D
    p, i0 = a % U, a // U
    acc = np.zeros(len(m), np.float64)
    for k in range(P):
        t = i0 + P // 2 - k
        tc = np.clip(t, 0, n - 1)
        v = np.where((t >= 0) & (t < n) & finite[tc], x[tc], np.float32(0.0)).astype(np.float64)
        acc = acc + C[p, k] * v
    return acc.astype(np.float32), n_out, int(n - finite.sum())
