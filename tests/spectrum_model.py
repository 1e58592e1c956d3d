"""The contract of short-time spectra (include/grail_spectrum.h, "levels, continued: short-time spectra") in numpy: the twiddle
table, the frames, the radix-2 stages with one ufunc per operation, the power and the bands.  numpy's float64 is IEEE
binary64, every ufunc rounds by itself and nothing is fused: the operations below are the header's, in the header's order,
vectorised over frames and over the butterflies of a stage (which do not depend on each other).  The designers' cos, sin,
log10 and pow are Python's math module's, which are the C library's: numpy's own may differ from them in the last bit."""
import math

import numpy as np

FLT_MAX = np.float32(3.4028234663852886e38)
LOG2_MIN, LOG2_MAX, BANDS_MAX, WEIGHTS_MAX, CHUNK_FRAMES = 6, 12, 256, 65536, 8
RECT, HANN, HAMMING = 0, 1, 2
TWO_PI = 2.0 * math.pi


def twiddles(p):
    """T as complex-free float64 [N/2][2] = (re, im)"""
    N = 1 << p
    Q = N // 4
    T = np.zeros((N // 2, 2), np.float64)
    for j in range(Q + 1):
        if j == 0:
            c, s = 1.0, 0.0
        elif j == Q:
            c, s = 0.0, 1.0
        else:
            x = (TWO_PI * float(j)) / float(N)
            c, s = math.cos(x), math.sin(x)
        T[j] = (c, 0.0 - s)
        if 1 <= j < Q:
            T[N // 2 - j] = (0.0 - c, 0.0 - s)
    return T


def frames(n, hop):
    return (n + hop - 1) // hop


def window(kind, W):
    if kind == RECT:
        return np.ones(W, np.float32)
    a = 0.5 if kind == HANN else 0.54
    return np.array([np.float32(a - (1.0 - a) * math.cos((TWO_PI * float(j)) / float(W))) for j in range(W)], np.float32)


def mel_design(rate, p, B, lo_hz, hi_hz):
    """(first uint32 [B], count uint32 [B], weights float32 [sum of the counts])"""
    N = 1 << p

    def mel_of(f):
        return 2595.0 * math.log10(1.0 + f / 700.0)

    def hz_of(m):
        return 700.0 * (math.pow(10.0, m / 2595.0) - 1.0)

    m_lo, m_hi = mel_of(lo_hz), mel_of(hi_hz)
    pts = [hz_of(m_lo + ((m_hi - m_lo) * float(i)) / float(B + 1)) for i in range(B + 2)]
    first, count, weights = [], [], []
    for b in range(B):
        l, c, r = pts[b], pts[b + 1], pts[b + 2]
        row = []
        for k in range(N // 2 + 1):
            f = (float(k) * float(rate)) / float(N)
            row.append(np.float32(max(0.0, min((f - l) / (c - l), (r - f) / (r - c)))))
        above = [k for k, w in enumerate(row) if w > 0]
        first.append(above[0] if above else 0)
        count.append(above[-1] - above[0] + 1 if above else 0)
        weights += row[first[-1]:first[-1] + count[-1]]
    return np.array(first, np.uint32), np.array(count, np.uint32), np.array(weights, np.float32)


def clean(x):
    """(the samples as binary64 with +0.0 in place of the non-finite ones, the count of those)"""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        finite = np.abs(x) <= FLT_MAX
    return np.where(finite, x, np.float32(0.0)).astype(np.float64), int(np.count_nonzero(~finite))


def bit_reverse(p):
    return np.array([int(format(j, "0%db" % p)[::-1], 2) for j in range(1 << p)], np.int64)


def transform(a, p, T=None):
    """the stages on a float64 [F][N] of real frames -> (re, im) float64 [F][N]"""
    N = 1 << p
    T = twiddles(p) if T is None else T
    F = a.shape[0]
    re, im = np.zeros((F, N), np.float64), np.zeros((F, N), np.float64)
    re[:, bit_reverse(p)] = a                       # A[rev(j)] = (a[j], +0.0)
    for s in range(1, p + 1):
        M, h = 1 << s, 1 << (s - 1)
        w = T[np.arange(h) * (N // M)]
        wr, wi = w[:, 0], w[:, 1]
        re4, im4 = re.reshape(F, N // M, 2, h), im.reshape(F, N // M, 2, h)
        ur, ui, vr, vi = re4[:, :, 0, :], im4[:, :, 0, :], re4[:, :, 1, :], im4[:, :, 1, :]
        tr = (vr * wr) - (vi * wi)
        ti = (vr * wi) + (vi * wr)
        nr, ni = np.empty_like(re4), np.empty_like(im4)
        nr[:, :, 0, :], ni[:, :, 0, :] = ur + tr, ui + ti
        nr[:, :, 1, :], ni[:, :, 1, :] = ur - tr, ui - ti
        re, im = nr.reshape(F, N), ni.reshape(F, N)
    return re, im


def row_frames(x, n, p, w, hop, pad):
    """a[f][j] float64 [n_frames][N] of the row's first n samples (cleaned), and the count of its non-finite ones"""
    N, W = 1 << p, len(w)
    v, bad = clean(np.asarray(x, np.float32)[:n])
    F = frames(n, hop)
    t = np.arange(F)[:, None] * hop - pad + np.arange(W)[None, :]
    inside = (t >= 0) & (t < n)
    vv = np.where(inside, v[np.clip(t, 0, max(n - 1, 0))] if n else 0.0, 0.0)
    a = np.zeros((F, N), np.float64)
    a[:, :W] = np.asarray(w, np.float32).astype(np.float64)[None, :] * vv
    return a, bad


def power_of(re, im, p):
    half = (1 << p) // 2 + 1
    return (re[:, :half] * re[:, :half]) + (im[:, :half] * im[:, :half])


def bands_of(P, first, count, weights):
    """e float64 [F][B]: the left folds from +0.0 in ascending k, the product rounded, then the sum"""
    F, B = P.shape[0], len(first)
    e = np.zeros((F, B), np.float64)
    at = 0
    for b in range(B):
        acc = np.zeros(F, np.float64)
        for k in range(int(count[b])):
            acc = acc + (np.float64(weights[at + k]) * P[:, int(first[b]) + k])
        e[:, b] = acc
        at += int(count[b])
    return e


def spectrum_model(rows, p, w, hop, pad, first=(), count=(), weights=()):
    """rows: a list of float32 arrays (a row's own samples) -> per row (power float32 [n_frames][N/2+1], bands float32
    [n_frames][B], n_frames, nonfinite).  The conversion to float32 is numpy's, round to nearest even, overflow to inf."""
    T = twiddles(p)
    out = []
    for x in rows:
        a, bad = row_frames(x, len(x), p, w, hop, pad)
        re, im = transform(a, p, T)
        P = power_of(re, im, p)
        with np.errstate(over="ignore"):
            out.append((P.astype(np.float32), bands_of(P, first, count, weights).astype(np.float32), a.shape[0], bad))
    return out
