"""Sample-rate conversion (include/grail_hip.h, "levels, continued: sample-rate conversion") without a GPU: the ratio and
the taps against the header's formula, the lengths against integer arithmetic, the properties of the table the library
returns (bounds, exact evenness, phase sums, stopband, ripple), the numpy model of tests/resample_model.py against known
answers (which pins the index convention that tests/test_resample_gpu.py holds the device to), and the argument errors
of grail_resample_async, which come before the device is asked for."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import grail_hip as G
from resample_model import resample_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = [8000, 11025, 16000, 22050, 24000, 44100, 48000, 96000]
TABLE_PAIRS = [(48000, 16000), (48000, 8000), (44100, 48000), (48000, 44100), (44100, 16000), (48000, 96000), (48000, 22050),
               (44100, 8000)]
Z = 24


def formula(rate_in, rate_out):
    g = math.gcd(rate_in, rate_out)
    U, D = rate_out // g, rate_in // g
    return U, D, 2 * -(-Z * max(U, D) // U)


@pytest.fixture(scope="module")
def tables(built):
    return {pair: G.resample_coefficients(*pair) for pair in TABLE_PAIRS}


# ---- the ratio, the taps, the lengths ---------------------------------------------------------------------------------------
def test_ratio_matches_the_formula(built):
    assert G.RESAMPLE_ZERO_CROSSINGS == Z and G.RESAMPLE_TABLE_MAX == 32768
    # every pair of the common rates fits the table but 11 025 <-> 96 000 (61 440 and 61 446 entries)
    pairs = TABLE_PAIRS + [(a, b) for a in RATES for b in RATES if a != b and {a, b} != {11025, 96000}] + [(2, 3), (3, 2), (5, 7)]
    for pair in pairs:
        U, D, P = formula(*pair)
        assert U * P <= G.RESAMPLE_TABLE_MAX, pair
        assert G.resample_ratio(*pair) == (U, D, P), pair
    assert formula(11025, 96000) == (1280, 147, 48) and formula(96000, 11025) == (147, 1280, 418)
    for pair in [(11025, 96000), (96000, 11025)]:
        with pytest.raises(G.GrailError):
            G.resample_ratio(*pair)
    assert G.resample_ratio(44100, 16000) == (160, 441, 134) and 160 * 134 == 21440
    assert G.resample_ratio(48000, 11025) == (147, 640, 210) and 147 * 210 == 30870
    assert G.resample_ratio(2, 3) == (3, 2, 48) and G.resample_ratio(3, 2) == (2, 3, 72)


def test_ratio_refuses_equal_rates_a_zero_rate_and_a_table_over_the_limit(built):
    lib = G.load()
    assert formula(48000, 44101)[0] * formula(48000, 44101)[2] > G.RESAMPLE_TABLE_MAX
    for pair in [(48000, 48000), (1, 1), (0, 48000), (48000, 0), (0, 0), (48000, 44101), (44101, 48000), (0xFFFFFFFF, 0xFFFFFFFE)]:
        u = (C.c_uint32 * 3)(7, 7, 7)
        a = C.addressof(u)
        assert lib.grail_resample_ratio(pair[0], pair[1], a, a + 4, a + 8) == G.ERR_INVALID_ARG, pair
        assert list(u) == [7, 7, 7]
        with pytest.raises(G.GrailError):
            G.resample_coefficients(*pair)
        with pytest.raises(G.GrailError):
            G.resample_len(100, *pair)
    assert lib.grail_resample_ratio(48000, 16000, None, None, None) == G.OK
    # a table one entry short, and no table at all
    num = np.full(144, 77, np.int32)
    assert lib.grail_resample_coefficients(48000, 16000, num.ctypes.data, 143) == G.ERR_INVALID_ARG and np.all(num == 77)
    assert lib.grail_resample_coefficients(48000, 16000, None, 144) == G.ERR_INVALID_ARG
    assert lib.grail_resample_coefficients(48000, 16000, num.ctypes.data, 144) == G.OK and num[72] == round(0.3 * 2 ** 26)


def test_len_matches_integer_arithmetic(built):
    for pair in [(44100, 16000), (16000, 44100), (48000, 16000), (2, 3), (3, 2), (48000, 96000)]:
        U, D, _ = formula(*pair)
        for n in [0, 1, 2, D - 1, D, D + 1, 441 * 7, 2 ** 31 - 1, 2 ** 32 - 2, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 40 + 12345,
                  2 ** 56 + 1]:
            assert G.resample_len(n, *pair) == -(-n * U // D), (pair, n)
    assert G.resample_len(2 ** 32 - 1, 44100, 16000) == -(-(2 ** 32 - 1) * 160 // 441)
    assert G.resample_len(2 ** 64 - 1, 48000, 16000) == -(-(2 ** 64 - 1) // 3)
    with pytest.raises(G.GrailError):
        G.resample_len(2 ** 63, 16000, 48000)           # three times 2^63 does not fit
    assert G.load().grail_resample_len(1, 48000, 16000, None) == G.ERR_INVALID_ARG


# ---- the table ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", TABLE_PAIRS)
def test_table_bounds_evenness_and_phase_sums(tables, pair):
    num = tables[pair]
    U, D, P = formula(*pair)
    assert num.shape == (U, P) and num.dtype == np.int32
    assert np.abs(num.astype(np.int64)).max() < 2 ** 26
    proto = num.T.reshape(-1).astype(np.int64)          # N(j) at index j + (P/2) U
    mid = P // 2 * U
    assert abs(proto[mid] - 0.9 * min(1.0, U / D) * 2 ** 26) <= 0.501           # N(0) = f 2^26, rounded
    # N(j) = N(-j) for every j that has a mirror (j = -(P/2) U has none)
    assert np.array_equal(proto[mid + 1:], proto[mid - 1:0:-1]) and len(proto[mid + 1:]) == mid - 1
    sums = num.astype(np.float64).sum(axis=1) / 2.0 ** 26
    assert np.abs(sums - 1.0).max() <= 1e-4, np.abs(sums - 1.0).max()


@pytest.mark.parametrize("pair", TABLE_PAIRS)
def test_table_stopband_and_ripple(tables, pair):
    num = tables[pair]
    U, D, P = formula(*pair)
    points = 1 << 20
    proto = num.T.reshape(-1).astype(np.float64) / 2.0 ** 26
    mag = np.abs(np.fft.rfft(proto, points))
    rel_db = 20.0 * np.log10(np.maximum(mag, 1e-300) / mag[0])
    nyquist = 0.5 / max(U, D) * points                  # the lower Nyquist frequency in bins of the prototype's rate
    bins = np.arange(len(mag))
    stop = rel_db[bins >= 1.01 * nyquist]
    passband = rel_db[bins <= 0.78 * nyquist]
    print(f"{pair}: stopband {stop.max():.2f} dB, ripple {np.abs(passband).max():.5f} dB")
    assert len(stop) > 1000 and len(passband) > 300
    assert stop.max() <= -78.0, stop.max()
    assert np.abs(passband).max() <= 0.01, np.abs(passband).max()


# ---- the model: the index convention -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", [(48000, 16000), (44100, 48000), (2, 3), (3, 2), (44100, 16000)])
def test_model_impulse_gives_the_table_column(built, pair):
    num = G.resample_coefficients(*pair)
    U, D, P = formula(*pair)
    n = 3 * P + 11
    for t0 in (0, 1, P // 2, n // 2, n - 1):
        x = np.zeros(n, np.float32)
        x[t0] = 1.0
        y, n_out, bad = resample_model(x, num, D)
        assert n_out == len(y) == -(-n * U // D) and bad == 0
        m = np.arange(n_out)
        p, i0 = (m * D) % U, (m * D) // U
        k = i0 + P // 2 - t0
        want = np.where((k >= 0) & (k < P), num[p, np.clip(k, 0, P - 1)].astype(np.float64) / 2.0 ** 26, 0.0).astype(np.float32)
        assert np.array_equal(y.view(np.uint32), want.view(np.uint32)), (pair, t0)
        assert np.count_nonzero(y) > P * U // D // 4


@pytest.mark.parametrize("pair", [(48000, 16000), (44100, 48000), (48000, 44100), (2, 3)])
def test_model_dc_and_ranges_and_nonfinite(built, pair):
    num = G.resample_coefficients(*pair)
    U, D, P = formula(*pair)
    n = 6 * P
    y, n_out, _ = resample_model(np.ones(n, np.float32), num, D)
    edge = -(-(P // 2 + 1) * U // D) + 1                  # outputs whose taps reach outside the row
    assert np.abs(y[edge:n_out - edge].astype(np.float64) - 1.0).max() <= 1e-4 and n_out - 2 * edge > 10
    # any range of m without the ones before; the clamp is a prefix; a non-finite sample is counted and enters as +0.0
    x = np.random.default_rng(5).uniform(-1, 1, n).astype(np.float32)
    full, _, _ = resample_model(x, num, D)
    part, _, _ = resample_model(x, num, D, m_lo=17, m_hi=91)
    assert np.array_equal(part.view(np.uint32), full[17:91].view(np.uint32))
    cut, cut_len, _ = resample_model(x, num, D, out_stride=40)
    assert cut_len == 40 and np.array_equal(cut.view(np.uint32), full[:40].view(np.uint32))
    holes = x.copy()
    holes[[0, n // 2, n - 1]] = [np.nan, np.inf, -np.inf]
    zeroed = x.copy()
    zeroed[[0, n // 2, n - 1]] = 0.0
    a, _, bad = resample_model(holes, num, D)
    b, _, none = resample_model(zeroed, num, D)
    assert bad == 3 and none == 0 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert resample_model(np.zeros(0, np.float32), num, D)[1:] == (0, 0)


def test_model_tones_48000_to_16000(built):
    num = G.resample_coefficients(48000, 16000)
    n = 48000 // 4
    t = np.arange(n, dtype=np.float64) / 48000.0
    keep = slice(200, n // 3 - 200 - (n // 3 - 400) % 16)           # whole periods of 1 kHz at 16 kHz, away from the edges
    y, n_out, _ = resample_model(np.sin(2 * np.pi * 1000.0 * t).astype(np.float32), num, 3)
    assert n_out == n // 3
    s = np.arange(n_out, dtype=np.float64)[keep] / 16000.0
    basis = np.stack([np.sin(2 * np.pi * 1000.0 * s), np.cos(2 * np.pi * 1000.0 * s)], axis=1)
    amp = np.hypot(*np.linalg.lstsq(basis, y[keep].astype(np.float64), rcond=None)[0])
    assert abs(20.0 * np.log10(amp)) <= 0.01, 20.0 * np.log10(amp)
    y, _, _ = resample_model(np.sin(2 * np.pi * 9000.0 * t).astype(np.float32), num, 3)
    leak = 20.0 * np.log10(np.abs(y[keep]).max())
    print(f"1 kHz gain {20.0 * np.log10(amp):+.5f} dB, 9 kHz leak {leak:.2f} dB")
    assert leak <= -78.0, leak


# ---- the arguments -------------------------------------------------------------------------------------------------------------
def test_argument_errors_come_before_the_device(built):
    lib = G.load()
    hdr = open(os.path.join(ROOT, "include", "grail_hip.h")).read()
    assert "levels, continued: sample-rate conversion" in hdr and "#define GRAIL_RESAMPLE_CHUNK 1024" in hdr
    assert G.RESAMPLE_CHUNK == 1024
    a, b, ln = 0x10000000, 0x20000000, 0x30000000                   # addresses nobody looks behind: every case returns first
    cases = [
        ((None, a, 64, ln, 1, 48000, 48000, b, 64, None, None), b"rates"),
        ((None, a, 64, ln, 1, 0, 16000, b, 64, None, None), b"rates"),
        ((None, a, 64, ln, 1, 48000, 44101, b, 64, None, None), b"rates"),
        ((None, a, 64, ln, 0, 48000, 48000, b, 64, None, None), b"rates"),           # (also with no rows)
        ((None, a, 64, None, 1, 48000, 16000, b, 64, None, None), b"NULL buffer"),
        ((None, None, 64, ln, 1, 48000, 16000, b, 64, None, None), b"NULL buffer"),
        ((None, a, 64, ln, 1, 48000, 16000, None, 64, None, None), b"NULL buffer"),
        ((None, a, 64, ln, 2, 48000, 16000, a + 4 * 64, 64, None, None), b"overlaps"),
        ((None, a, 64, ln, 2, 48000, 16000, a - 4 * 32 * 2 + 4, 32, None, None), b"overlaps"),
        ((None, a, 64, ln, 1, 48000, 16000, a, 64, None, None), b"overlaps"),
        ((None, a, 2 ** 33, ln, 1, 16000, 48000, 2 ** 50, 2 ** 34, None, None), b"2^32"),
    ]
    for args, word in cases:
        assert lib.grail_resample_async(*args) == G.ERR_INVALID_ARG, args
        assert word in lib.grail_last_error(), (args, lib.grail_last_error())
    if G.device_count() == 0:        # no context can exist: the valid call says why, it does not compute on the CPU
        assert lib.grail_resample_async(None, a, 64, ln, 2, 48000, 16000, a + 4 * 128, 64, None, None) == G.ERR_NO_DEVICE
        assert b"no usable HIP device" in lib.grail_last_error()
        assert lib.grail_resample_async(None, None, 0, None, 0, 48000, 16000, None, 0, None, None) == G.ERR_NO_DEVICE


def test_dialogue_example_knows_the_rate_option(built):
    exe = os.path.join(ROOT, "grail-rs_amd", "lib", "grail_dialogue")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "[--rate R]" in r.stderr
    for bad in ("fast", "0", "-16000", "16000.5", "4294967296"):
        r = subprocess.run([exe, "--rate", bad, "a", "e"], capture_output=True, text=True)
        assert r.returncode == 2 and "usage" in r.stderr, bad
    if G.device_count() == 0:
        r = subprocess.run([exe, "-o", os.devnull, "--rate", "16000", "a", "e"], capture_output=True, text=True)
        assert r.returncode == 1 and "no HIP device" in r.stderr
