"""FIR filtering (include/grail_hip.h, "levels, continued: FIR filtering") without a GPU: the numpy model of
tests/fir_model.py against known answers (which pins the index convention that tests/test_fir_gpu.py holds the device to),
the order of the fold showing in the bits, the argument that lets the kernel pad the taps with +0.0, grail_fir_design
against its formula and the response of the table it returns, grail_fir_len, and the argument errors, which come before
the device is asked for."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import grail_hip as G
from fir_model import cancelling_taps, fir_model, steps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ["grail_fir_async", "grail_fir_create", "grail_fir_design", "grail_fir_free", "grail_fir_len"]
DESIGNS = [(8000, 300.0, 3400.0, 255), (48000, 300.0, 3400.0, 1023), (48000, 0.0, 8000.0, 255), (48000, 100.0, 24000.0, 1023)]


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


# ---- the model ------------------------------------------------------------------------------------------------------------------
def test_model_one_tap_of_one_copies_all_but_minus_zero_and_non_finite_samples(built):
    rng = np.random.default_rng(1)
    x = rng.uniform(-1, 1, 300).astype(np.float32)
    x[5], x[17], x[40], x[41], x[299] = -0.0, np.nan, np.inf, -np.inf, np.float32(1e-42)
    y, n_out, bad = fir_model(x, [1.0], 0)
    assert (n_out, bad) == (300, 3)
    want = x.copy()
    want[[5, 17, 40, 41]] = 0.0                     # +0.0, also where the sample was -0.0
    assert np.array_equal(bits(y), bits(want)) and bits(y)[5] == 0 and y[299] == x[299]
    assert fir_model(np.zeros(0, np.float32), [1.0], 0)[1:] == (0, 0)


def test_model_shifting_the_origin_shifts_the_output(built):
    rng = np.random.default_rng(2)
    x, h = rng.uniform(-1, 1, 500).astype(np.float32), rng.uniform(-1, 1, 33).astype(np.float32)
    causal, n0, _ = fir_model(x, h, 0)
    assert n0 == 532
    for o in (1, 16, 32):
        y, n_out, _ = fir_model(x, h, o)
        assert n_out == 532 - o and np.array_equal(bits(y), bits(causal[o:]))
    # an impulse at t0 gives the taps, tap o at t0
    for t0 in (0, 7, 499):
        d = np.zeros(500, np.float32)
        d[t0] = 1.0
        y, _, _ = fir_model(d, h, 16)
        want = np.zeros(516, np.float32)
        lo = t0 - 16
        want[max(lo, 0):lo + 33] = h[max(-lo, 0):]
        assert np.array_equal(bits(y), bits(want)), t0
    # a range of m, and the clamp, are the same samples
    part, _, _ = fir_model(x, h, 16, m_lo=17, m_hi=91)
    full, _, _ = fir_model(x, h, 16)
    cut, cut_len, bad = fir_model(np.r_[x, np.float32(np.nan)], h, 16, out_stride=40)
    assert np.array_equal(bits(part), bits(full[17:91])) and cut_len == 40 and bad == 1 and np.array_equal(bits(cut), bits(full[:40]))


def test_len_agrees_with_the_models_formula(built):
    assert (G.FIR_TAPS_MAX, G.FIR_FILTERS_MAX, G.FIR_CHUNK) == (4096, 64, 2048)
    for K, o in [(1, 0), (2, 1), (9, 4), (255, 127), (255, 0), (4096, 4095), (4096, 0)]:
        for n in [0, 1, 2, 2047, 2 ** 32 - 1, 2 ** 40 + 3, 2 ** 64 - 1 - (K - 1 - o)]:
            assert G.fir_len(n, K, o) == (0 if n == 0 else n + K - 1 - o), (K, o, n)
        assert fir_model(np.ones(7, np.float32), np.ones(K, np.float32), o)[1] == G.fir_len(7, K, o)
    lib = G.load()
    out = C.c_uint64(77)
    for n, K, o in [(5, 0, 0), (5, 4097, 0), (5, 9, 9), (5, 1, 1), (2 ** 64 - 1, 2, 0), (2 ** 64 - 4095, 4096, 0)]:
        assert lib.grail_fir_len(n, K, o, C.addressof(out)) == G.ERR_INVALID_ARG and out.value == 77, (n, K, o)
    assert lib.grail_fir_len(5, 9, 4, None) == G.ERR_INVALID_ARG


def test_the_order_of_the_fold_shows_in_the_bits(built):
    """the "cancelling" content: a fold in two chains (even taps, odd taps, then their sum) differs from the contract's one
    chain in more than 5 % of the outputs; so would numpy's own convolution.  A kernel that reorders the sum cannot pass
    tests/test_fir_gpu.py by luck."""
    rng = np.random.default_rng(3)
    n, K = 5000, 64
    h, x = cancelling_taps(K, rng), steps(n, rng)
    y, n_out, _ = fir_model(x, h, 0)
    assert n_out == n + K - 1
    v = np.zeros(n + 2 * K, np.float64)
    v[K:K + n] = x
    chains = [np.zeros(n_out), np.zeros(n_out)]
    for k in range(K):
        chains[k & 1] = chains[k & 1] + np.float64(h[k]) * v[K - k:K - k + n_out]
    two = (chains[0] + chains[1]).astype(np.float32)
    conv = np.convolve(x.astype(np.float64), h.astype(np.float64)).astype(np.float32)
    d_two, d_conv = int(np.count_nonzero(bits(two) != bits(y))), int(np.count_nonzero(bits(conv) != bits(y)))
    print(f"\ntwo chains differ in {d_two} of {n_out} outputs, numpy.convolve in {d_conv}")
    assert d_two > 0.05 * n_out
    assert np.abs(two.astype(np.float64) - y).max() <= 1e-6 * np.abs(y).max()       # (the same filter, other roundings)


@pytest.mark.parametrize("K", [1, 7, 9, 64])
def test_padding_the_taps_with_plus_zero_changes_no_bit(built, K):
    """what lets the kernel round the taps up to a multiple of eight: acc is never -0.0, so adding a product of +0.0 (or
    -0.0, where the sample is negative) changes nothing, also with -0.0 among the taps and the samples and rows of zeros"""
    rng = np.random.default_rng(4 + K)
    h = rng.uniform(-1, 1, K).astype(np.float32)
    h[rng.random(K) < 0.3] = np.float32(-0.0)
    padded = np.r_[h, np.zeros(-K % 8 + 8, np.float32)]
    for x in (rng.uniform(-1, 1, 400).astype(np.float32), np.full(400, -0.0, np.float32), -np.abs(rng.uniform(-1, 1, 400)).astype(np.float32)):
        x[rng.random(400) < 0.3] = np.float32(-0.0)
        for o in sorted({0, K - 1}):
            y, n_out, _ = fir_model(x, h, o)
            z, _, _ = fir_model(x, padded, o)
            assert np.array_equal(bits(y), bits(z[:n_out])), (K, o)
            assert not np.any(bits(y) == 0x80000000)                                    # no output is -0.0


# ---- the design -------------------------------------------------------------------------------------------------------------------
def i0_model(y):
    total, t, k = 1.0, 1.0, 1
    while True:
        t = t * (y / 2.0) / float(k)
        nxt = total + t * t
        if nxt == total:
            return total
        total, k = nxt, k + 1


def sinc_model(a):
    return 1.0 if a == 0.0 else math.sin(math.pi * a) / (math.pi * a)


def design_model(rate, lo, hi, K):
    """the header's formula in Python floats (binary64), in the order the header writes it"""
    c = (K - 1) // 2
    W, f_l, f_h, i0_beta = c + 1.0, lo / float(rate), hi / float(rate), i0_model(8.0)
    out = np.zeros(K, np.float64)
    for k in range(K):
        x = float(k - c)
        r = x / W
        window = i0_model(8.0 * math.sqrt(1.0 - r * r)) / i0_beta
        out[k] = window * (2.0 * f_h * sinc_model(2.0 * f_h * x) - 2.0 * f_l * sinc_model(2.0 * f_l * x))
    return out


def response_db(h, rate, points=1 << 18):
    mag = np.abs(np.fft.rfft(np.asarray(h, np.float64), points))
    return np.arange(len(mag)) * (rate / points), 20.0 * np.log10(np.maximum(mag, 1e-300))


@pytest.mark.parametrize("rate,lo,hi,K", DESIGNS)
def test_design_matches_its_formula_and_its_response_holds(built, rate, lo, hi, K):
    h = G.fir_design(rate, lo, hi, K)
    assert h.dtype == np.float32 and len(h) == K and np.all(np.isfinite(h))
    want = design_model(rate, lo, hi, K).astype(np.float32)
    exact = np.array_equal(bits(h), bits(want))
    ulps = np.abs(bits(h).astype(np.int64) - bits(want).astype(np.int64))
    near = np.maximum(np.abs(h.astype(np.float64) - want), 0) <= np.spacing(np.maximum(np.abs(h), np.abs(want)))
    print(f"\n{rate} Hz {lo:g} - {hi:g} Hz, {K} taps: " + ("bit for bit" if exact else f"{int(np.count_nonzero(ulps))} taps differ, all within 1 ulp: {bool(near.all())}"))
    assert exact or bool(near.all())
    assert np.array_equal(bits(h), bits(h[::-1]))                               # linear phase: exactly even about c
    df = (81.3 - 7.95) / (2.285 * 2.0 * math.pi * (K - 1)) * rate
    f, mag = response_db(h, rate)
    passband = mag[(f >= lo + df) & (f <= hi - df)]
    assert len(passband) > 1000
    line = f"passband {passband.min():+.5f} .. {passband.max():+.5f} dB"
    assert np.abs(passband).max() <= 0.001, line
    for name, stop in (("below", mag[f <= lo - df]), ("above", mag[f >= hi + df])):
        if len(stop):
            line += f", stopband {name} {stop.max():.2f} dB"
            assert stop.max() <= -80.0, line
    assert ("below" in line) == (lo - df >= 0) and ("above" in line) == (hi + df <= rate / 2)
    model_f, model_mag = response_db(design_model(rate, lo, hi, K), rate)
    print(f"{line}; rounding the taps to binary32 moves the response by {20 * np.log10(np.abs(10 ** (mag / 20) - 10 ** (model_mag / 20)).max()):.1f} dB re 1")


def test_design_low_pass_high_pass_and_refusals(built):
    # (0 Hz lies in the low-pass's passband, within 0.001 dB of 1, and 240 Hz = df below the high-pass's edge at 1 kHz, at
    # or below -80 dB = 1e-4; the Nyquist frequency is in its passband)
    lp, hp = G.fir_design(48000, 0.0, 8000.0, 255), G.fir_design(48000, 1000.0, 24000.0, 1023)
    assert abs(lp.astype(np.float64).sum() - 1.0) <= 1.2e-4 and abs(hp.astype(np.float64).sum()) <= 1e-4
    alt = (hp.astype(np.float64) * (-1.0) ** np.arange(1023)).sum()                 # the response at Nyquist, up to its sign
    assert abs(abs(alt) - 1.0) <= 1.2e-4                                               # (0.001 dB is 1.15e-4)
    lib = G.load()
    buf = np.full(4096, 77, np.float32)
    nan = float("nan")
    for rate, lo, hi, K in [(0, 0.0, 1.0, 255), (8000, 300.0, 3400.0, 254), (8000, 300.0, 3400.0, 1), (8000, 300.0, 3400.0, 4097),
                            (8000, 300.0, 3400.0, 0), (8000, -1.0, 3400.0, 255), (8000, 3400.0, 3400.0, 255), (8000, 3400.0, 300.0, 255),
                            (8000, 300.0, 4000.5, 255), (8000, nan, 3400.0, 255), (8000, 300.0, nan, 255), (8000, 300.0, float("inf"), 255)]:
        assert lib.grail_fir_design(rate, lo, hi, K, buf.ctypes.data) == G.ERR_INVALID_ARG, (rate, lo, hi, K)
        assert np.all(buf == 77)
    assert lib.grail_fir_design(8000, 300.0, 3400.0, 255, None) == G.ERR_INVALID_ARG
    assert lib.grail_fir_design(8000, 0.0, 4000.0, 4095, buf.ctypes.data) == G.OK and buf[4095] == 77 and buf[2047] == 1.0


# ---- the arguments -------------------------------------------------------------------------------------------------------------
def test_argument_errors_come_before_the_device(built):
    lib = G.load()
    taps = np.linspace(-1, 1, 4200).astype(np.float32)
    out = C.c_void_p(0x77)
    po = C.addressof(out)

    def create(t, ks, os_, F, where=po):
        ks, os_ = np.array(ks, np.uint32), np.array(os_, np.uint32)
        return lib.grail_fir_create(None, None if t is None else t.ctypes.data, ks.ctypes.data, os_.ctypes.data, F, where)

    bad = taps.copy()
    refused = [(taps, [9], [4], 1, None), (None, [9], [4], 1, po), (taps, [9], [4], 0, po), (taps, [1] * 65, [0] * 65, 65, po),
               (taps, [0], [0], 1, po), (taps, [4097], [0], 1, po), (taps, [9], [9], 1, po), (taps, [9, 1], [4, 1], 2, po),
               (taps, [4096, 9], [4095, 4294967295], 2, po)]
    for case in refused:
        assert create(*case) == G.ERR_INVALID_ARG, case[1:4]
        assert b"grail_fir_create" in lib.grail_last_error()
    assert lib.grail_fir_create(None, taps.ctypes.data, None, taps.ctypes.data, 1, po) == G.ERR_INVALID_ARG
    assert lib.grail_fir_create(None, taps.ctypes.data, taps.ctypes.data, None, 1, po) == G.ERR_INVALID_ARG
    for at, what in ((0, np.nan), (8, np.inf), (9, -np.inf)):               # (the last tap of filter 0, the first of filter 1 ...)
        bad[:] = taps
        bad[at] = what
        assert create(bad, [9, 1], [4, 0], 2) == G.ERR_INVALID_ARG and b"not finite" in lib.grail_last_error()
    bad[:] = taps
    bad[10] = np.nan                                                             # past the set's taps: not looked at
    a, b, ln, fake = 0x10000000, 0x20000000, 0x30000000, 0x40000000           # addresses nobody looks behind
    cases = [
        ((None, None, a, 64, ln, 1, None, b, 128, None, None), b"set is NULL"),
        ((None, None, a, 64, ln, 0, None, b, 128, None, None), b"set is NULL"),
        ((None, fake, a, 64, None, 1, None, b, 128, None, None), b"NULL buffer"),
        ((None, fake, None, 64, ln, 1, None, b, 128, None, None), b"NULL buffer"),
        ((None, fake, a, 64, ln, 1, None, None, 128, None, None), b"NULL buffer"),
        ((None, fake, a, 64, ln, 2, None, a + 4 * 64, 64, None, None), b"overlaps"),
        ((None, fake, a, 64, ln, 2, None, a - 4 * 32 * 2 + 4, 32, None, None), b"overlaps"),
        ((None, fake, a, 64, ln, 1, None, a, 64, None, None), b"overlaps"),
        ((None, fake, a, 2 ** 32 - 1, ln, 1024, None, 2 ** 50, 2 ** 32 - 1, None, None), b"2^31 chunks"),
    ]
    for args, word in cases:
        assert lib.grail_fir_async(*args) == G.ERR_INVALID_ARG, args
        assert word in lib.grail_last_error(), (args, lib.grail_last_error())
    assert lib.grail_fir_free(None, fake) == G.ERR_INVALID_ARG and lib.grail_fir_free(None, None) == G.OK
    if G.device_count() == 0:        # no context can exist: the valid calls say why, they do not compute on the CPU
        assert create(bad, [9, 1], [4, 0], 2) == G.ERR_NO_DEVICE and out.value == 0x77
        assert b"no usable HIP device" in lib.grail_last_error()
        assert lib.grail_fir_async(None, fake, a, 64, ln, 2, None, a + 4 * 128, 128, None, None) == G.ERR_NO_DEVICE
        assert lib.grail_fir_async(None, fake, None, 0, None, 0, None, None, 0, None, None) == G.ERR_NO_DEVICE


def test_header_python_and_rust_name_the_same_functions_and_constants(built):
    hdr = open(os.path.join(ROOT, "include", "grail_hip.h")).read()
    assert "levels, continued: FIR filtering" in hdr
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(set(re.findall(r"\b(grail_fir_[a-z0-9_]+)\s*\(", code))) == FUNCTIONS
    assert sorted(n for n in G.EXPORTS if n.startswith("grail_fir")) == FUNCTIONS
    sys_rs = open(os.path.join(ROOT, "grail-rs_amd", "rust", "grail-hip-sys", "src", "lib.rs")).read()
    assert sorted(set(re.findall(r"pub fn (grail_fir_[a-z0-9_]+)\s*\(", sys_rs))) == FUNCTIONS
    constants = dict(re.findall(r"#define (GRAIL_FIR_[A-Z_]+) (\d+)", hdr))
    assert constants == {"GRAIL_FIR_TAPS_MAX": "4096", "GRAIL_FIR_FILTERS_MAX": "64", "GRAIL_FIR_CHUNK": "2048"}
    assert dict(re.findall(r"pub const (GRAIL_FIR_[A-Z_]+): u32 = (\d+);", sys_rs)) == constants
    assert {"GRAIL_FIR_TAPS_MAX": str(G.FIR_TAPS_MAX), "GRAIL_FIR_FILTERS_MAX": str(G.FIR_FILTERS_MAX), "GRAIL_FIR_CHUNK": str(G.FIR_CHUNK)} == constants
    lib = G.load()
    assert lib.grail_abi_version() == G.ABI_VERSION == 4 and re.search(r"#define GRAIL_ABI_VERSION (\d+)", hdr).group(1) == "4"
    for name in FUNCTIONS:
        assert hasattr(lib, name), name


def test_dialogue_example_knows_the_band_option(built):
    exe = os.path.join(ROOT, "grail-rs_amd", "lib", "grail_dialogue")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "[--band LO HI [--taps K]]" in r.stderr
    for bad in (["--band", "300"], ["--band", "3400", "300"], ["--band", "-1", "300"], ["--band", "300", "1e9"], ["--band", "x", "300"],
                ["--band", "300", "3400", "--taps", "254"], ["--band", "300", "3400", "--taps", "1"], ["--band", "300", "3400", "--taps", "4097"],
                ["--taps", "255"]):
        r = subprocess.run([exe] + bad + ["a", "e"], capture_output=True, text=True)
        assert r.returncode == 2 and "usage" in r.stderr, bad
    if G.device_count() == 0:
        r = subprocess.run([exe, "-o", os.devnull, "--band", "300", "3400", "a", "e"], capture_output=True, text=True)
        assert r.returncode == 1 and "no HIP device" in r.stderr
