"""Recursive filtering (include/grail_hip.h, "levels, continued: recursive filtering" and "... of streams") without a GPU: the
numpy model of tests/iir_model.py tied to the K-weighting model it generalises, grail_iir_design against the header's
formulas and against what the kinds promise of their responses, grail_iir_stream_len against the stream model, and every
refusal of the designer, grail_iir_create, grail_iir_async and the stream calls before the device is looked for."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import grail_hip as G
import iir_model as M
from test_loudness_host import kweight_hops_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = sorted(["grail_iir_design", "grail_iir_create", "grail_iir_free", "grail_iir_async", "grail_iir_stream_len",
                    "grail_iir_stream_open", "grail_iir_stream_next_async", "grail_iir_stream_finish_async",
                    "grail_iir_stream_close"])
KINDS = {"lowpass": G.IIR_LOWPASS, "highpass": G.IIR_HIGHPASS, "bandpass": G.IIR_BANDPASS, "notch": G.IIR_NOTCH,
         "peak": G.IIR_PEAK, "lowshelf": G.IIR_LOWSHELF, "highshelf": G.IIR_HIGHSHELF}


NEGATIVE_ZEROS = [-1.0, -1.0, -1.0, 0.0, 0.0]      # a section that answers silence with -0.0 (below)


def bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


# ---- the model is the K-weighting model's recurrence ---------------------------------------------------------------------
def test_the_model_fed_the_k_weighting_gives_the_loudness_models_z():
    """The two sections of grail_kweighting(48000) through the model, read before the final rounding, are the z of the
    loudness model: folded as it folds them (acc = acc + z*z from +0.0 per hop of 4800), they give its hop sums bit for bit.
    Rows with NaN, Inf, -0.0 and denormals among them."""
    rng = np.random.default_rng(7)
    coef = np.zeros(10)
    assert G.load().grail_kweighting(48000, coef.ctypes.data) == G.OK
    rows = []
    for n in (0, 1, 4799, 4800, 9700, 14401):
        x = rng.uniform(-1.0, 1.0, n).astype(np.float32)
        if n > 10:
            x[[1, n // 2, n - 1]] = (np.nan, np.inf, -np.inf)
            x[3], x[4] = np.float32(-0.0), np.float32(1e-42)
        rows.append(x)
    want = kweight_hops_model(rows, 48000, coef)
    got = M.iir_model(rows, [coef.reshape(2, 5)], tail=0, exact=True)
    for (z, n_out, bad), (hops, w_bad), x in zip(got, want, rows):
        assert n_out == len(x) and bad == w_bad
        mine = []
        for h in range(len(x) // 4800):
            acc = 0.0
            for zt in z[h * 4800:(h + 1) * 4800].tolist():
                acc = acc + zt * zt
            mine.append(acc)
        assert np.array_equal(bits(mine), bits(hops)), len(x)
    assert sum(len(h) for h, _ in want) == 1 + 2 + 3


def test_a_section_is_not_an_identity_and_fewer_sections_are_not_padded():
    """b0 = 1 alone turns -0.0 into +0.0; two of them too; and a row of one section beside a row of eight comes out as it
    does alone (the model runs both in one array, as a wave does)."""
    ident = [1.0, 0.0, 0.0, 0.0, 0.0]
    x = np.array([-0.0, 1.0, -0.0, -2.5], np.float32)
    (y, n_out, bad), = M.iir_model([x], [[ident]])
    assert n_out == 4 and bad == 0 and np.array_equal(y.view(np.uint32), np.array([0.0, 1.0, 0.0, -2.5], np.float32).view(np.uint32))
    # on silence b = -1 -1 -1 makes s2 = -0.0 at once, s1 = -0.0 a sample later and the third y = -0.0 + -0.0 = -0.0 ...
    gain = [NEGATIVE_ZEROS]
    eight = [NEGATIVE_ZEROS] + [ident] * 7                                          # ... unless identities follow it
    zero = np.zeros(5, np.float32)
    alone = M.iir_model([zero], [gain])[0][0]
    both = M.iir_model([zero, zero], [gain, eight], which=[0, 1])
    assert np.signbit(alone).tolist()[:3] == [False, False, True] and np.all(alone == 0.0)
    assert np.array_equal(alone.view(np.uint32), both[0][0].view(np.uint32))
    assert not np.any(np.signbit(both[1][0]))


# ---- the designer -----------------------------------------------------------------------------------------------------------
def design_model(kind, rate, f0, q, g):
    """the header's formulas in Python floats (binary64), in the order the header writes them"""
    K = math.tan(3.141592653589793 * f0 / float(rate))
    KQ, KK = K / q, K * K
    D = (1.0 + KQ) + KK
    a1, a2 = 2.0 * (KK - 1.0) / D, ((1.0 - KQ) + KK) / D
    if kind == "lowpass":
        b = (KK / D, 2.0 * KK / D, KK / D)
    elif kind == "highpass":
        b = (1.0 / D, -2.0 / D, 1.0 / D)
    elif kind == "bandpass":
        b = (KQ / D, 0.0, -KQ / D)
    elif kind == "notch":
        b = ((1.0 + KK) / D, 2.0 * (KK - 1.0) / D, (1.0 + KK) / D)
    elif kind == "highshelf":
        V = math.pow(10.0, g / 20.0)
        W = math.sqrt(V)
        b = (((V + W * KQ) + KK) / D, 2.0 * (KK - V) / D, ((V - W * KQ) + KK) / D)
    elif kind == "lowshelf":
        V = math.pow(10.0, g / 20.0)
        W = math.sqrt(V)
        b = (((1.0 + W * KQ) + V * KK) / D, 2.0 * (V * KK - 1.0) / D, ((1.0 - W * KQ) + V * KK) / D)
    elif g >= 0.0:
        V = math.pow(10.0, g / 20.0)
        b = (((1.0 + V * KQ) + KK) / D, 2.0 * (KK - 1.0) / D, ((1.0 - V * KQ) + KK) / D)
    else:
        V = math.pow(10.0, -g / 20.0)
        E = (1.0 + V * KQ) + KK
        b = (D / E, 2.0 * (KK - 1.0) / E, ((1.0 - KQ) + KK) / E)
        a1, a2 = 2.0 * (KK - 1.0) / E, ((1.0 - V * KQ) + KK) / E
    return np.array([b[0], b[1], b[2], a1, a2], np.float64)


DESIGNS = [(kind, rate, f0, q, g) for kind in KINDS for rate, f0 in ((48000, 1000.0), (44100, 3000.0), (8000, 1200.5), (96000, 6000.0))
           for q, g in ((0.7071067811865476, 6.0), (4.0, -9.5), (0.5, 12.0))]


@pytest.mark.parametrize("kind,rate,f0,q,g", DESIGNS)
def test_design_matches_its_formulas(built, kind, rate, f0, q, g):
    """as tests/test_fir_host.py holds grail_fir_design: the table is the header's formulas, bit for bit where the C library's
    tan, pow and sqrt are Python's, within one unit in the last place of each number otherwise"""
    got, want = G.iir_design(KINDS[kind], rate, f0, q, g), design_model(kind, rate, f0, q, g)
    assert got.dtype == np.float64 and got.shape == (5,) and np.all(np.isfinite(got))
    exact = np.array_equal(bits(got), bits(want))
    near = np.abs(got - want) <= np.spacing(np.maximum(np.abs(got), np.abs(want)))
    print(f"\n{kind} {rate} Hz f0 {f0:g} Q {q:g} G {g:g}: " + ("bit for bit" if exact else f"within 1 ulp: {bool(near.all())}"))
    assert exact or bool(near.all()), (got, want)


RESPONSES = [(rate, f0, q) for rate, f0 in ((48000, 1000.0), (44100, 3000.0), (8000, 1200.5)) for q in (0.7071067811865476, 2.0)]


@pytest.mark.parametrize("rate,f0,q", RESPONSES)
def test_design_responses(built, rate, f0, q):
    """|H| from the returned coefficients, in numpy's complex128, where each kind's is known in closed form.  The bound is
    relative 1e-12 (absolute where the value is 0): a biquad's response is a five-term rational; at 0 and at half the rate
    the sums 1 + a1 + a2 and b0 + b1 + b2 cancel down to 4 K^2 / D, which for these f0 / rate (K >= 0.065) is at least 1 / 100
    of their terms, so the 2^-53 of each term and of each sum is at most a few hundred times 1.1e-16 of the result."""
    tol = 1e-12
    w0, nyq = 2.0 * math.pi * f0 / rate, math.pi

    def at(kind, w, g=0.0):
        return float(M.response(G.iir_design(KINDS[kind], rate, f0, q, g), [w])[0])

    assert abs(at("lowpass", 0.0) - 1.0) <= tol and at("lowpass", nyq) <= tol
    assert at("highpass", 0.0) <= tol and abs(at("highpass", nyq) - 1.0) <= tol
    assert abs(at("bandpass", w0) - 1.0) <= tol and at("bandpass", 0.0) <= tol and at("bandpass", nyq) <= tol
    assert at("notch", w0) <= tol and abs(at("notch", 0.0) - 1.0) <= tol and abs(at("notch", nyq) - 1.0) <= tol
    for g in (6.0, -6.0, 12.5, -3.25):
        V = 10.0 ** (g / 20.0)
        assert abs(at("peak", w0, g) / V - 1.0) <= tol, g
        assert abs(at("peak", 0.0, g) - 1.0) <= tol and abs(at("peak", nyq, g) - 1.0) <= tol, g
        assert abs(at("lowshelf", 0.0, g) / V - 1.0) <= tol and abs(at("lowshelf", nyq, g) - 1.0) <= tol, g
        assert abs(at("highshelf", 0.0, g) - 1.0) <= tol and abs(at("highshelf", nyq, g) / V - 1.0) <= tol, g


def test_design_has_the_k_weighting_shelfs_form_and_the_butterworth_recipe_works(built):
    # the high-pass of grail_kweighting(48000) is the designer's at its f0 and Q up to the rounding of D's grouping
    kw = np.zeros(10)
    assert G.load().grail_kweighting(48000, kw.ctypes.data) == G.OK
    hp = G.iir_design(G.IIR_HIGHPASS, 48000, 38.13547087602444, 0.5003270373238773)
    assert np.allclose(hp[3:], kw[8:], rtol=1e-15, atol=0) and np.allclose(hp[:3] / hp[0], kw[5:8], rtol=1e-15, atol=0)
    # order 2m = 6 low-pass at 2 kHz: |H|^2 = 1 / (1 + (tan(w/2) / tan(w0/2))^12), 1/2 at f0
    m, rate, f0 = 3, 48000, 2000.0
    secs = [G.iir_design(G.IIR_LOWPASS, rate, f0, 1.0 / (2.0 * math.cos(math.pi * (2 * k + 1) / (4 * m)))) for k in range(m)]
    w = 2.0 * math.pi * np.array([100.0, 1000.0, 2000.0, 4000.0, 12000.0]) / rate
    want = 1.0 / np.sqrt(1.0 + (np.tan(w / 2.0) / math.tan(math.pi * f0 / rate)) ** (4 * m))
    assert np.allclose(M.response(np.array(secs), w), want, rtol=1e-11, atol=0)


def test_design_refusals(built):
    lib = G.load()
    buf = np.full(8, 77.0, np.float64)
    nan, inf = float("nan"), float("inf")
    for kind, rate, f0, q, g in [(-1, 48000, 1000.0, 1.0, 0.0), (7, 48000, 1000.0, 1.0, 0.0), (0, 0, 1000.0, 1.0, 0.0),
                                 (0, 48000, 0.0, 1.0, 0.0), (0, 48000, -5.0, 1.0, 0.0), (0, 48000, 24000.0, 1.0, 0.0),
                                 (0, 48000, 30000.0, 1.0, 0.0), (0, 48000, nan, 1.0, 0.0), (0, 48000, inf, 1.0, 0.0),
                                 (0, 48000, 1000.0, 0.0, 0.0), (0, 48000, 1000.0, -1.0, 0.0), (0, 48000, 1000.0, nan, 0.0),
                                 (0, 48000, 1000.0, inf, 0.0), (4, 48000, 1000.0, 1.0, nan), (4, 48000, 1000.0, 1.0, inf),
                                 (0, 48000, 1000.0, 1.0, -inf), (6, 48000, 1000.0, 1.0, 1e5)]:
        assert lib.grail_iir_design(kind, rate, f0, q, g, buf.ctypes.data) == G.ERR_INVALID_ARG, (kind, rate, f0, q, g)
        assert np.all(buf == 77.0)
    assert lib.grail_iir_design(0, 48000, 1000.0, 1.0, 0.0, None) == G.ERR_INVALID_ARG
    assert lib.grail_iir_design(0, 48000, 1000.0, 1.0, 0.0, buf.ctypes.data) == G.OK and np.all(buf[5:] == 77.0) and np.all(buf[:5] != 77.0)


# ---- the stream's lengths -----------------------------------------------------------------------------------------------------
def test_stream_len_is_the_stream_models(built):
    lib = G.load()
    out = C.c_uint64(77)
    model = M.IirStreamModel([[[1.0, 0.0, 0.0, 0.0, 0.0]]], [0, 0, 0], tail=5)
    fed = [0, 0, 0]
    for feed in ([0, 3, 0], [2, 0, 0], [0, 1, 0]):
        got = model.next([np.zeros(n, np.float32) for n in feed])
        for r, n in enumerate(feed):
            assert G.iir_stream_len(fed[r], n, 5) == got[r][1] == M.stream_len(fed[r], n, 5, False) == n
            fed[r] += n
    tails = model.finish()
    assert [len(t) for t in tails] == [G.iir_stream_len(f, 0, 5, True) for f in fed] == [5, 5, 0]
    for before, n, tail in ((0, 0, 0), (0, 7, 0), (2 ** 40, 2 ** 32 - 1, 2 ** 32 - 1), (2 ** 63 - 2, 1, 9)):
        assert G.iir_stream_len(before, n, tail) == n and G.iir_stream_len(before, 0, tail, True) == (tail if before else 0)
    for args in ((0, 1, 5, 1), (2 ** 63, 0, 5, 0), (2 ** 63 - 1, 1, 5, 0), (5, 2 ** 63, 5, 0)):
        assert lib.grail_iir_stream_len(*args, C.addressof(out)) == G.ERR_INVALID_ARG and out.value == 77, args
    assert lib.grail_iir_stream_len(0, 1, 5, 0, None) == G.ERR_INVALID_ARG


# ---- the arguments --------------------------------------------------------------------------------------------------------------
def test_argument_errors_come_before_the_device(built):
    lib = G.load()
    coef = np.linspace(-0.9, 0.9, 5 * 8 * 65)
    out = C.c_void_p(0x77)
    po = C.addressof(out)

    def create(c, ss, F, where=po):
        ss = np.array(ss, np.uint32)
        return lib.grail_iir_create(None, None if c is None else c.ctypes.data, ss.ctypes.data, F, where)

    for case in [(coef, [2], 1, None), (None, [2], 1, po), (coef, [2], 0, po), (coef, [1] * 65, 65, po), (coef, [0], 1, po),
                 (coef, [9], 1, po), (coef, [8, 4294967295], 2, po)]:
        assert create(*case) == G.ERR_INVALID_ARG, case[1:3]
        assert b"grail_iir_create" in lib.grail_last_error()
    assert lib.grail_iir_create(None, coef.ctypes.data, None, 1, po) == G.ERR_INVALID_ARG
    bad = coef.copy()
    for at, what in ((0, np.nan), (14, np.inf), (15, -np.inf)):               # (the last of filter 0, the first of filter 1 ...)
        bad[:] = coef
        bad[at] = what
        assert create(bad, [3, 1], 2) == G.ERR_INVALID_ARG and b"not finite" in lib.grail_last_error()
    bad[:] = coef
    bad[20] = np.nan                                                             # past the set's sections: not looked at
    a, b, ln, fake = 0x10000000, 0x20000000, 0x30000000, 0x40000000           # addresses nobody looks behind
    cases = [
        ((None, None, a, 64, ln, 1, None, 0, b, 128, None, None), b"set is NULL"),
        ((None, None, a, 64, ln, 0, None, 0, b, 128, None, None), b"set is NULL"),
        ((None, fake, a, 64, None, 1, None, 0, b, 128, None, None), b"NULL buffer"),
        ((None, fake, None, 64, ln, 1, None, 0, b, 128, None, None), b"NULL buffer"),
        ((None, fake, a, 64, ln, 1, None, 0, None, 128, None, None), b"NULL buffer"),
        ((None, fake, a, 64, ln, 2, None, 9, a + 4 * 64, 64, None, None), b"overlaps"),
        ((None, fake, a, 64, ln, 2, None, 0, a - 4 * 32 * 2 + 4, 32, None, None), b"overlaps"),
        ((None, fake, a, 64, ln, 1, None, 0, a, 64, None, None), b"overlaps"),
        ((None, fake, a, 2 ** 33, ln, 1, None, 2 ** 32 - 1, 2 ** 50, 2 ** 33, None, None), b"2^32 output samples"),
        ((None, fake, a, 2 ** 32 - 1, ln, 1, None, 1, 2 ** 50, 2 ** 32, None, None), b"2^32 output samples"),
        ((None, fake, a, 2 ** 59, ln, 4, None, 0, 2 ** 62, 64, None, None), b"2^60 samples"),
    ]
    for args, word in cases:
        assert lib.grail_iir_async(*args) == G.ERR_INVALID_ARG, args
        assert word in lib.grail_last_error() and b"grail_iir_async" in lib.grail_last_error(), (args, lib.grail_last_error())
    assert lib.grail_iir_free(None, fake) == G.ERR_INVALID_ARG and lib.grail_iir_free(None, None) == G.OK
    # streams: no context, no stream; a stream nobody looks into
    assert lib.grail_iir_stream_open(None, fake, 1, None, 0, po) == G.ERR_INVALID_ARG and out.value == 0x77
    assert lib.grail_iir_stream_close(None, fake) == G.ERR_INVALID_ARG and lib.grail_iir_stream_close(None, None) == G.OK
    stream_cases = [
        (lib.grail_iir_stream_next_async, (None, None, a, 64, ln, b, 64, None, None), b"the stream is NULL"),
        (lib.grail_iir_stream_next_async, (None, fake, a, 64, ln, b, 63, None, None), b"out_stride < in_stride"),
        (lib.grail_iir_stream_next_async, (None, fake, a, 64, None, b, 64, None, None), b"NULL buffer"),
        (lib.grail_iir_stream_next_async, (None, fake, None, 64, ln, b, 64, None, None), b"NULL buffer"),
        (lib.grail_iir_stream_next_async, (None, fake, a, 64, ln, None, 64, None, None), b"NULL buffer"),
        (lib.grail_iir_stream_next_async, (None, fake, a, 64, ln, a + 4 * 63, 64, None, None), b"overlaps"),
        (lib.grail_iir_stream_finish_async, (None, None, None, b, 64, None), b"the stream is NULL"),
        (lib.grail_iir_stream_finish_async, (None, fake, None, b, 0, None), b"below the stream's tail"),
        (lib.grail_iir_stream_finish_async, (None, fake, None, None, 64, None), b"NULL buffer"),
    ]
    for fn, args, word in stream_cases:
        assert fn(*args) == G.ERR_INVALID_ARG, args
        assert word in lib.grail_last_error(), (args, lib.grail_last_error())
    if G.device_count() == 0:        # no context can exist: the valid calls say why, they do not compute on the CPU
        assert create(bad, [3, 1], 2) == G.ERR_NO_DEVICE and out.value == 0x77
        assert b"no usable HIP device" in lib.grail_last_error()
        assert lib.grail_iir_async(None, fake, a, 64, ln, 2, None, 7, a + 4 * 128, 128, None, None) == G.ERR_NO_DEVICE
        assert lib.grail_iir_async(None, fake, None, 0, None, 0, None, 0, None, 0, None, None) == G.ERR_NO_DEVICE
        assert lib.grail_iir_stream_next_async(None, fake, a, 64, ln, b, 64, None, None) == G.ERR_NO_DEVICE
        assert lib.grail_iir_stream_finish_async(None, fake, None, b, 64, None) == G.ERR_NO_DEVICE


def test_header_python_and_rust_name_the_same_functions_and_constants(built):
    hdr = open(os.path.join(ROOT, "include", "grail_hip.h")).read()
    assert "levels, continued: recursive filtering" in hdr and "levels, continued: recursive filtering of streams" in hdr
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(set(re.findall(r"\b(grail_iir_[a-z0-9_]+)\s*\(", code))) == FUNCTIONS
    assert sorted(n for n in G.EXPORTS if n.startswith("grail_iir")) == FUNCTIONS
    sys_rs = open(os.path.join(ROOT, "grail-rs_amd", "rust", "grail-hip-sys", "src", "lib.rs")).read()
    assert sorted(set(re.findall(r"pub fn (grail_iir_[a-z0-9_]+)\s*\(", sys_rs))) == FUNCTIONS
    constants = dict(re.findall(r"#define (GRAIL_IIR_[A-Z_]+)\s+(\d+)", hdr))
    assert constants == {"GRAIL_IIR_SECTIONS_MAX": "8", "GRAIL_IIR_FILTERS_MAX": "64", "GRAIL_IIR_LOWPASS": "0",
                         "GRAIL_IIR_HIGHPASS": "1", "GRAIL_IIR_BANDPASS": "2", "GRAIL_IIR_NOTCH": "3", "GRAIL_IIR_PEAK": "4",
                         "GRAIL_IIR_LOWSHELF": "5", "GRAIL_IIR_HIGHSHELF": "6"}
    assert dict(re.findall(r"pub const (GRAIL_IIR_[A-Z_]+): (?:u32|c_int) = (\d+);", sys_rs)) == constants
    mine = {"GRAIL_IIR_SECTIONS_MAX": G.IIR_SECTIONS_MAX, "GRAIL_IIR_FILTERS_MAX": G.IIR_FILTERS_MAX, "GRAIL_IIR_LOWPASS": G.IIR_LOWPASS,
            "GRAIL_IIR_HIGHPASS": G.IIR_HIGHPASS, "GRAIL_IIR_BANDPASS": G.IIR_BANDPASS, "GRAIL_IIR_NOTCH": G.IIR_NOTCH,
            "GRAIL_IIR_PEAK": G.IIR_PEAK, "GRAIL_IIR_LOWSHELF": G.IIR_LOWSHELF, "GRAIL_IIR_HIGHSHELF": G.IIR_HIGHSHELF}
    assert {k: str(v) for k, v in mine.items()} == constants and M.SECTIONS_MAX == G.IIR_SECTIONS_MAX and M.REFUSED == G.LIMIT_REFUSED
    lib = G.load()
    assert lib.grail_abi_version() == G.ABI_VERSION == 4 and re.search(r"#define GRAIL_ABI_VERSION (\d+)", hdr).group(1) == "4"
    for name in FUNCTIONS:
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None, name


def test_dialogue_example_knows_the_eq_option(built):
    import subprocess
    exe = os.path.join(ROOT, "grail-rs_amd", "lib", "grail_dialogue")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "[--eq KIND:F0:Q[:GAIN]]..." in r.stderr
    for bad in (["--eq"], ["--eq", "peak"], ["--eq", "peak:1000"], ["--eq", "treble:1000:1"], ["--eq", "peak:1000:1:3:4"],
                ["--eq", "peak:x:1"], ["--eq", "peak:1000:0"], ["--eq", "lowpass:22050:1"], ["--eq", "lowpass:0:1"],
                ["--eq", "peak:1000:1:"], ["--eq", "peak:1000:1:nan"], ["--eq", "highpass:100:0.7"] * 9):
        r = subprocess.run([exe] + bad + ["a", "e"], capture_output=True, text=True)
        assert r.returncode == 2 and "usage" in r.stderr, bad
    if G.device_count() == 0:
        r = subprocess.run([exe, "-o", os.devnull, "--eq", "highpass:100:0.707", "--eq", "peak:3000:1.5:4", "a", "e"],
                           capture_output=True, text=True)
        assert r.returncode == 1 and "no HIP device" in r.stderr


def test_interactive_example_knows_the_eq_option(built):
    import subprocess
    exe = os.path.join(ROOT, "grail-rs_amd", "lib", "grail_interactive")
    r = subprocess.run([exe, "--nothing"], capture_output=True, text=True)
    assert r.returncode == 2 and "[--eq KIND:F0:Q[:GAIN]]..." in r.stderr
    for bad in (["--eq"], ["--eq", "peak"], ["--eq", "peak:1000"], ["--eq", "treble:1000:1"], ["--eq", "peak:1000:1:3:4"],
                ["--eq", "peak:x:1"], ["--eq", "peak:1000:0"], ["--eq", "lowpass:22050:1"], ["--eq", "lowpass:0:1"],
                ["--eq", "peak:1000:1:"], ["--eq", "peak:1000:1:nan"], ["--eq", "highpass:100:0.7"] * 9,
                ["--rate", "8000", "--eq", "lowpass:4000:1"]):         # (designed at the rate that is written: 4 000 Hz is its half)
        r = subprocess.run([exe] + bad, capture_output=True, text=True, input="")
        assert r.returncode == 2 and "usage" in r.stderr, bad
    if G.device_count() == 0:
        r = subprocess.run([exe, "--eq", "highpass:100:0.707", "--eq", "peak:3000:1.5:4", "--rate", "8000"],
                           capture_output=True, text=True, input="a e\n")
        assert r.returncode == 1 and "no HIP device" in r.stderr
