"""The pure-host side of short-time spectra against the page of numpy (tests/spectrum_model.py): the twiddle table, the windows
and the mel triangles bit for bit; what the contract rests on (the table's mirror, the conjugate symmetry of the model's bins,
the model against numpy's own FFT, triangles that tile); every refusal that can be reached without a device, and that a
correct call fails with GRAIL_ERR_NO_DEVICE only once its arguments have passed.  The refusals of grail_spectrum_async that
read the set's facts (frames_stride against the hop, bands_dev on a set of no bands, outputs that overlap the rows, the
grid) need a live set: tests/test_spectrum_gpu.py reaches them through the C ABI, tests/test_spectrum_sanitize.py in
spectrum_plan.cpp itself."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import grail_hip as G
import spectrum_model as M
from grail_hip import spectrum as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = list(range(M.LOG2_MIN, M.LOG2_MAX + 1))
FUNCTIONS = sorted(["grail_spectrum_twiddles", "grail_spectrum_frames", "grail_spectrum_window", "grail_spectrum_create",
                    "grail_spectrum_free", "grail_spectrum_async"])


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the tables -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", SIZES)
def test_twiddles_equal_the_models_and_mirror_exactly(built, p):
    T = S.twiddles(p)
    N = 1 << p
    assert T.shape == (N // 2, 2) and np.array_equal(bits(T), bits(M.twiddles(p)))
    # T[N/2 - j] = -conj(T[j]): the real part negated, the imaginary part the same, bit for bit
    j = np.arange(1, N // 4)
    assert np.array_equal(bits(T[N // 2 - j, 0]), bits(0.0 - T[j, 0])) and np.array_equal(bits(T[N // 2 - j, 1]), bits(T[j, 1]))
    assert tuple(T[0]) == (1.0, 0.0) and tuple(T[N // 4]) == (0.0, -1.0)
    # ... and they are the roots of unity: against numpy's cos and sin of the unmirrored argument, whose rounding (up to half
    # an ulp of pi, 2.2e-16) and the two results' (1.1e-16 each) bound the difference by 4.4e-16
    assert np.max(np.abs(T[:, 0] - np.cos(2 * np.pi * np.arange(N // 2) / N))) <= 4.5e-16
    assert np.max(np.abs(T[:, 1] + np.sin(2 * np.pi * np.arange(N // 2) / N))) <= 4.5e-16


@pytest.mark.parametrize("kind", [M.RECT, M.HANN, M.HAMMING])
@pytest.mark.parametrize("W", [1, 2, 63, 64, 100, 400, 1024, 4001, 4096])
def test_windows_equal_the_models(built, kind, W):
    w = S.window(kind, W)
    assert w.dtype == np.float32 and np.array_equal(bits32(w), bits32(M.window(kind, W)))
    if kind == M.HANN and W > 2:        # the periodic form: w[0] = 0, w[j] = w[W - j], and for an even W the peak of 1 at W / 2
        assert w[0] == 0.0 and np.allclose(w[1:], w[1:][::-1], atol=1e-6) and (W % 2 or w[W // 2] == 1.0)


MELS = [(16000, 9, 40, 0.0, 8000.0), (22050, 10, 80, 0.0, 11025.0), (48000, 12, 128, 20.0, 20000.0), (8000, 6, 8, 100.0, 3800.0),
        (44100, 7, 200, 0.0, 22050.0), (16000, 12, 256, 50.0, 7600.0)]


@pytest.mark.parametrize("rate,p,B,lo,hi", MELS)
def test_mel_tables_equal_the_models_and_tile(built, rate, p, B, lo, hi):
    first, count, weights = S.mel_design(rate, p, B, lo, hi)
    mf, mc, mw = M.mel_design(rate, p, B, lo, hi)
    assert np.array_equal(first, mf) and np.array_equal(count, mc) and np.array_equal(bits32(weights), bits32(mw))
    N = 1 << p
    assert np.all(first.astype(np.int64) + count <= N // 2 + 1) and np.all(weights > 0) and np.all(weights <= 1)
    # between the first and the last centre the neighbouring triangles sum to 1 at every bin, within binary32 rounding: each
    # of the two weights there is within 2^-24 relative of its binary64 value, and those two sum to 1 within a few 2^-53; the
    # weights sum to 1 in exact arithmetic, so the error is at most 2^-24 and a little
    dense = np.zeros((B, N // 2 + 1), np.float64)
    at = 0
    for b in range(B):
        dense[b, first[b]:first[b] + count[b]] = weights[at:at + count[b]]
        at += count[b]
    mel = lambda f: 2595.0 * np.log10(1.0 + f / 700.0)                              # noqa: E731
    centres = 700.0 * (10.0 ** ((mel(lo) + (mel(hi) - mel(lo)) * np.arange(1, B + 1) / (B + 1)) / 2595.0) - 1.0)
    f = np.arange(N // 2 + 1) * rate / N
    inside = (f >= centres[0] * (1 + 1e-12)) & (f <= centres[-1] * (1 - 1e-12))
    assert np.max(np.abs(dense[:, inside].sum(axis=0) - 1.0), initial=0.0) <= 2.0 ** -24 * 1.001
    if (rate, p, B) == (44100, 7, 200):
        assert np.any(count == 0)                                                   # more bands than bins: some catch none


# ---- what the contract rests on ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", SIZES)
def test_model_bins_are_conjugate_symmetric_and_near_numpys_fft(p):
    N = 1 << p
    rng = np.random.default_rng(p)
    a = np.concatenate([rng.standard_normal((3, N)), (rng.standard_normal((2, N)) * 1e-3).astype(np.float32).astype(np.float64),
                        np.ones((1, N))])
    re, im = M.transform(a, p)
    k = np.arange(1, N // 2)
    # X[N - k] = conj(X[k]) bit for bit, but for the sign of a zero
    assert np.array_equal(re[:, N - k], re[:, k])
    assert np.array_equal(im[:, N - k], 0.0 - im[:, k])
    P = M.power_of(re, im, p)
    want = np.abs(np.fft.rfft(a, axis=1)) ** 2
    worst = np.max(np.abs(P - want) / np.sum(want, axis=1, keepdims=True))
    print("p", p, "worst |P - rfft^2| / sum", worst)
    assert worst <= 1e-13


def test_frames_and_bands_of_the_model(built):
    for n, hop in [(0, 1), (0, 7), (1, 7), (7, 7), (8, 7), (2 ** 32 - 1, 1), (2 ** 64 - 1, 2 ** 32 - 1), (300000, 256)]:
        assert S.frames(n, hop) == M.frames(n, hop) == -(-n // hop)
    # a band's energy is the left fold, not numpy's pairwise sum
    P = np.array([[1e16, 1.0, 1.0, 1.0, 1.0]])
    assert M.bands_of(P, [0], [5], np.ones(5, np.float32))[0, 0] == 1e16
    assert M.bands_of(P, [1, 0, 4], [4, 0, 1], np.ones(5, np.float32)).tolist() == [[4.0, 0.0, 1.0]]


# ---- the arguments ------------------------------------------------------------------------------------------------------------------
def test_designer_refusals(built):
    lib = G.load()
    nan, inf = float("nan"), float("inf")
    buf = np.full(2 * 4096 + 8, 77.0, np.float64)
    for p in (0, 5, 13, 2 ** 31):
        assert lib.grail_spectrum_twiddles(p, buf.ctypes.data) == G.ERR_INVALID_ARG and np.all(buf == 77.0)
    assert lib.grail_spectrum_twiddles(6, None) == G.ERR_INVALID_ARG
    assert lib.grail_spectrum_twiddles(12, buf.ctypes.data) == G.OK and np.all(buf[4096:] == 77.0)
    out = C.c_uint64(77)
    assert lib.grail_spectrum_frames(5, 0, C.addressof(out)) == G.ERR_INVALID_ARG and out.value == 77
    assert lib.grail_spectrum_frames(5, 1, None) == G.ERR_INVALID_ARG
    w = np.full(4100, 77.0, np.float32)
    for kind, W in [(-1, 8), (3, 8), (1, 0), (1, 4097)]:
        assert lib.grail_spectrum_window(kind, W, w.ctypes.data) == G.ERR_INVALID_ARG and np.all(w == 77.0)
    assert lib.grail_spectrum_window(1, 8, None) == G.ERR_INVALID_ARG
    assert lib.grail_spectrum_window(2, 4096, w.ctypes.data) == G.OK and np.all(w[4096:] == 77.0)
    first, count, wt = np.full(260, 77, np.uint32), np.full(260, 77, np.uint32), np.full(70000, 77.0, np.float32)
    total = C.c_uint32(77)
    ok = (16000, 9, 40, 0.0, 8000.0)

    def mel(args, f=first, c=count, weights=wt, cap=len(wt), n=C.addressof(total)):
        return lib.grail_mel_design(*args, None if f is None else f.ctypes.data, None if c is None else c.ctypes.data,
                                    None if weights is None else weights.ctypes.data, cap, n)

    for at, bad in [(0, 0), (1, 5), (1, 13), (2, 0), (2, 257), (3, -1.0), (3, nan), (3, 8000.0), (3, 9000.0), (4, 8000.5), (4, nan),
                    (4, inf)]:
        args = list(ok)
        args[at] = bad
        assert mel(args) == G.ERR_INVALID_ARG, args
    assert mel((16000, 9, 256, 1000.0, 1000.0 + 1e-11)) == G.ERR_INVALID_ARG           # the 258 points coincide
    for kw in ({"f": None}, {"c": None}, {"weights": None}, {"n": None}):
        assert mel(ok, **kw) == G.ERR_INVALID_ARG, kw
    assert total.value == 77 and np.all(first == 77) and np.all(count == 77) and np.all(wt == 77.0)
    assert mel(ok, weights=None, cap=0) == G.ERR_BUFFER_TOO_SMALL and total.value == int(M.mel_design(*ok)[1].sum())
    assert mel(ok, cap=total.value - 1) == G.ERR_BUFFER_TOO_SMALL and np.all(first == 77) and np.all(wt == 77.0)
    assert mel(ok, cap=total.value) == G.OK and np.all(first[40:] == 77) and np.all(wt[total.value:] == 77.0)


def test_argument_errors_come_before_the_device(built):
    lib = G.load()
    out = C.c_void_p(0x77)
    po = C.addressof(out)
    win = np.ones(4096, np.float32)
    first, count = np.array([0, 10, 32], np.uint32), np.array([5, 0, 1], np.uint32)
    wts = np.ones(70000, np.float32)

    def create(p=6, w=win, W=64, hop=16, pad=0, B=3, f=first, c=count, wt=wts, where=po):
        ptr = lambda a: None if a is None else a.ctypes.data                           # noqa: E731
        return lib.grail_spectrum_create(None, p, ptr(w), W, hop, pad, B, ptr(f), ptr(c), ptr(wt), where)

    bad_window = win.copy()
    bad_window[63] = np.inf
    bad_weight = wts.copy()
    bad_weight[5] = np.nan
    cases = [
        ({"where": None}, b"NULL"), ({"w": None}, b"NULL"), ({"p": 5}, b"log2n"), ({"p": 13}, b"log2n"), ({"W": 0}, b"n_window"),
        ({"W": 65}, b"n_window"), ({"hop": 0}, b"hop is 0"), ({"pad": 64}, b"pad"), ({"W": 10, "pad": 10}, b"pad"),
        ({"B": 257, "f": np.zeros(257, np.uint32), "c": np.zeros(257, np.uint32)}, b"above 256"),
        ({"w": bad_window}, b"window number is not finite"), ({"f": None}, b"without band_first"), ({"c": None}, b"without band_first"),
        ({"c": np.array([5, 0, 2], np.uint32)}, b"leaves the bins"), ({"f": np.array([0, 34, 32], np.uint32)}, b"leaves the bins"),
        ({"f": np.array([0, 2 ** 32 - 1, 32], np.uint32), "c": np.array([5, 2, 1], np.uint32)}, b"leaves the bins"),
        ({"p": 12, "W": 64, "B": 33, "f": np.zeros(33, np.uint32), "c": np.full(33, 2000, np.uint32)}, b"more than 65 536"),
        ({"wt": None}, b"without band_weights"), ({"wt": bad_weight}, b"weight is not finite"),
    ]
    for kw, word in cases:
        assert create(**kw) == G.ERR_INVALID_ARG and out.value == 0x77, kw
        assert b"grail_spectrum_create" in lib.grail_last_error() and word in lib.grail_last_error(), (kw, lib.grail_last_error())
    a, b, ln, fake = 0x10000000, 0x20000000, 0x40000000, 0x50000000                    # addresses nobody looks behind
    # (ctx, set, rows, row_stride, len, n_rows, power, bands, frames_stride, n_frames, nonfinite)
    calls = [
        ((None, None, a, 64, ln, 1, b, None, 64, None, None), b"set is NULL"),
        ((None, None, a, 64, ln, 0, b, None, 64, None, None), b"set is NULL"),
        ((None, fake, a, 64, ln, 1, None, None, 64, None, None), b"both NULL"),
        ((None, fake, a, 64, ln, 0, None, None, 64, None, None), b"both NULL"),
        ((None, fake, a, 64, None, 1, b, None, 64, None, None), b"NULL buffer"),
        ((None, fake, None, 64, ln, 1, None, b, 64, None, None), b"NULL buffer"),
        ((None, fake, a, 2 ** 59, ln, 4, b, None, 2 ** 59, None, None), b"2^60 samples"),
    ]
    for args, word in calls:
        assert lib.grail_spectrum_async(*args) == G.ERR_INVALID_ARG, args
        assert word in lib.grail_last_error() and b"grail_spectrum_async" in lib.grail_last_error(), (args, lib.grail_last_error())
    assert lib.grail_spectrum_free(None, fake) == G.ERR_INVALID_ARG and lib.grail_spectrum_free(None, None) == G.OK
    if G.device_count() == 0:        # no context can exist: the valid calls say why, they do not compute on the CPU
        for kw in ({}, {"B": 0, "f": None, "c": None, "wt": None}, {"p": 12, "W": 4096, "pad": 4095, "hop": 2 ** 32 - 1},
                   {"c": np.array([5, 0, 0], np.uint32), "f": np.array([0, 33, 33], np.uint32)}):
            assert create(**kw) == G.ERR_NO_DEVICE and out.value == 0x77, kw
            assert b"no usable HIP device" in lib.grail_last_error()
        assert lib.grail_spectrum_async(None, fake, a, 64, ln, 2, b, None, 4, None, None) == G.ERR_NO_DEVICE
        assert lib.grail_spectrum_async(None, fake, a, 64, ln, 2, None, b, 4, ln, ln) == G.ERR_NO_DEVICE
        assert lib.grail_spectrum_async(None, fake, None, 0, None, 0, b, None, 0, None, None) == G.ERR_NO_DEVICE
        with pytest.raises(G.GrailError) as ei:
            G.Context(0)
        assert ei.value.status == G.ERR_NO_DEVICE


def header_model():
    """include/grail_spectrum.h as tests/test_abi.py reads grail_hip.h: {function: (return type, [parameter types])}, the types
    in that module's canonical form"""
    from test_abi import _c_decl, _c_type
    src = open(os.path.join(ROOT, "include", "grail_spectrum.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"^\s*#.*$", "", src, flags=re.M)
    src = re.sub(r"typedef struct \w+\s+\w+;", "", src).replace('extern "C" {', "")
    funcs = {}
    for ret, name, params in re.findall(r"([\w\s\*]+?)\b(grail_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        funcs[name] = (_c_type(re.findall(r"\w+|\*", ret)), [_c_decl(prm)[1] for prm in params.split(",")])
    return funcs


def test_header_python_and_rust_declare_the_same_functions_and_constants(built):
    """The family has a header, a Python module and a Rust module of its own (the recorded listing of the package's top level,
    tests/golden/binding_surface.txt, stays as it is): here they are held to each other as tests/test_abi.py holds the rest, by
    name, parameter count, and kind and width of every parameter and return value."""
    from test_abi import _ctypes_class, _header_class, _rust_type
    main = open(os.path.join(ROOT, "include", "grail_hip.h")).read()
    assert '#include "grail_spectrum.h"' in main and "grail_spectrum_" not in re.sub(r"/\*.*?\*/|^\s*#.*$", "", main, flags=re.S | re.M)
    hdr = open(os.path.join(ROOT, "include", "grail_spectrum.h")).read()
    assert "levels, continued: short-time spectra" in hdr and "NO LOGARITHM ON THE DEVICE" in hdr and "Slaney" in hdr
    funcs = header_model()
    assert sorted(funcs) == sorted(FUNCTIONS + ["grail_mel_design"]) == sorted(S.SIGNATURES)
    assert not [n for n in G.EXPORTS if "spectrum" in n or "mel" in n]              # (the table of grail_hip.h's functions)
    lib = G.load()
    for name, (ret, params) in funcs.items():
        fn = getattr(lib, name)
        header = [_header_class(ret)] + [_header_class(t) for t in params]
        assert header == [_ctypes_class(fn.restype)] + [_ctypes_class(t) for t in fn.argtypes], name
    rs = open(os.path.join(ROOT, "grail-rs_amd", "rust", "grail-hip-sys", "src", "spectrum.rs")).read()
    assert "pub mod spectrum;" in open(os.path.join(ROOT, "grail-rs_amd", "rust", "grail-hip-sys", "src", "lib.rs")).read()
    rust = {}
    for name, params, ret in re.findall(r"pub fn (grail_[a-z0-9_]+)\s*\(([^)]*)\)\s*->\s*([^;]+?)\s*;", rs, flags=re.S):
        rust[name] = (_rust_type(ret.strip()), [_rust_type(prm.split(":", 1)[1].strip()) for prm in params.split(",") if prm.strip()])
    assert rust == funcs
    constants = dict(re.findall(r"#define (GRAIL_SPECTRUM_[A-Z0-9_]+)\s+(\d+)", hdr))
    assert constants == {"GRAIL_SPECTRUM_LOG2_MIN": "6", "GRAIL_SPECTRUM_LOG2_MAX": "12", "GRAIL_SPECTRUM_BANDS_MAX": "256",
                         "GRAIL_SPECTRUM_WEIGHTS_MAX": "65536", "GRAIL_SPECTRUM_RECT": "0", "GRAIL_SPECTRUM_HANN": "1",
                         "GRAIL_SPECTRUM_HAMMING": "2", "GRAIL_SPECTRUM_CHUNK_FRAMES": "8"}
    assert dict(re.findall(r"pub const (GRAIL_SPECTRUM_[A-Z0-9_]+): (?:u32|c_int) = (\d+);", rs)) == constants
    mine = {"GRAIL_SPECTRUM_LOG2_MIN": S.LOG2_MIN, "GRAIL_SPECTRUM_LOG2_MAX": S.LOG2_MAX, "GRAIL_SPECTRUM_BANDS_MAX": S.BANDS_MAX,
            "GRAIL_SPECTRUM_WEIGHTS_MAX": S.WEIGHTS_MAX, "GRAIL_SPECTRUM_RECT": S.RECT, "GRAIL_SPECTRUM_HANN": S.HANN,
            "GRAIL_SPECTRUM_HAMMING": S.HAMMING, "GRAIL_SPECTRUM_CHUNK_FRAMES": S.CHUNK_FRAMES}
    assert {k: str(v) for k, v in mine.items()} == constants
    assert (M.LOG2_MIN, M.LOG2_MAX, M.BANDS_MAX, M.WEIGHTS_MAX, M.CHUNK_FRAMES) == (6, 12, 256, 65536, 8)
    assert (M.RECT, M.HANN, M.HAMMING) == (S.RECT, S.HANN, S.HAMMING)
    assert G.spectrum is S and all(callable(getattr(S, name)) for name in ("create", "free", "transform_async", "transform"))
