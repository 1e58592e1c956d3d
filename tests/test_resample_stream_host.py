"""Resample streams (include/grail_hip.h, "levels, continued: sample-rate conversion of streams") without a GPU:
grail_resample_stream_len against the numpy model of tests/resample_stream_model.py and against Python integers where N U
has long outgrown 64 bits; the model's concatenation property against tests/resample_model.py (the calls' outputs end to end,
then the tail, are the one-shot row, bit for bit, whatever the split), also in the form the kernel works in (a ring of the
last samples, the next output's input time and phase kept from call to call, never a product of N); the argument errors of
the calls, which come before the device is asked for; and the launch arithmetic, which shows that the GPU file's pairs and
layouts start every instantiation of resample_stream_kernel."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import grail_hip as G
from resample_model import resample_model
from resample_stream_model import advance, ceil_div, known, splits, stream_len, stream_model
from test_resample_gpu import VARIANTS, variant
import test_resample_stream_gpu as GPU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ["grail_resample_stream_close", "grail_resample_stream_finish_async", "grail_resample_stream_len",
             "grail_resample_stream_next_async", "grail_resample_stream_open"]
RATES = [8000, 11025, 16000, 22050, 24000, 44100, 48000, 96000]
LISTED = [(a, b) for a in RATES for b in RATES if a != b and {a, b} != {11025, 96000}]
OTHER = [(2, 3), (3, 2), (50, 3), (48000, 2000)]
SMALL = [(2, 3), (3, 2), (48000, 16000), (48000, 96000), (44100, 48000), (48000, 44100), (50, 3), (8000, 96000)]


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def ring_capacity(P):
    """the samples of a row's ring: P - 1 rounded up to a power of two"""
    cap = 1
    while cap < P - 1:
        cap *= 2
    return cap


# ---- the length ----------------------------------------------------------------------------------------------------------------
def test_stream_len_agrees_with_the_model_and_with_python_integers(built):
    assert len(LISTED) == 54
    for pair in LISTED + OTHER:
        U, D, P = G.resample_ratio(*pair)
        h = P // 2
        for N in (0, 1, h - 1, h, h + 1, P, 2 ** 40, 2 ** 62 - 1):
            for n in (0, 1, 2, h, h + 1, 480, 4800):
                got = G.resample_stream_len(N, n, *pair)
                # (the model is Python integers throughout: at 2^40 and 2^62 - 1 this is the check against them)
                assert got == stream_len(N, n, U, D, P) <= ceil_div(n * U, D), (pair, N, n)
                # fed in two calls or in one: the same outputs
                assert got + G.resample_stream_len(N + n, 7, *pair) == G.resample_stream_len(N, n + 7, *pair)
            tail = G.resample_stream_len(N, 0, *pair, finishing=True)
            assert tail == stream_len(N, 0, U, D, P, finishing=True) <= ceil_div(h * U, D), (pair, N)
            assert (N == 0) == (tail == 0)
            # everything a row writes is what the one-shot call writes for it
            if N < 2 ** 50:
                assert known(N, U, D, P) + tail == G.resample_len(N, *pair), (pair, N)


def test_the_incremental_form_agrees_with_the_closed_one_near_2_40_and_2_62(built):
    """the device keeps i = floor(M D / U) and p = M D mod U of the next output M and never multiplies N: started from the
    closed form at a large N (in Python integers) and stepped call by call, the counts are grail_resample_stream_len's,
    and every intermediate stays below 2^44"""
    rng = np.random.default_rng(62)
    for pair in [(48000, 16000), (44100, 48000), (48000, 44100), (8000, 96000), (50, 3), (3, 2)]:
        U, D, P = G.resample_ratio(*pair)
        for N0 in (2 ** 40 - 3, 2 ** 40 + 12345, 2 ** 62 - 100000, 2 ** 62 - 4801):
            N, M = N0, known(N0, U, D, P)
            i, p = M * D // U, M * D % U
            for n in [0, 1, 480, 4800, 0, 7] + [int(v) for v in rng.integers(0, 5000, 6)]:
                if N + n > 2 ** 62 - 1:
                    break
                c, i2, p2 = advance(i, p, N, n, U, D, P)
                assert c == G.resample_stream_len(N, n, *pair), (pair, N, n)
                assert (max(N + n - 1 - P // 2 - i + 1, 0) * U + D) < 2 ** 44 and p + c * D < 2 ** 44
                N, M, i, p = N + n, M + c, i2, p2
                assert (i, p) == (M * D // U, M * D % U) and i < 2 ** 64 and p < U
            assert advance(i, p, N, 0, U, D, P, finishing=True)[0] == G.resample_stream_len(N, 0, *pair, finishing=True)


def test_stream_len_refusals(built):
    lib = G.load()
    out = C.c_uint64(77)
    for N, n, ri, ro, fin in [(5, 1, 0, 8000, 0), (5, 1, 8000, 0, 0), (5, 1, 8000, 8000, 0), (5, 1, 11025, 96000, 0),
                              (5, 1, 48000, 16000, 1),                             # finish feeds nothing
                              (2 ** 64 - 1, 1, 48000, 16000, 0), (2 ** 63, 2 ** 63, 48000, 16000, 0),
                              (0, 2 ** 64 - 1, 8000, 96000, 0)]:                     # 12 outputs a sample: the count outgrows 64 bits
        assert lib.grail_resample_stream_len(N, n, ri, ro, fin, C.addressof(out)) == G.ERR_INVALID_ARG and out.value == 77, (N, n, ri, ro, fin)
    assert lib.grail_resample_stream_len(5, 1, 48000, 16000, 0, None) == G.ERR_INVALID_ARG
    assert lib.grail_resample_stream_len(2 ** 64 - 1, 0, 8000, 96000, 1, C.addressof(out)) == G.OK and out.value == 24 * 12


# ---- the concatenation property --------------------------------------------------------------------------------------------------
def holes(x, at):
    for i, t in enumerate(at):
        if 0 <= t < len(x):
            x[t] = (np.nan, np.inf, -np.inf)[i % 3]
    return x


def local_form(x, num, D, split, cap):
    """The calls as the kernels compute them.  State: N, the next output's input time i and phase p, a ring of `cap` samples
    (sample t at t mod cap, +0.0 where it was not finite).  Per call, local time = global time - N: v below 0 is the ring
    (+0.0 before the row's first sample), the call's samples from 0, +0.0 past them; output r starts at local time
    (i - N) + (p + r D) div U with phase (p + r D) mod U.  -> the calls' outputs and the tail, as stream_model returns them."""
    U, P = num.shape
    h = P // 2
    assert cap >= P - 1 and cap & (cap - 1) == 0
    ring = np.full(cap, np.float32(np.nan))             # (never read before it is written: NaN would show)
    Cf = num.astype(np.float64) / 2.0 ** 26
    st = {"N": 0, "i": 0, "p": 0}

    def call(chunk, finishing):
        N, i, p, n = st["N"], st["i"], st["p"], len(chunk)
        c, i2, p2 = advance(i, p, N, n, U, D, P, finishing)
        lo = P - 1                                          # v[lo + t] is local time t, t = -(P - 1) .. n + h
        v = np.zeros(lo + n + h + 1, np.float64)
        for t in range(-min(P - 1, N), 0):
            v[lo + t] = ring[(N + t) % cap]
        v[lo:lo + n] = np.where(np.isfinite(chunk), chunk, np.float32(0.0))
        off = p + np.arange(c, dtype=np.int64) * D
        t0, ph = (i - N) + off // U, off % U
        acc = np.zeros(c, np.float64)
        for k in range(P):
            acc = acc + Cf[ph, k] * v[lo + t0 + h - k]
        for t in range(max(0, n - cap), n):
            ring[(N + t) % cap] = chunk[t] if np.isfinite(chunk[t]) else np.float32(0.0)
        st.update(N=N + n, i=i2, p=p2)
        return acc.astype(np.float32)

    out, at = [], 0
    for n in split:
        chunk = np.asarray(x[at:at + n], np.float32)
        out.append((call(chunk, False), int(np.count_nonzero(~np.isfinite(chunk)))))
        at += n
    return out, call(np.zeros(0, np.float32), True)


@pytest.mark.parametrize("pair", SMALL)
def test_calls_end_to_end_then_the_tail_are_the_one_shot_row(built, pair):
    """rows up to 3 P + 5 samples under the model's four splits, non-finite samples at the rows' ends, at the cuts and in the
    middle: the model (which asserts E(N), the two bounds and that nothing before N - (P - 1) is needed) and the local
    form, with the ring a stream has and a larger one"""
    rng = np.random.default_rng(500 + pair[0] % 97 + pair[1] % 89)
    U, D, P = G.resample_ratio(*pair)
    num = G.resample_coefficients(*pair)
    h = P // 2
    Ci = ceil_div(64 * D, U)
    cases = 0
    for N in sorted({0, 1, h, h + 1, P - 1, P, 3 * P + 5}):
        for split in splits(N, P, Ci, rng):
            x = rng.uniform(-1.0, 1.0, N).astype(np.float32)
            cuts = np.cumsum(split)
            x = holes(x, [0, N - 1, N // 2] + [c - 1 for c in cuts] + [c for c in cuts])
            whole, n_out, bad = resample_model(x, num, D)
            for what, (calls, tail) in (("model", stream_model(x, num, D, split)),
                                        ("local", local_form(x, num, D, split, ring_capacity(P))),
                                        ("wide ring", local_form(x, num, D, split, 4 * ring_capacity(P)))):
                joined = np.concatenate([y for y, _ in calls] + [tail])
                assert len(joined) == n_out and sum(b for _, b in calls) == bad, (what, pair, N, split)
                assert np.array_equal(bits(joined), bits(whole)), (what, pair, N, split)
            cases += 1
    assert cases >= 4 * 6


# ---- the arguments -------------------------------------------------------------------------------------------------------------
def test_argument_errors_come_before_the_device(built):
    lib = G.load()
    a, b, ln, fake = 0x10000000, 0x20000000, 0x30000000, 0x40000000       # addresses nobody looks behind
    out = C.c_void_p(0x77)
    po = C.addressof(out)
    # open: no context can be NULL (and none exists without a device), no out
    for args in ((None, 48000, 16000, 4, po), (None, 48000, 48000, 4, po), (None, 0, 16000, 4, po), (None, 11025, 96000, 4, po),
                 (None, 48000, 16000, 0, po), (None, 48000, 16000, 4, None)):
        assert lib.grail_resample_stream_open(*args) == G.ERR_INVALID_ARG, args
        assert b"grail_resample_stream_open" in lib.grail_last_error() and out.value == 0x77
    # (without a context the stream is not looked into: the checks run for one row at a ratio of 1 / 1)
    cases = [
        ((None, None, a, 64, ln, b, 64, None, None), b"stream is NULL"),
        ((None, fake, a, 64, None, b, 64, None, None), b"NULL buffer"),
        ((None, fake, None, 64, ln, b, 64, None, None), b"NULL buffer"),
        ((None, fake, a, 64, ln, None, 64, None, None), b"NULL buffer"),
        ((None, fake, None, 0, None, None, 0, None, None), b"NULL buffer"),
        ((None, fake, a, 64, ln, b, 63, None, None), b"never cuts outputs short"),
        ((None, fake, a, 64, ln, b, 0, None, None), b"never cuts outputs short"),
        ((None, fake, a, 64, ln, a, 64, None, None), b"overlaps"),
        ((None, fake, a, 64, ln, a + 4 * 63, 64, None, None), b"overlaps"),
        ((None, fake, a, 64, ln, a - 4 * 127, 128, None, None), b"overlaps"),
        ((None, fake, a, 2 ** 61, ln, 2 ** 63, 2 ** 61, None, None), b"2^60"),
    ]
    for args, word in cases:
        assert lib.grail_resample_stream_next_async(*args) == G.ERR_INVALID_ARG, args
        assert word in lib.grail_last_error(), (args, lib.grail_last_error())
    assert lib.grail_resample_stream_finish_async(None, None, None, b, 64, None) == G.ERR_INVALID_ARG
    assert b"stream is NULL" in lib.grail_last_error()
    assert lib.grail_resample_stream_finish_async(None, fake, None, b, 0, None) == G.ERR_INVALID_ARG
    assert b"longest tail" in lib.grail_last_error()
    assert lib.grail_resample_stream_finish_async(None, fake, None, None, 64, None) == G.ERR_INVALID_ARG
    assert b"NULL buffer" in lib.grail_last_error()
    assert lib.grail_resample_stream_close(None, fake) == G.ERR_INVALID_ARG and lib.grail_resample_stream_close(None, None) == G.OK
    if G.device_count() == 0:        # no context can exist: the valid calls say why, they do not compute on the CPU
        assert lib.grail_resample_stream_next_async(None, fake, a, 64, ln, b, 64, None, None) == G.ERR_NO_DEVICE
        assert b"no usable HIP device" in lib.grail_last_error()
        assert lib.grail_resample_stream_next_async(None, fake, None, 0, ln, None, 0, None, None) == G.ERR_NO_DEVICE
        assert lib.grail_resample_stream_finish_async(None, fake, None, b, 64, None) == G.ERR_NO_DEVICE


def test_header_python_and_rust_name_the_same_functions(built):
    hdr = open(os.path.join(ROOT, "include", "grail_hip.h")).read()
    assert "levels, continued: sample-rate conversion of streams" in hdr
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(set(re.findall(r"\b(grail_resample_stream_[a-z0-9_]+)\s*\(", code))) == FUNCTIONS
    assert "typedef struct grail_resample_stream grail_resample_stream;" in code
    assert sorted(n for n in G.EXPORTS if n.startswith("grail_resample_stream")) == FUNCTIONS
    sys_rs = open(os.path.join(ROOT, "grail-rs_amd", "rust", "grail-hip-sys", "src", "lib.rs")).read()
    assert sorted(set(re.findall(r"pub fn (grail_resample_stream_[a-z0-9_]+)\s*\(", sys_rs))) == FUNCTIONS
    assert "pub struct grail_resample_stream {" in sys_rs
    safe_rs = open(os.path.join(ROOT, "grail-rs_amd", "rust", "grail-hip", "src", "lib.rs")).read()
    for name in FUNCTIONS:
        assert "sys::" + name + "(" in safe_rs, name
    lib = G.load()
    assert lib.grail_abi_version() == G.ABI_VERSION == 4
    for name in FUNCTIONS:
        assert hasattr(lib, name), name


# ---- the launch arithmetic -----------------------------------------------------------------------------------------------------
def test_the_gpu_files_pairs_and_layouts_start_every_instantiation():
    """launch_resample_stream chooses <STAGED, VEC, TAB> by launch_resample's arithmetic (the chunk is the same), which
    test_resample_gpu.py's variant() mirrors: the pairs of the every-split test run aligned (16-byte loads and stores), the
    layout test runs its pairs aligned, one float off and on odd strides; together they start all ten instantiations"""
    started = set()
    for pair in GPU.PAIRS:
        started.add(variant(*G.resample_ratio(*pair), aligned=True))
    for pair in GPU.LAYOUT_PAIRS:
        U, D, P = G.resample_ratio(*pair)
        started |= {variant(U, D, P, aligned=True), variant(U, D, P, aligned=False)}
    assert started == set(VARIANTS) and len(VARIANTS) == 10
    # ... and the issue's three layout pairs are among them, on three different ways to the coefficients
    assert {variant(*G.resample_ratio(*pair), aligned=False) for pair in [(48000, 16000), (44100, 48000), (50, 3)]} == \
        {("staged", False, "uniform"), ("staged", False, "lds"), ("unstaged", False, "global")}
    assert set(GPU.LAYOUT_PAIRS) >= {(48000, 16000), (44100, 48000), (50, 3)}


def test_interactive_example_knows_the_rate_option(built):
    import subprocess
    exe = os.path.join(ROOT, "grail-rs_amd", "lib", "grail_interactive")
    for bad in (["--rate"], ["--rate", "0"], ["--rate", "x"], ["--rate", "-8000"], ["--rate", "44100"],     # (44100 is the voice's own)
                ["--rate", "7"], ["--rote", "8000"]):
        r = subprocess.run([exe] + bad, input=b"a\n", capture_output=True, text=False)
        assert r.returncode == 2 and b"[--rate R]" in r.stderr, (bad, r.stderr)
    if G.device_count() == 0:
        r = subprocess.run([exe, "--band", "300", "3400", "--rate", "8000", "441", "0.1"], input=b"a\n", capture_output=True)
        assert r.returncode == 1 and b"no HIP device" in r.stderr
