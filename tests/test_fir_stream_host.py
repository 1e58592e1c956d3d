"""Filter streams (include/grail_hip.h, "levels, continued: FIR filtering of streams") without a GPU: grail_filter_stream_len
against the numpy model of tests/fir_stream_model.py; the model's concatenation property against tests/fir_model.py (the
calls' outputs end to end, then the tail, are the one-shot row, bit for bit, whatever the split), also in the frame of one
call that the kernel works in (a ring of the last samples, the origin max(0, o - N)); and the argument errors of the four
calls, which come before the device is asked for."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import grail_hip as G
from fir_model import cancelling_taps, fir_model, steps
from fir_stream_model import known, splits, stream_len, stream_model
from test_fir_gpu import origins, random_taps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ["grail_filter_stream_close", "grail_filter_stream_finish_async", "grail_filter_stream_len",
             "grail_filter_stream_next_async", "grail_filter_stream_open"]


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def ring_capacity(longest_taps):
    """the samples of a row's ring: the longest K - 1 rounded up to a power of two, at least 1"""
    cap = 1
    while cap < longest_taps - 1:
        cap *= 2
    return cap


# ---- the length ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 8, 9, 4096])
def test_stream_len_agrees_with_the_model(built, K):
    for o in origins(K):
        for N in sorted({0, 1, max(o - 1, 0), o, o + 1, o + K, 2 ** 40}):          # N straddling o
            for n in (0, 1, 2, o, o + 1, K, 4800):
                assert G.fir_stream_len(N, n, K, o) == stream_len(N, n, K, o) <= n, (K, o, N, n)
                # fed in two calls or in one: the same outputs
                assert G.fir_stream_len(N, n, K, o) + G.fir_stream_len(N + n, 7, K, o) == G.fir_stream_len(N, n + 7, K, o)
            tail = G.fir_stream_len(N, 0, K, o, finishing=True)
            assert tail == stream_len(N, 0, K, o, finishing=True) == (0 if N == 0 else K - 1 - o + min(N, o)) <= K - 1
            # everything a row writes is what the one-shot call writes for it
            assert known(N, o) + tail == G.fir_len(N, K, o), (K, o, N)


def test_stream_len_refuses_what_fir_len_refuses(built):
    lib = G.load()
    out = C.c_uint64(77)
    for N, n, K, o, fin in [(5, 1, 0, 0, 0), (5, 1, 4097, 0, 0), (5, 1, 9, 9, 0), (5, 1, 1, 1, 1), (2 ** 64 - 1, 1, 2, 0, 0),
                            (2 ** 64 - 4095, 0, 4096, 0, 0), (2 ** 64 - 4095, 0, 4096, 0, 1), (2 ** 63, 2 ** 63, 1, 0, 0),
                            (5, 1, 9, 4, 1)]:                                        # (the last: finish feeds nothing)
        assert lib.grail_filter_stream_len(N, n, K, o, fin, C.addressof(out)) == G.ERR_INVALID_ARG and out.value == 77, (N, n, K, o, fin)
    assert lib.grail_filter_stream_len(5, 1, 9, 4, 0, None) == G.ERR_INVALID_ARG
    assert lib.grail_filter_stream_len(2 ** 64 - 4096, 0, 4096, 0, 1, C.addressof(out)) == G.OK and out.value == 4095


# ---- the concatenation property --------------------------------------------------------------------------------------------------
def holes(x, at):
    for i, t in enumerate(at):
        if 0 <= t < len(x):
            x[t] = (np.nan, np.inf, -np.inf)[i % 3]
    return x


def local_form(x, h, origin, split, cap):
    """The calls as the kernel computes them: per call, local time = global time - N; output r is the left fold of
    h[k] * v[r + d - k] with d = max(0, origin - N); v below 0 is a ring of `cap` samples (sample t at t mod cap, +0.0 where
    it was not finite, +0.0 before the row's first sample), the call's samples from 0, +0.0 past them.  -> the calls'
    outputs and the tail, as stream_model returns them."""
    K = len(h)
    assert cap >= max(K - 1, 1) and cap & (cap - 1) == 0
    ring = np.full(cap, np.float32(np.nan))             # (never read before it is written: NaN would show)
    N, out = 0, []

    def call(chunk, count):
        n = len(chunk)
        d = max(0, origin - N)
        v = np.zeros(K - 1 + n + K, np.float64)         # local times -(K - 1) .. n + K - 1
        for t in range(-min(K - 1, N), 0):
            v[K - 1 + t] = ring[(N + t) % cap]
        v[K - 1:K - 1 + n] = np.where(np.isfinite(chunk), chunk, np.float32(0.0))
        acc = np.zeros(count, np.float64)
        for k in range(K):
            at = K - 1 + d - k
            acc = acc + np.float64(h[k]) * v[at:at + count]
        with np.errstate(over="ignore"):
            return acc.astype(np.float32)

    at = 0
    for n in split:
        chunk = np.asarray(x[at:at + n], np.float32)
        y = call(chunk, stream_len(N, n, K, origin))
        bad = int(np.count_nonzero(~np.isfinite(chunk)))
        for t in range(max(0, n - cap), n):
            ring[(N + t) % cap] = chunk[t] if np.isfinite(chunk[t]) else np.float32(0.0)
        out.append((y, bad))
        N, at = N + n, at + n
    return out, call(np.zeros(0, np.float32), stream_len(N, 0, K, origin, finishing=True))


@pytest.mark.parametrize("K", [1, 2, 8, 9, 17, 40])
def test_calls_end_to_end_then_the_tail_are_the_one_shot_row(built, K):
    """for every origin and a range of totals: every split, with non-finite samples at the rows' ends, at the cuts and in
    the middle; the model and the local form (with the ring a stream of this filter alone would have, and a larger one)"""
    rng = np.random.default_rng(500 + K)
    cases = 0
    for o in origins(K):
        for N in sorted({0, 1, max(K - 1, 0), K, 3 * K + 5, 150}):
            for split in splits(N, K, 64, rng):
                x = rng.uniform(-1.0, 1.0, N).astype(np.float32)
                cuts = np.cumsum(split)
                x = holes(x, [0, N - 1, N // 2] + [c - 1 for c in cuts] + [c for c in cuts])
                h = random_taps(K, rng)
                whole, n_out, bad = fir_model(x, h, o)
                for what, (calls, tail) in (("model", stream_model(x, h, o, split)),
                                            ("local", local_form(x, h, o, split, ring_capacity(K))),
                                            ("wide ring", local_form(x, h, o, split, 4 * ring_capacity(K)))):
                    joined = np.concatenate([y for y, _ in calls] + [tail])
                    assert len(joined) == n_out and sum(b for _, b in calls) == bad, (what, K, o, N, split)
                    assert np.array_equal(bits(joined), bits(whole)), (what, K, o, N, split)
                cases += 1
    assert cases >= 4 * 4 * len(origins(K))


def test_the_order_of_the_fold_survives_the_split(built):
    """cancelling taps on steps of equal samples: the low bits depend on the order the products were added in, so a local
    form that folded the ring's part and the chunk's part apart would differ here"""
    rng = np.random.default_rng(7)
    for K in (9, 40, 255):
        h, o = cancelling_taps(K, rng), (K - 1) // 2
        x = steps(1500, rng)
        whole, n_out, _ = fir_model(x, h, o)
        two_chains = (fir_model(x, np.where(np.arange(K) % 2 == 0, h, np.float32(0.0)), o)[0].astype(np.float64) +
                      fir_model(x, np.where(np.arange(K) % 2 == 1, h, np.float32(0.0)), o)[0].astype(np.float64)).astype(np.float32)
        assert np.count_nonzero(bits(two_chains) != bits(whole)) > 0.02 * n_out          # the content shows the order
        for split in splits(1500, K, 480, rng):
            for calls, tail in (stream_model(x, h, o, split), local_form(x, h, o, split, ring_capacity(K))):
                joined = np.concatenate([y for y, _ in calls] + [tail])
                assert np.array_equal(bits(joined), bits(whole)), (K, split)


# ---- the arguments -------------------------------------------------------------------------------------------------------------
def test_argument_errors_come_before_the_device(built):
    lib = G.load()
    a, b, ln, fake, fset = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000       # addresses nobody looks behind
    out = C.c_void_p(0x77)
    po = C.addressof(out)
    which = np.zeros(4, np.uint32)
    # open: no context can be NULL (and none exists without a device), no out
    for args in ((None, fset, 4, which.ctypes.data, po), (None, fset, 4, None, po), (None, None, 4, None, po), (None, fset, 0, None, po),
                 (None, fset, 4, None, None)):
        assert lib.grail_filter_stream_open(*args) == G.ERR_INVALID_ARG, args
        assert b"grail_filter_stream_open" in lib.grail_last_error() and out.value == 0x77
    cases = [
        ((None, None, a, 64, ln, b, 64, None, None), b"stream is NULL"),
        ((None, fake, a, 64, None, b, 64, None, None), b"NULL buffer"),
        ((None, fake, None, 64, ln, b, 64, None, None), b"NULL buffer"),
        ((None, fake, a, 64, ln, None, 64, None, None), b"NULL buffer"),
        ((None, fake, a, 64, ln, b, 63, None, None), b"out_stride < in_stride"),
        ((None, fake, a, 64, ln, b, 0, None, None), b"out_stride < in_stride"),
        ((None, fake, a, 64, ln, a, 64, None, None), b"overlaps"),
        ((None, fake, a, 64, ln, a + 4 * 63, 64, None, None), b"overlaps"),
        ((None, fake, a, 64, ln, a - 4 * 127, 128, None, None), b"overlaps"),
        ((None, fake, a, 2 ** 61, ln, 2 ** 63, 2 ** 61, None, None), b"2^60"),
    ]
    for args, word in cases:
        assert lib.grail_filter_stream_next_async(*args) == G.ERR_INVALID_ARG, args
        assert word in lib.grail_last_error(), (args, lib.grail_last_error())
    assert lib.grail_filter_stream_finish_async(None, None, None, b, 64, None) == G.ERR_INVALID_ARG
    assert b"stream is NULL" in lib.grail_last_error()
    assert lib.grail_filter_stream_close(None, fake) == G.ERR_INVALID_ARG and lib.grail_filter_stream_close(None, None) == G.OK
    if G.device_count() == 0:        # no context can exist: the valid calls say why, they do not compute on the CPU
        assert lib.grail_filter_stream_next_async(None, fake, a, 64, ln, b, 64, None, None) == G.ERR_NO_DEVICE
        assert b"no usable HIP device" in lib.grail_last_error()
        assert lib.grail_filter_stream_next_async(None, fake, None, 0, ln, None, 0, None, None) == G.ERR_NO_DEVICE
        assert lib.grail_filter_stream_finish_async(None, fake, None, b, 64, None) == G.ERR_NO_DEVICE
        assert lib.grail_filter_stream_finish_async(None, fake, None, None, 0, None) == G.ERR_NO_DEVICE


def test_header_python_and_rust_name_the_same_functions(built):
    hdr = open(os.path.join(ROOT, "include", "grail_hip.h")).read()
    assert "levels, continued: FIR filtering of streams" in hdr
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(set(re.findall(r"\b(grail_filter_stream_[a-z0-9_]+)\s*\(", code))) == FUNCTIONS
    assert sorted(n for n in G.EXPORTS if n.startswith("grail_filter_stream")) == FUNCTIONS
    sys_rs = open(os.path.join(ROOT, "grail-rs_amd", "rust", "grail-hip-sys", "src", "lib.rs")).read()
    assert sorted(set(re.findall(r"pub fn (grail_filter_stream_[a-z0-9_]+)\s*\(", sys_rs))) == FUNCTIONS
    lib = G.load()
    assert lib.grail_abi_version() == G.ABI_VERSION == 4
    for name in FUNCTIONS:
        assert hasattr(lib, name), name


def test_interactive_example_knows_the_band_option(built):
    import subprocess
    exe = os.path.join(ROOT, "grail-rs_amd", "lib", "grail_interactive")
    for bad in (["--band", "300"], ["--band", "3400", "300"], ["--band", "-1", "300"], ["--band", "x", "300"],
                ["--band", "300", "3400", "--taps", "254"], ["--band", "300", "3400", "--taps", "1"], ["--band", "300", "3400", "--taps", "4097"],
                ["--taps", "255"], ["--bend", "300", "3400"], ["441", "1", "2"]):
        r = subprocess.run([exe] + bad, input=b"a\n", capture_output=True, text=False)
        assert r.returncode == 2 and b"[--band LO HI [--taps K]]" in r.stderr, bad
    if G.device_count() == 0:
        r = subprocess.run([exe, "--band", "300", "3400", "441", "0.1"], input=b"a\n", capture_output=True)
        assert r.returncode == 1 and b"no HIP device" in r.stderr


def test_every_line_of_the_stream_kernels_census_names_a_test_that_exists():
    """tests/KERNEL_PATHS_FIR_STREAM.md: every row names, in its last column, test ids `file.py::name` that exist"""
    with open(os.path.join(ROOT, "tests", "KERNEL_PATHS_FIR_STREAM.md")) as f:
        rows = [line for line in f if line.startswith("|") and not re.match(r"\|\s*(-+|kernel)\s*\|", line)]
    assert len(rows) >= 8
    for line in rows:
        ids = re.findall(r"`(test_\w+\.py)::(test_\w+)", line.rstrip().rstrip("|").split("|")[-1])
        assert ids, "a line without a test id: " + line
        for name, test in ids:
            with open(os.path.join(ROOT, "tests", name)) as src:
                assert re.search(r"^def " + test + r"\(", src.read(), flags=re.M), (name, test)
