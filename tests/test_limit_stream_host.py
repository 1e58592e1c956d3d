"""Limit streams (include/grail_hip.h, "levels, continued: the limiter on streams") without a GPU: the claims of the numpy
model of tests/limit_stream_model.py that tests/test_limit_stream_gpu.py holds the device to (E(N) and that it is tight, the
calls and the tail end to end are the one-shot row, the per-call results combine to its results, nothing before N - 3 L - 19
is needed, the tail against fed zeros), grail_limit_stream_len, every argument refusal ahead of the missing device,
the signatures in the header, the Python package and the Rust crates, and the example's usage."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import grail_hip as G
from limit_stream_model import (LIMIT_CHUNK, bits, check_against_one_shot, delay, known, ring_capacity, splits, stream_len,
                                stream_model)
from test_limiter_host import limiter_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = sorted(["grail_limit_stream_len", "grail_limit_stream_open", "grail_limit_stream_next_async",
                    "grail_limit_stream_finish_async", "grail_limit_stream_close"])
CEILING = np.float32(0.5)


# ---- the model's own claims --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ell", [0, 1, 3, 5, 8])
def test_calls_end_to_end_then_the_tail_are_the_one_shot_row(ell):
    """rows of noise above the ceiling with holes, alone and as a linked pair, under the model's splits: check_against_one_shot
    asserts the concatenation, the combined results and (in stream_model) that nothing before N - 3 L - 19 is needed"""
    L, lam = 1 << ell, delay(ell)
    rng = np.random.default_rng(600 + ell)
    cases = 0
    for N in sorted({0, 1, lam - 1, lam, lam + 1, 4 * L + 150}):
        x = rng.uniform(-0.6, 0.6, N).astype(np.float32)
        y = rng.uniform(-0.6, 0.6, N).astype(np.float32)
        for t in (0, N // 2, N - 1):
            if 0 <= t < N:
                x[t] = (np.nan, np.inf, -np.inf)[t % 3]
        for split in splits(N, L, rng):
            calls, tail = check_against_one_shot([x], CEILING, ell, split)
            assert [len(c[0][0]) for c in calls] == [stream_len(sum(split[:k]), n, ell) for k, n in enumerate(split)]
            check_against_one_shot([x, y], CEILING, ell, split)
            cases += 1
    assert cases == 6 * 5


def test_a_split_around_a_chunk_of_outputs():
    """the splits aim at GRAIL_LIMIT_CHUNK: a call of one output less than a chunk, then one across the seam; a call of one more"""
    rng = np.random.default_rng(610)
    ell, N = 3, 2 * LIMIT_CHUNK + 37
    x = rng.uniform(-0.6, 0.6, N).astype(np.float32)
    found = [[len(c[0][0]) for c in check_against_one_shot([x], CEILING, ell, s)[0]] for s in splits(N, 1 << ell, rng)]
    assert found[0] == [N - delay(ell)] and found[2][:2] == [LIMIT_CHUNK - 1, 2] and found[3][0] == LIMIT_CHUNK + 1
    assert found[1][:4] == [0, 1, delay(ell) + 1, 0] and 0 in found[4]
    assert LIMIT_CHUNK == G.LIMIT_CHUNK


@pytest.mark.parametrize("ell", [0, 1, 3, 5, 8])
def test_known_outputs_are_final_and_the_bound_is_tight(ell):
    """outputs below E(N) do not change with what is fed later, whatever it is; output N - LAMBDA does change with sample N for
    some row: a quiet row followed by one loud sample"""
    L, lam = 1 << ell, delay(ell)
    rng = np.random.default_rng(620 + ell)
    N = 3 * L + 40
    x = rng.uniform(-0.3, 0.3, N + lam + 5).astype(np.float32)
    x[N] = 30.0
    before = limiter_model([x[:N]], CEILING, ell)[0][0]
    for more in (1, 2, lam, lam + 5):
        after = limiter_model([x[:N + more]], CEILING, ell)[0][0]
        assert np.array_equal(bits(before[:known(N, ell)]), bits(after[:known(N, ell)])), more
    after = limiter_model([x[:N + 1]], CEILING, ell)[0][0]
    assert bits(before[N - lam]) != bits(after[N - lam])                    # E(N) is tight
    assert known(N, ell) == N - lam and known(lam, ell) == 0 and known(lam + 1, ell) == 1
    # ... and the oldest sample a later output needs is no older than N - 3 L - 19: the ring holds that many
    assert ring_capacity(ell) >= 3 * L + 19 > ring_capacity(ell) // 2 or ell == 0
    assert ring_capacity(ell) & (ring_capacity(ell) - 1) == 0


@pytest.mark.parametrize("ell", [0, 5, 8])
def test_the_tail_against_fed_zeros(ell):
    """The row's end: q[s] = Q for s >= N, the samples to come +0.0 in the detector.  After the last sample the e's are not
    zero, and a fed zero gets their q where the row's end gets Q; the issue behind this test expected the tail to differ from
    what feeding LAMBDA zeros and cutting gives.  It does not, and cannot: q[N + k] sees only e's that q[N - 1] sees as well
    (e[N + k .. N + 10]; the rest are +0.0), so q[N + k] >= q[N - 1], and every window under an output t < N that reaches past
    the end holds q[N - 1].  So the q's do differ and the outputs never do.  Both are asserted, and that the loud samples at
    the end are what shapes the tail (the case is not vacuous)."""
    lam = delay(ell)
    rng = np.random.default_rng(630 + ell)
    n = 3 * lam + 20
    quiet = rng.uniform(-0.02, 0.02, n).astype(np.float32)
    x = quiet.copy()
    x[[n - 1, n - 12]] = 0.9
    _, tail = stream_model([x], CEILING, ell, [n])
    zeros = np.zeros(lam, np.float32)
    out, _, _, _, ((q_padded, _, _),) = limiter_model([np.concatenate([x, zeros])], CEILING, ell, curves=True)
    assert np.all(q_padded[n:n + 5] < 1 << 24) and np.all(q_padded[n:] >= q_padded[n - 1])     # where the row's end has Q
    assert len(tail[0][0]) == lam and np.array_equal(bits(tail[0][0]), bits(out[0][n - lam:n]))
    _, quiet_tail = stream_model([quiet], CEILING, ell, [n])
    assert tail[2] > 0 and quiet_tail[2] == 0 and tail[1] < 0.6 and quiet_tail[1] == 1


# ---- grail_limit_stream_len ---------------------------------------------------------------------------------------------------
def test_stream_len_against_the_model_and_its_refusals(built):
    for ell in range(11):
        lam = delay(ell)
        assert G.limit_stream_delay(ell) == lam
        for fed in (0, 1, lam - 1, lam, lam + 1, 5000, 2 ** 40, 2 ** 64 - 1 - 4096):
            for n in (0, 1, lam, lam + 1, 4096):
                assert G.limit_stream_len(fed, n, ell) == stream_len(fed, n, ell), (ell, fed, n)
            assert G.limit_stream_len(fed, 0, ell, finishing=True) == stream_len(fed, 0, ell, finishing=True) == min(fed, lam)
    assert G.limit_stream_len(0, 2 ** 64 - 1, 10) == 2 ** 64 - 1 - 1034 and G.limit_stream_len(2 ** 64 - 2, 1, 0) == 1
    lib = G.load()
    out = C.c_uint64(77)
    po = C.addressof(out)
    for args in ((0, 10, 11, 0, po), (0, 10, 0xFFFFFFFF, 0, po), (0, 10, 8, 0, None), (100, 1, 8, 1, po), (2 ** 64 - 1, 1, 8, 0, po),
                 (2 ** 63, 2 ** 63, 8, 0, po)):
        assert lib.grail_limit_stream_len(*args) == G.ERR_INVALID_ARG and out.value == 77, args
    with pytest.raises(G.GrailError):
        G.limit_stream_len(0, 1, 8, finishing=True)


# ---- the arguments -------------------------------------------------------------------------------------------------------------
def test_argument_errors_come_before_the_device(built):
    lib = G.load()
    a, b, ln, fake = 0x10000000, 0x20000000, 0x30000000, 0x40000000       # addresses nobody looks behind
    out = C.c_void_p(0x77)
    po = C.addressof(out)
    # open: what grail_limit_async refuses, n_rows = 0, no out; no context can be NULL (and none exists without a device)
    words = [((None, 4, 1, 0.5, 11, po), b"lookahead_log2"), ((None, 4, 0, 0.5, 8, po), b"multiple of group"),
             ((None, 4, 3, 0.5, 8, po), b"multiple of group"), ((None, 4, 1, 0.0, 8, po), b"ceiling"),
             ((None, 4, 1, -0.5, 8, po), b"ceiling"), ((None, 4, 1, float("nan"), 8, po), b"ceiling"),
             ((None, 4, 1, float("inf"), 8, po), b"ceiling"), ((None, 0, 1, 0.5, 8, po), b"n_rows is 0"),
             ((None, 4, 2, 0.5, 8, None), b"NULL argument"), ((None, 4, 2, 0.5, 8, po), b"NULL argument")]
    for args, word in words:
        assert lib.grail_limit_stream_open(*args) == G.ERR_INVALID_ARG, args
        assert b"grail_limit_stream_open" in lib.grail_last_error() and word in lib.grail_last_error() and out.value == 0x77, args
    # (without a context the stream is not looked into: the checks run for one row alone)
    nothing = (None, None, None, None)
    cases = [
        ((None, None, a, 64, ln, b, 64) + nothing, b"stream is NULL"),
        ((None, fake, a, 64, None, b, 64) + nothing, b"NULL buffer"),
        ((None, fake, None, 64, ln, b, 64) + nothing, b"NULL buffer"),
        ((None, fake, a, 64, ln, None, 64) + nothing, b"NULL buffer"),
        ((None, fake, None, 0, None, None, 0) + nothing, b"NULL buffer"),
        ((None, fake, a, 64, ln, b, 63) + nothing, b"never cuts outputs short"),
        ((None, fake, a, 64, ln, b, 0) + nothing, b"never cuts outputs short"),
        ((None, fake, a, 64, ln, a, 64) + nothing, b"overlaps"),
        ((None, fake, a, 64, ln, a + 4 * 63, 64) + nothing, b"overlaps"),
        ((None, fake, a, 64, ln, a - 4 * 127, 128) + nothing, b"overlaps"),
        ((None, fake, a, 2 ** 61, ln, 2 ** 63, 2 ** 61) + nothing, b"2^60"),
    ]
    for args, word in cases:
        assert lib.grail_limit_stream_next_async(*args) == G.ERR_INVALID_ARG, args
        assert word in lib.grail_last_error(), (args, lib.grail_last_error())
    assert lib.grail_limit_stream_finish_async(None, None, None, b, 64, None, None, None) == G.ERR_INVALID_ARG
    assert b"stream is NULL" in lib.grail_last_error()
    assert lib.grail_limit_stream_finish_async(None, fake, None, b, 10, None, None, None) == G.ERR_INVALID_ARG
    assert b"delay" in lib.grail_last_error()
    assert lib.grail_limit_stream_finish_async(None, fake, None, None, 64, None, None, None) == G.ERR_INVALID_ARG
    assert b"NULL buffer" in lib.grail_last_error()
    assert lib.grail_limit_stream_close(None, fake) == G.ERR_INVALID_ARG and lib.grail_limit_stream_close(None, None) == G.OK
    if G.device_count() == 0:        # no context can exist: the valid calls say why, they do not compute on the CPU
        assert lib.grail_limit_stream_next_async(None, fake, a, 64, ln, b, 64, None, None, None, None) == G.ERR_NO_DEVICE
        assert b"no usable HIP device" in lib.grail_last_error()
        assert lib.grail_limit_stream_next_async(None, fake, None, 0, ln, None, 0, None, None, None, None) == G.ERR_NO_DEVICE
        assert lib.grail_limit_stream_finish_async(None, fake, None, b, 11, None, None, None) == G.ERR_NO_DEVICE


def test_header_python_and_rust_name_the_same_functions(built):
    hdr = open(os.path.join(ROOT, "include", "grail_hip.h")).read()
    assert "levels, continued: the limiter on streams" in hdr
    assert hdr.index("levels, continued: sample-rate conversion of streams") < hdr.index("levels, continued: the limiter on streams")
    assert "#define GRAIL_LIMIT_STREAM_DELAY(l) ((1u << (l)) + 10u)" in hdr
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(set(re.findall(r"\b(grail_limit_stream_[a-z0-9_]+)\s*\(", code))) == FUNCTIONS
    assert "typedef struct grail_limit_stream grail_limit_stream;" in code
    assert sorted(n for n in G.EXPORTS if n.startswith("grail_limit_stream")) == FUNCTIONS
    sys_rs = open(os.path.join(ROOT, "grail-rs_amd", "rust", "grail-hip-sys", "src", "lib.rs")).read()
    assert sorted(set(re.findall(r"pub fn (grail_limit_stream_[a-z0-9_]+)\s*\(", sys_rs))) == FUNCTIONS
    assert "pub struct grail_limit_stream {" in sys_rs
    safe_rs = open(os.path.join(ROOT, "grail-rs_amd", "rust", "grail-hip", "src", "lib.rs")).read()
    facade = open(os.path.join(ROOT, "include", "grail.hpp")).read()
    for name in FUNCTIONS:
        assert "sys::" + name + "(" in safe_rs, name
        assert name + "(" in facade or name == "grail_limit_stream_len", name
    lib = G.load()
    assert lib.grail_abi_version() == G.ABI_VERSION == 4                    # additive: the version stays
    for name, n_args in zip(FUNCTIONS, (2, 8, 5, 11, 6)):
        assert len(getattr(lib, name).argtypes) == n_args, name
    assert hasattr(G, "LimitStream") and hasattr(G.Context, "limit_stream_open")


def test_interactive_example_knows_the_ceiling_option(built):
    exe = os.path.join(ROOT, "grail-rs_amd", "lib", "grail_interactive")
    for bad in (["--ceiling"], ["--ceiling", "x"], ["--ceiling", "nan"], ["--ceiling", "-6", "--lookahead", "11"],
                ["--ceiling", "-6", "--lookahead", "-1"], ["--ceiling", "-6", "--lookahead", "x"], ["--lookahead", "8"],
                ["--cieling", "-6"]):
        r = subprocess.run([exe] + bad, input=b"a\n", capture_output=True, text=False)
        assert r.returncode == 2 and b"[--ceiling DB [--lookahead l]]" in r.stderr, (bad, r.stderr)
    if G.device_count() == 0:
        r = subprocess.run([exe, "--band", "300", "3400", "--ceiling", "-6", "--lookahead", "8", "--rate", "8000", "441", "0.1"],
                           input=b"a\n", capture_output=True)
        assert r.returncode == 1 and b"no HIP device" in r.stderr
