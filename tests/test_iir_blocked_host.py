"""Recursive filtering parallel in time (include/grail_hip.h, "levels, continued: recursive filtering, parallel in time")
without a GPU: grail_biquad_block_matrix against the numpy model of tests/iir_blocked_model.py bit for bit and its refusals; the
blocked model against the serial one (tests/iir_model.py) on filters that do not decay within a block: within 1e-9 of the
serial output's peak before the rounding to binary32 (the rounding of the entry states is all that parts them: some fifty
times what they differed by when the contract was written, 2.1e-11 at a block of 256), identical over every row's first
block and over rows of at most one block; the header, the binding and the -sys crate name the call; grail_dialogue knows
--eq-blocked and refuses it alone."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import grail_hip as G
import iir_blocked_model as BM
import iir_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATE = 44100
N = 150_000
BOUND = 1e-9                    # of the serial output's peak, before the rounding to binary32
DC_BLOCKER = [1.0, -1.0, 0.0, -0.9995, 0.0]


def bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def butterworth(kind, f0, m):
    return [G.iir_design(kind, RATE, f0, 1.0 / (2.0 * math.cos(math.pi * (2 * k + 1) / (4 * m)))) for k in range(m)]


def hard_filters():
    """filters whose memory is longer than any block: (name, sections)"""
    return [("100 Hz high-pass", [G.iir_design(G.IIR_HIGHPASS, RATE, 100.0, 0.7071067811865476)]),
            ("8th-order 20 Hz Butterworth high-pass", butterworth(G.IIR_HIGHPASS, 20.0, 4)),
            ("50 Hz notch, Q = 30", [G.iir_design(G.IIR_NOTCH, RATE, 50.0, 30.0)]),
            ("high-pass, then a 3 kHz peak", [G.iir_design(G.IIR_HIGHPASS, RATE, 100.0, 0.7071067811865476),
                                              G.iir_design(G.IIR_PEAK, RATE, 3000.0, 1.5, 4.0)]),
            ("16th-order 3.4 kHz low-pass", butterworth(G.IIR_LOWPASS, 3400.0, 8)),
            ("DC blocker, pole at 0.9995", [DC_BLOCKER]),
            ("pole at 0.999999", [[1.0, 0.0, 0.0, -0.999999, 0.0]])]


def signals():
    rng = np.random.default_rng(1)
    t = np.arange(N)
    return [("noise", (rng.standard_normal(N) * 0.25).astype(np.float32)),
            ("DC + 50 Hz", (0.5 + 0.4 * np.sin(2.0 * np.pi * 50.0 * t / RATE)).astype(np.float32))]


@pytest.fixture(scope="module")
def both(built):
    """every filter on every signal through the serial model and through the blocked one, before the rounding: computed once"""
    filters = hard_filters()
    rows, which, names = [], [], []
    for f, (fname, _) in enumerate(filters):
        for sname, x in signals():
            rows.append(x)
            which.append(f)
            names.append((fname, sname))
    sections = [np.array(sec) for _, sec in filters]
    serial = M.iir_model(rows, sections, which, exact=True)
    blocked = BM.iir_blocked_model(rows, sections, which, exact=True)
    return names, serial, blocked


# ---- the matrix -------------------------------------------------------------------------------------------------------------
def matrix_filters():
    return [[G.iir_design(G.IIR_HIGHPASS, 48000, 100.0, 0.7071067811865476)],
            [G.iir_design(G.IIR_HIGHPASS, 44100, 100.0, 0.7071067811865476), G.iir_design(G.IIR_PEAK, 44100, 3000.0, 1.5, 4.0)],
            butterworth(G.IIR_LOWPASS, 2000.0, 3),
            butterworth(G.IIR_LOWPASS, 3400.0, 8),
            [DC_BLOCKER]]


def test_block_matrix_is_the_models_bit_for_bit(built):
    assert [len(f) for f in matrix_filters()] == [1, 2, 3, 8, 1]
    for sec in matrix_filters():
        got, want = G.iir_block_matrix(np.array(sec)), BM.block_matrix(np.array(sec))
        S = len(sec)
        assert got.shape == want.shape == (2 * S, 2 * S)
        assert np.array_equal(bits(got), bits(want)), (S, np.flatnonzero(bits(got) != bits(want))[:8])
        # a state is reached from its own section and from those before it, from no later one
        for i in range(2 * S):
            assert np.all(got[i, 2 * (i // 2) + 2:] == 0.0), (S, i)
    # the DC blocker: s1 decays by its pole a step, s2 is never fed
    T = G.iir_block_matrix(DC_BLOCKER)
    p = 1.0
    for _ in range(G.IIR_BLOCK):
        p = -(-0.9995 * p)
    assert T[0, 0] == p and T[1, 0] == 0.0 and T[1, 1] == 0.0 and G.IIR_BLOCK == BM.BLOCK == 1024


def test_block_matrix_refusals(built):
    lib = G.load()
    coef = np.linspace(-0.9, 0.9, 45)
    out = np.full(18 * 18, 77.0)
    for c, S, m in [(None, 1, out), (coef, 1, None), (coef, 0, out), (coef, 9, out), (coef, 0xFFFFFFFF, out)]:
        rc = lib.grail_biquad_block_matrix(None if c is None else c.ctypes.data, S, None if m is None else m.ctypes.data)
        assert rc == G.ERR_INVALID_ARG and np.all(out == 77.0), S
    for at, what in ((0, np.nan), (9, np.inf), (14, -np.inf)):
        bad = coef.copy()
        bad[at] = what
        assert lib.grail_biquad_block_matrix(bad.ctypes.data, 3, out.ctypes.data) == G.ERR_INVALID_ARG and np.all(out == 77.0), at
    bad = coef.copy()
    bad[15] = np.nan                                             # past the filter's three sections: not looked at
    assert lib.grail_biquad_block_matrix(bad.ctypes.data, 3, out.ctypes.data) == G.OK
    assert np.all(out[:36] != 77.0) and np.all(out[36:] == 77.0)


# ---- model against model ----------------------------------------------------------------------------------------------------
def test_the_blocked_model_stays_within_the_bound_of_the_serial_one(both):
    names, serial, blocked = both
    worst = 0.0
    for (fname, sname), (ys, ns, bs), (yb, nb, bb) in zip(names, serial, blocked):
        assert ns == nb == N and bs == bb == 0
        peak = float(np.max(np.abs(ys)))
        apart = float(np.max(np.abs(ys - yb))) / peak
        differ = int(np.count_nonzero(M.to_f32(ys).view(np.uint32) != M.to_f32(yb).view(np.uint32)))
        print(f"\n{fname}, {sname}: |blocked - serial| <= {apart:.3e} of the peak, {differ} of {N} binary32 outputs differ")
        assert apart <= BOUND, (fname, sname, apart)
        worst = max(worst, apart)
    print(f"\nthe largest: {worst:.3e} of the peak")


def test_the_first_block_is_the_serial_models(both):
    names, serial, blocked = both
    for name, (ys, _, _), (yb, _, _) in zip(names, serial, blocked):
        assert np.array_equal(bits(ys[:BM.BLOCK]), bits(yb[:BM.BLOCK])), name


def test_rows_of_at_most_a_block_are_the_serial_models():
    rng = np.random.default_rng(3)
    filters = [rng.uniform(-0.5, 0.5, (S, 5)) for S in (1, 3, 8)]
    rows = [rng.uniform(-1.0, 1.0, n).astype(np.float32) for n in (0, 1, 700, 1023, 1024, 1000, 1024, 5)]
    rows[2][[0, 5]] = (np.float32(-0.0), np.nan)
    which = [0, 1, 2, 0, 1, 2, 7, 2]
    for tail, out_stride in ((0, None), (24, None), (24, 1024), (500, 900), (1500, 1024)):
        want = M.iir_model(rows, filters, which, tail, out_stride)
        got = BM.iir_blocked_model(rows, filters, which, tail, out_stride)
        for r, ((yw, nw, bw), (yg, ng, bg)) in enumerate(zip(want, got)):
            if max(len(rows[r]), 0 if nw == M.REFUSED else nw) > BM.BLOCK:
                continue
            assert (nw, bw) == (ng, bg), (tail, out_stride, r)
            assert (yw is None and yg is None) or np.array_equal(yw.view(np.uint32), yg.view(np.uint32)), (tail, out_stride, r)
    assert got[6] == (None, M.REFUSED, 0) and got[2][2] == 1


# ---- the names ----------------------------------------------------------------------------------------------------------------
def test_header_binding_and_sys_crate_declare_the_call(built):
    hdr = open(os.path.join(ROOT, "include", "grail_hip.h")).read()
    assert "levels, continued: recursive filtering, parallel in time" in hdr and "is not offered" not in hdr
    assert "WHICH CALL FOR WHAT" in hdr and re.search(r"#define GRAIL_BIQUAD_BLOCK 1024\b", hdr)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    sys_rs = open(os.path.join(ROOT, "grail-rs_amd", "rust", "grail-hip-sys", "src", "lib.rs")).read()
    safe_rs = open(os.path.join(ROOT, "grail-rs_amd", "rust", "grail-hip", "src", "lib.rs")).read()
    lib = G.load()
    for name in ("grail_biquad_blocked_async", "grail_biquad_block_matrix"):
        assert re.search(r"\bint %s\s*\(" % name, code), name
        assert name in G.EXPORTS and getattr(lib, name).argtypes is not None, name
        assert re.search(r"pub fn %s\s*\(" % name, sys_rs) and ("sys::" + name) in safe_rs, name
    assert lib.grail_biquad_blocked_async.argtypes == lib.grail_iir_async.argtypes
    for method in ("iir_blocked_async", "iir_blocked"):
        assert callable(getattr(G.Context, method))
    assert lib.grail_abi_version() == G.ABI_VERSION == 4


def test_the_calls_argument_errors_are_the_serial_calls_under_its_own_name(built):
    lib = G.load()
    a, b, ln, fake = 0x10000000, 0x20000000, 0x30000000, 0x40000000           # addresses nobody looks behind
    cases = [
        ((None, None, a, 64, ln, 1, None, 0, b, 128, None, None), b"set is NULL"),
        ((None, fake, a, 64, None, 1, None, 0, b, 128, None, None), b"NULL buffer"),
        ((None, fake, None, 64, ln, 1, None, 0, b, 128, None, None), b"NULL buffer"),
        ((None, fake, a, 64, ln, 1, None, 0, None, 128, None, None), b"NULL buffer"),
        ((None, fake, a, 64, ln, 2, None, 9, a + 4 * 64, 64, None, None), b"overlaps"),
        ((None, fake, a, 2 ** 33, ln, 1, None, 2 ** 32 - 1, 2 ** 50, 2 ** 33, None, None), b"2^32 output samples"),
        ((None, fake, a, 2 ** 59, ln, 4, None, 0, 2 ** 62, 64, None, None), b"2^60 samples"),
        # 2^32 - 1 samples and as long a tail are 2^23 blocks, 2^17 workgroups a row
        ((None, fake, a, 2 ** 32 - 1, ln, 2 ** 14, None, 2 ** 32 - 1, 2 ** 50, 64, None, None), b"more than 2^31 workgroups"),
    ]
    for args, word in cases:
        assert lib.grail_biquad_blocked_async(*args) == G.ERR_INVALID_ARG, args
        assert word in lib.grail_last_error() and b"grail_biquad_blocked_async" in lib.grail_last_error(), (args, lib.grail_last_error())
    if G.device_count() == 0:
        assert lib.grail_biquad_blocked_async(None, fake, a, 64, ln, 2, None, 7, a + 4 * 128, 128, None, None) == G.ERR_NO_DEVICE
        assert lib.grail_biquad_blocked_async(None, fake, a, 2 ** 32 - 1, ln, 2 ** 14 - 1, None, 2 ** 32 - 1, 2 ** 50, 64, None,
                                           None) == G.ERR_NO_DEVICE


def test_dialogue_example_refuses_eq_blocked_without_eq(built):
    exe = os.path.join(ROOT, "grail-rs_amd", "lib", "grail_dialogue")
    r = subprocess.run([exe, "--eq-blocked", "a", "e"], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr and "[--eq KIND:F0:Q[:GAIN]]... [--eq-blocked]" in r.stderr
    if G.device_count() == 0:
        r = subprocess.run([exe, "-o", os.devnull, "--eq", "highpass:100:0.707", "--eq-blocked", "a", "e"], capture_output=True, text=True)
        assert r.returncode == 1 and "no HIP device" in r.stderr
