"""The look-ahead limiter (include/grail_hip.h, "levels, continued: limiter") without a GPU: the numpy model of the contract
that tests/test_limiter_gpu.py holds the device to, the contract's own claims checked on the model (|z| <= c exactly, rows
under the ceiling untouched, the dip of a lone sample, the derived true-peak bound), grail_limit_ceiling, every argument
refusal of grail_limit_async ahead of the missing device, the signatures and the example's usage."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import grail_hip as G
from test_true_peak_host import FLT_MAX, NUMERATORS, TAP_SUM, TAPS, db, same_bits, tone, true_peak_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = 1 << 24
REFUSED = 0xFFFFFFFF


def detector(x):
    """step 1 for one row: d[t] = max(|v[t]|, e[t] .. e[t + 11]) with e[u] = max_p |y[p][u]|, the y of true_peak_model (the
    same left fold, element by element) -> (d float64 [n], count of non-finite samples)"""
    x = np.asarray(x, np.float32)
    n = len(x)
    with np.errstate(invalid="ignore"):
        finite = np.abs(x) <= FLT_MAX
    v = np.where(finite, x, np.float32(0.0)).astype(np.float64)
    padded = np.concatenate([np.zeros(11), v, np.zeros(11)])
    e = np.zeros(n + 11)
    for p in range(4):
        acc = np.zeros(n + 11)
        for k in range(12):
            acc = acc + TAPS[p, k] * padded[11 - k:11 - k + n + 11]
        e = np.maximum(e, np.abs(acc))
    d = np.abs(v)
    for j in range(12):
        d = np.maximum(d, e[j:j + n])
    return d, int(n - np.count_nonzero(finite))


def limiter_model(rows, c, ell, group=1, curves=False):
    """the header's five steps in numpy.  rows: float32 arrays, n_rows a multiple of group.
    -> (out: one float32 array per row, None for the rows of a refused group; min_gain float32, n_limited uint32,
    nonfinite uint32, one per group); with curves=True also the groups' (q, S, g)"""
    c = np.float32(c)
    cd, L = float(c), 1 << ell
    assert len(rows) % group == 0 and cd > 0 and 0 <= ell <= 10
    out, min_gain, n_limited, nonfinite, kept = [], [], [], [], []
    for first in range(0, len(rows), group):
        members = [np.asarray(x, np.float32) for x in rows[first:first + group]]
        n = len(members[0])
        if any(len(x) != n for x in members):
            out += [None] * group
            min_gain.append(np.float32(np.nan)), n_limited.append(REFUSED), nonfinite.append(0), kept.append(None)
            continue
        found = [detector(x) for x in members]
        d = np.max([f[0] for f in found], axis=0) if n else np.zeros(0)
        with np.errstate(divide="ignore"):
            ratio = np.floor(cd * Q / d)                                    # one rounded division; cd * Q is exact
        q = np.where(d <= cd, Q, np.minimum(Q, ratio)).astype(np.int64)
        m = np.concatenate([np.full(L - 1, Q), q, np.full(L - 1, Q)])       # q[s], s = -(L - 1) .. n + L - 2
        w = 1
        while w < L:                                                        # the minimum over L = 2^ell by doubling
            m = np.minimum(m[:-w], m[w:])
            w *= 2
        total = np.concatenate([[0], np.cumsum(m)])                         # m[s], s = -(L - 1) .. n - 1: integers
        S = total[L:] - total[:-L]
        assert len(S) == n
        g = (S.astype(np.float64) * 2.0 ** -(24 + ell)).astype(np.float32)
        for x in members:
            with np.errstate(invalid="ignore", over="ignore"):
                z = g * x
                z = np.where(z < -c, -c, np.where(z > c, c, z))
                z = np.where(np.abs(x) <= FLT_MAX, z, np.float32(0.0)).astype(np.float32)
            out.append(z)
        min_gain.append(g.min() if n else np.float32(1.0))
        n_limited.append(int(np.count_nonzero(S < L * Q)))
        nonfinite.append(sum(f[1] for f in found))
        kept.append((q, S, g))
    res = (out, np.array(min_gain, np.float32), np.array(n_limited, np.uint32), np.array(nonfinite, np.uint32))
    return res + (kept,) if curves else res


def bound_of(c, ell, x):
    """the header's BOUND on the true peak of the limited row"""
    c = float(np.float32(c))
    return c + 11.0 / (1 << ell) * TAP_SUM * float(np.abs(x).max()) + TAP_SUM * 2.0 ** -24 * c


def named_signals():
    """noise, the quarter-rate tone sampled 45 degrees off its crests, loud and quiet bursts, a lone impulse"""
    rng = np.random.default_rng(17)
    noise = (rng.standard_normal(6000) * 0.4).astype(np.float32)
    bursts = (rng.standard_normal(6000) * 0.02).astype(np.float32)
    for at in (300, 1700, 1712, 4000):
        bursts[at:at + 150] *= np.float32(60.0)
    impulse = np.zeros(3000, np.float32)
    impulse[1500] = 2.0
    return {"noise": noise, "tone": tone(12000.0, 45.0, 0.9, seconds=0.125, fade=500), "bursts": bursts, "impulse": impulse}


# ---- the contract's claims, on the model ------------------------------------------------------------------------------------
@pytest.mark.parametrize("ell", [0, 1, 4, 6, 8, 10])
def test_the_result_is_within_the_ceiling_exactly_and_the_bound_holds(ell):
    c = np.float32(0.5)
    for name, x in named_signals().items():
        (z,), min_gain, n_limited, bad, ((q, S, g),) = limiter_model([x], c, ell, curves=True)
        assert np.all(np.abs(z) <= c), name                                # exactly
        assert 0 < n_limited[0] <= len(x) and bad[0] == 0 and min_gain[0] == g.min() < 1
        assert np.all(g.astype(np.float64) <= q / Q), name                 # g[t] <= q[t] / Q: what the guarantee rests on
        assert np.all(np.abs(np.diff(S)) <= Q)                             # g moves by at most 1 / L per sample
        tp = true_peak_model(z)[0]
        print(f"\n{name}, L = {1 << ell}: true peak {db(tp / float(c)):+.5f} dB against c, bound {db(bound_of(c, ell, x) / float(c)):+.3f} dB, "
              f"min gain {min_gain[0]:.4f}, {n_limited[0]} samples limited")
        assert tp <= bound_of(c, ell, x), (name, tp)


def test_the_clamp_catches_the_last_ulp_only():
    """|g x| exceeds c by rounding alone, if at all: at most one float above c before the clamp"""
    c = np.float32(0.5)
    for ell in (0, 5):
        for name, x in named_signals().items():
            _, _, _, _, ((q, S, g),) = limiter_model([x], c, ell, curves=True)
            assert np.abs(g * x).max() <= np.nextafter(c, np.float32(1.0)), (name, ell)


def test_rows_under_the_ceiling_come_back_bit_for_bit():
    rng = np.random.default_rng(18)
    x = (rng.standard_normal(5000) * 0.05).astype(np.float32)
    x[[0, 17, 4999]] = [-0.0, 1e-45, -3e-39]
    d, _ = detector(x)
    c = np.float32(d.max())                                                 # the smallest ceiling that no d is above
    c = c if float(c) >= d.max() else np.nextafter(c, np.float32(np.inf))
    for ell in (0, 3, 10):
        (z,), min_gain, n_limited, _, ((q, S, g),) = limiter_model([x], c, ell, curves=True)
        assert same_bits(z, x) and np.all(g == np.float32(1.0)) and min_gain[0] == 1 and n_limited[0] == 0
    # a non-finite sample writes +0.0 and is counted; the rest still passes untouched
    y = x.copy()
    y[[5, 600]] = [np.nan, -np.inf]
    (z,), _, n_limited, bad = limiter_model([y], np.float32(10.0), 4)
    want = y.copy()
    want[[5, 600]] = 0.0
    assert same_bits(z, want) and bad[0] == 2 and n_limited[0] == 0
    # empty rows
    out, min_gain, n_limited, bad = limiter_model([np.zeros(0, np.float32)] * 2, c, 6, group=2)
    assert [len(z) for z in out] == [0, 0] and min_gain[0] == 1 and n_limited[0] == 0 and bad[0] == 0


@pytest.mark.parametrize("ell", [0, 1, 6, 10])
def test_a_lone_sample_of_four_times_the_ceiling(ell):
    """min_gain = 0.25 within the quantum (it is exact: c Q / 4c = Q / 4), at the sample itself.  The dip is one run of
    2 L - 2 + h samples, h the number of hot d[t].  A sample feeds the 23 values d[p - 11 .. p + 11], so the dip always lies
    within 2 L - 1 + 11 + 11 samples around it, and spans exactly those when every one of the twelve outputs carries the
    sample above the ceiling (the weakest carries 239 / 8192 of it: a sample of 64 c does).  At 4 c only the taps above 1 / 4
    do (7964, 6388 and 3810 of 8192: outputs p + 5 and p + 6), so d is hot for t = p - 6 .. p + 6: h = 13, counted here
    from the table."""
    c, L = np.float32(0.125), 1 << ell
    n, p = 4 * 1024 + 200, 2100
    strongest = np.abs(NUMERATORS).max(axis=0)                              # of the four phases, per tap
    for amplitude, h in ((4.0, 13), (64.0, 23)):
        x = np.zeros(n, np.float32)
        x[p] = np.float32(amplitude) * c
        hot_outputs = np.flatnonzero(strongest * amplitude > 8192)
        assert np.array_equal(hot_outputs, np.arange(hot_outputs[0], hot_outputs[-1] + 1))
        assert h == hot_outputs[-1] - hot_outputs[0] + 12                   # the t with an output of t .. t + 11 among them
        (z,), min_gain, n_limited, _, ((q, S, g),) = limiter_model([x], c, ell, curves=True)
        dipped = np.flatnonzero(g < 1)
        assert len(dipped) == n_limited[0] == 2 * L - 2 + h, (amplitude, len(dipped))
        assert np.array_equal(dipped, np.arange(dipped[0], dipped[0] + len(dipped)))        # one run
        assert p - 11 - (L - 1) <= dipped[0] and dipped[-1] <= p + 11 + (L - 1)
        if amplitude == 4.0:
            assert abs(float(min_gain[0]) - 0.25) <= 2.0 ** -24 and g[p] == min_gain[0] == 0.25
            assert z[p] == c and np.count_nonzero(z) == 1
        else:
            assert len(dipped) == 2 * L - 1 + 11 + 11 and dipped[0] == p - 11 - (L - 1)
            assert np.abs(z).max() <= c


def test_a_linked_pair_shares_one_curve_and_unequal_members_are_refused():
    rng = np.random.default_rng(19)
    left = (rng.standard_normal(3000) * 0.01).astype(np.float32)
    right = (rng.standard_normal(3000) * 0.01).astype(np.float32)
    left[1234] = 0.9
    c = np.float32(0.25)
    out, min_gain, n_limited, bad, ((q, S, g),) = limiter_model([left, right], c, 5, group=2, curves=True)
    alone = limiter_model([left], c, 5)
    assert same_bits(out[0], alone[0][0]) and min_gain[0] == alone[1][0] and n_limited[0] == alone[2][0]
    with np.errstate(invalid="ignore"):
        assert same_bits(out[1], g * right) and np.count_nonzero(out[1] != right) > 2 * 32
    out, min_gain, n_limited, bad = limiter_model([left, right[:-1], right, right], c, 5, group=2)
    assert out[0] is None and out[1] is None and np.isnan(min_gain[0]) and n_limited[0] == REFUSED and bad[0] == 0
    assert same_bits(out[2], right) and min_gain[1] == 1


# ---- grail_limit_ceiling ----------------------------------------------------------------------------------------------------
def test_limit_ceiling(built):
    for ceiling_db in (-1.0, 0.0, -0.1, -23.5, 6.0, -120.0, 1e-3, -6.0205999):
        want = np.float32(math.pow(10.0, float(np.float32(ceiling_db)) / 20.0))
        got = G.limit_ceiling(ceiling_db)
        assert got.dtype == np.float32 and same_bits(np.array([got]), np.array([want])), ceiling_db
    assert G.limit_ceiling(0.0) == 1 and G.limit_ceiling(-1.0) == np.float32(0.8912509381337456)
    assert math.isnan(G.limit_ceiling(float("nan"))) and G.limit_ceiling(-math.inf) == 0 and G.limit_ceiling(math.inf) == math.inf


# ---- signatures, refusals, and the device entry point without a device ------------------------------------------------------
def test_signatures_and_header(built):
    lib = G.load()
    for name in ("grail_limit_async", "grail_limit_ceiling"):
        assert name in G.EXPORTS and getattr(lib, name).argtypes is not None
    assert len(lib.grail_limit_async.argtypes) == 13 and lib.grail_limit_ceiling.restype is C.c_float
    assert lib.grail_abi_version() == 4                                     # additive: the version stays
    hdr = open(os.path.join(ROOT, "include", "grail_hip.h")).read()
    assert "levels, continued: limiter" in hdr
    assert "#define GRAIL_LIMIT_LOOKAHEAD_LOG2_MAX 10" in hdr and "#define GRAIL_LIMIT_REFUSED 0xFFFFFFFFu" in hdr
    assert f"#define GRAIL_LIMIT_CHUNK {G.LIMIT_CHUNK}" in hdr
    assert (G.LIMIT_LOOKAHEAD_LOG2_MAX, G.LIMIT_REFUSED) == (10, REFUSED)
    kernels_h = open(os.path.join(ROOT, "grail-rs_amd", "csrc", "kernels.h")).read()
    assert f"constexpr uint32_t LIMIT_CHUNK = {G.LIMIT_CHUNK};" in kernels_h


def test_every_argument_refusal_comes_before_the_missing_device(built):
    """no pointer is followed before the device is asked for, so made-up addresses serve; ctx is NULL throughout: with a
    device that is the well-formed call's INVALID_ARG, without one its NO_DEVICE"""
    lib = G.load()
    rows, out, lens = 0x10000000, 0x20000000, 0x30000000
    stride, n_rows = 1024, 4

    def call(rows=rows, row_stride=stride, lens=lens, n_rows=n_rows, group=1, ceiling=0.5, ell=8, out=out, out_stride=stride):
        return lib.grail_limit_async(None, rows, row_stride, lens, n_rows, group, ceiling, ell, out, out_stride, None, None, None)

    refused = dict(
        ell_11=call(ell=11), ell_huge=call(ell=0xFFFFFFFF), group_0=call(group=0), group_3_of_4=call(group=3),
        group_above=call(group=8), ceiling_0=call(ceiling=0.0), ceiling_negative=call(ceiling=-0.5),
        ceiling_nan=call(ceiling=float("nan")), ceiling_inf=call(ceiling=float("inf")), ceiling_minus_inf=call(ceiling=float("-inf")),
        rows_null=call(rows=None), out_null=call(out=None), len_null=call(lens=None), out_stride_short=call(out_stride=stride - 1),
        in_place=call(out=rows), out_starts_inside=call(out=rows + (n_rows * stride - 1) * 4),
        out_ends_inside=call(out=rows - (n_rows * stride - 1) * 4),
        out_wider_around=call(out=rows - 4 * 2 * stride, out_stride=2 * stride))
    assert all(rc == G.ERR_INVALID_ARG for rc in refused.values()), refused
    call(ell=11)
    assert b"lookahead_log2" in lib.grail_last_error()
    call(out=rows)
    assert b"overlaps" in lib.grail_last_error()
    no_device = G.device_count() == 0
    well_formed = [call(), call(ell=0), call(ell=10, group=2), call(group=4), call(out=rows + n_rows * stride * 4),
                   call(out=rows - n_rows * stride * 4), call(n_rows=0, rows=None, out=None, lens=None),
                   call(row_stride=0, rows=None, out=None, out_stride=0), call(ceiling=1e-45), call(ceiling=3.4028234663852886e38)]
    assert all(rc == (G.ERR_NO_DEVICE if no_device else G.ERR_INVALID_ARG) for rc in well_formed), well_formed
    if no_device:
        call()
        assert b"no usable HIP device" in lib.grail_last_error()
        with pytest.raises(G.GrailError):
            G.Context(0)


def test_dialogue_example_knows_the_limit_option(built):
    exe = os.path.join(ROOT, "grail-rs_amd", "lib", "grail_dialogue")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "--limit" in r.stderr and "--ceiling DBTP" in r.stderr
    r = subprocess.run([exe, "--lufs", "-23", "--limit", "a", "e"], capture_output=True, text=True)       # no ceiling to hold
    assert r.returncode == 2 and "usage" in r.stderr
    if G.device_count() == 0:
        r = subprocess.run([exe, "-o", os.devnull, "--lufs", "-23", "--ceiling", "-1", "--limit", "a", "e"], capture_output=True,
                           text=True)
        assert r.returncode == 1 and "no HIP device" in r.stderr
