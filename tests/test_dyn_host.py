"""Dynamics (include/grail_hip.h, "levels, continued: dynamics" and "... of streams") without a GPU: the stream model of
tests/dyn_model.py against its row model, grail_dyn_design and grail_dyn_ballistics against the header's formulas, what the
table promises of the curve between its points, every refusal of the designer, the ballistics, grail_dyn_create, grail_dyn_async
and the stream calls before the device is looked for, and the header, the binding and the -sys crate naming the same things."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import dyn_model as M
import grail_hip as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = sorted(["grail_dyn_design", "grail_dyn_ballistics", "grail_dyn_create", "grail_dyn_free", "grail_dyn_async",
                    "grail_dyn_stream_open", "grail_dyn_stream_next_async", "grail_dyn_stream_close"])


def bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def bits32(a):
    return np.asarray(a, np.float32).view(np.uint32)


def staircase():
    """a caller's own table, G[k] = k: a wrong k or f shows in every bit"""
    return np.arange(M.POINTS, dtype=np.float64)


def curves():
    comp = G.dyn_design(G.DYN_COMPRESS, G.DYN_PEAK, -24.0, 4.0, 6.0, 0.0, 3.0)
    gate = G.dyn_design(G.DYN_EXPAND, G.DYN_SQUARE, -40.0, 3.0, 4.0, 30.0, 0.0)
    return [(comp, G.dyn_ballistics(48000, 1.0, 50.0), G.DYN_PEAK), (gate, G.dyn_ballistics(48000, 0.2, 5.0), G.DYN_SQUARE),
            (staircase(), (0.25, 0.875), G.DYN_PEAK)]


# ---- the stream model is the row model -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("keyed", [False, True])
def test_stream_model_equals_row_model_for_any_chunking(built, keyed):
    rng = np.random.default_rng(11)
    cs = curves()
    n = [200, 129, 64, 500, 0, 200]
    which = [0, 1, 2, 0, 1, 2]
    rows = [(rng.uniform(-1.0, 1.0, k) * 10.0 ** rng.uniform(-4, 1, k)).astype(np.float32) for k in n]
    rows[0][[3, 77]] = (np.nan, -np.inf)
    keys = [(rng.uniform(-1.0, 1.0, 500) * 10.0 ** rng.uniform(-3, 0, 500)).astype(np.float32) for _ in range(5)]
    keys[1][5] = np.inf
    key_row = [0, 1, 2, 3, 4, 0] if keyed else None             # rows 0 and 5, equally long, listen to one key
    # one shot: a key as long as its row's samples, as a stream reads it
    want = M.dyn_model(rows, cs, which, keys=keys if keyed else None, key_row=key_row, key_lens=[200, 129, 64, 500, 0] if keyed else None)
    stream = M.DynStreamModel(cs, which, key_row)
    got = [[] for _ in rows]
    bad, mg, at = [0] * 6, [math.inf] * 6, [0] * 6
    for step in (1, 63, 64, 65, 0, 10 ** 6):
        chunks = [rows[r][at[r]:at[r] + step] for r in range(6)]
        # (a call's key rows start where the rows they drive start)
        call_keys = [keys[j][at[j]:at[j] + step] for j in range(5)] if keyed else None
        for r, (y, k, b, m) in enumerate(stream.next(chunks, call_keys)):
            assert k == len(chunks[r]) and (k or m == 1.0)
            got[r].append(y)
            bad[r] += b
            mg[r] = min(mg[r], m) if k else mg[r]               # (over the calls that fed the row something)
            at[r] += k
    for r in range(6):
        y = np.concatenate(got[r])
        assert np.array_equal(bits32(y), bits32(want[r][0])) and len(y) == n[r] == want[r][1], r
        assert bad[r] == want[r][2] and bits(mg[r] if n[r] else 1.0) == bits(want[r][3]), r
    assert want[0][2] == 2 and want[4][3] == 1.0 and min(w[3] for w in want) < 1.0 < max(w[3] for w in want)


# ---- the designer and the ballistics ---------------------------------------------------------------------------------------------
DESIGNS = [(kind, det, T, R, W, rng_db, mk) for kind in (M.COMPRESS, M.EXPAND) for det in (M.PEAK, M.SQUARE)
           for T, R, W, rng_db, mk in ((-24.0, 4.0, 6.0, 0.0, 0.0), (-18.5, 2.0, 12.0, 20.0, 3.5), (-30.0, 20.0, 0.0, 60.0, -2.0),
                                      (-12.0, 1e9, 0.0, 80.0, 0.0), (-40.0, 1.0, 3.0, 10.0, 6.0))]


@pytest.mark.parametrize("kind,det,T,R,W,range_db,makeup", DESIGNS)
def test_design_matches_its_formulas(built, kind, det, T, R, W, range_db, makeup):
    """the rule of tests/test_iir_host.py: the table is the header's formulas, bit for bit where the C library's log10 and pow
    are Python's, within one unit in the last place of each number otherwise"""
    got, want = G.dyn_design(kind, det, T, R, W, range_db, makeup), M.design_model(kind, det, T, R, W, range_db, makeup)
    assert got.dtype == np.float64 and got.shape == (M.POINTS,) and np.all(np.isfinite(got)) and np.all(got >= 0.0)
    exact = np.array_equal(bits(got), bits(want))
    near = np.abs(got - want) <= np.spacing(np.maximum(np.abs(got), np.abs(want)))
    print("\nbit for bit" if exact else f"\nwithin 1 ulp: {bool(near.all())}")
    assert exact or bool(near.all())
    # the shape: unity (times the make-up) on the side of the threshold that is left alone, an expander held at its range at
    # the bottom, monotone up to the rounding of r: levels run to 200 dB, so r carries a few times 2^-52 * 200 = 4e-14 dB,
    # which is 5e-15 of a gain; 1e-13 of it is the slack
    unity, slack = math.pow(10.0, makeup / 20.0), 1e-13 * got[:-1]
    if kind == M.COMPRESS:
        assert got[0] == unity and np.all(np.diff(got) <= slack)
    else:
        assert got[M.POINTS - 1] == unity and np.all(np.diff(got) >= -slack)
        if R > 1.0:
            assert got[0] == math.pow(10.0, (-range_db + makeup) / 20.0)


def test_levels_are_the_lookups_points():
    """lev[k] is where the lookup lands on k with f = 0, and the float below it on k - 1"""
    k, f, inside = M.index(M.LEVELS)
    assert np.array_equal(k[:-1], np.arange(M.POINTS - 1)) and np.all(f == 0.0) and inside[:-1].all() and not inside[-1]
    k, f, inside = M.index(np.nextafter(M.LEVELS[1:], 0.0))
    assert np.array_equal(k, np.arange(M.POINTS - 1)) and inside.all() and np.all(f == 1.0 - 2.0 ** -48)
    assert M.LEVELS[0] == 2.0 ** -32 and M.LEVELS[-1] == 2.0 ** 8 and M.POINTS == (8 + 32) * 16 + 1


@pytest.mark.parametrize("rate,attack,release", [(48000, 5.0, 120.0), (44100, 0.0, 50.0), (8000, 0.05, 0.0), (96000, 1000.0, 2500.5)])
def test_ballistics_match_their_formula(built, rate, attack, release):
    got, want = G.dyn_ballistics(rate, attack, release), M.ballistics_model(rate, attack, release)
    near = np.abs(got - want) <= np.spacing(np.maximum(got, want))
    assert np.array_equal(bits(got), bits(want)) or bool(near.all()), (got, want)
    assert np.all((got >= 0.0) & (got < 1.0)) and (attack != 0.0 or bits(got[0]) == 0) and (release != 0.0 or bits(got[1]) == 0)


# ---- what the table promises ------------------------------------------------------------------------------------------------------
def reduction_db_np(x, T, R, W):
    """the compressor's r of the header over an array of levels in dB (numpy: the bound is 1e-2 dB, not an ulp)"""
    d, h = x - T, W / 2.0
    knee = ((1.0 / R - 1.0) * (d + h) ** 2) / (2.0 * W) if W > 0.0 else np.zeros_like(x)
    return np.where(d <= -h, 0.0, np.where(d >= h, (T + d / R) - x, knee))


# (-17.7985 dB is the middle, in dB, of the segment 2^-3 .. 2^-3 * 17/16 of the PEAK detector: a corner where the chord is
# farthest from it, in the widest kind of segment)
PROMISES = [(-24.0, 4.0, 6.0), (-24.0, 2.0, 12.0), (-24.0, 20.0, 0.0), (-24.0, 1e9, 0.0), (-17.7985, 20.0, 0.0), (-17.7985, 1e9, 0.0)]


@pytest.mark.parametrize("det", [M.PEAK, M.SQUARE])
@pytest.mark.parametrize("T,R,W", PROMISES)
def test_interpolated_curve_stays_near_the_ideal(built, T, R, W, det):
    """200 000 levels, logarithmically from 2^-31 to 2^7.9, through the lookup on grail_dyn_design's table, against the formula
    evaluated at the level itself.  Bounds: 0.01 dB on segments that hold no corner of the curve (for g = lev^s the chord lies
    within s (s - 1) d^2 / 8 of it, d = 1/16 and |s| <= 1: 0.0085 dB); 0.14 dB on the one segment that holds a hard corner
    ((1 - 1/R) w / 4 with w = 20 log10(17/16) = 0.527 dB, the widest a segment is)."""
    gain = G.dyn_design(G.DYN_COMPRESS, det, T, R, W, 0.0, 0.0)
    e = 2.0 ** np.linspace(-31.0, 7.9, 200000)
    per_db = 20.0 if det == M.PEAK else 10.0
    got = 20.0 * np.log10(M.lookup_one(gain, e))
    want = reduction_db_np(per_db * np.log10(e), T, R, W)
    err = np.abs(got - want)
    k = M.index(e)[0]
    corner = np.zeros(len(e), bool)
    if W == 0.0:                                                # the segment lev[kc] <= the threshold's level < lev[kc + 1]
        kc = int(np.searchsorted(M.LEVELS, 10.0 ** (T / per_db), side="right")) - 1
        corner = k == kc
        assert corner.any()
    smooth, hard = float(err[~corner].max()), float(err[corner].max()) if corner.any() else 0.0
    print(f"\n{R:g}:1 knee {W:g} dB detector {det}: {smooth:.4f} dB off the corner, {hard:.4f} dB on it")
    assert smooth <= 0.01 and hard <= 0.14


# ---- the arguments --------------------------------------------------------------------------------------------------------------
def test_design_and_ballistics_refusals(built):
    lib = G.load()
    buf = np.full(M.POINTS + 3, 77.0, np.float64)
    nan, inf = float("nan"), float("inf")
    ok = (0, 0, -24.0, 4.0, 6.0, 0.0, 0.0)
    for at, bad in [(0, -1), (0, 2), (1, -1), (1, 2), (2, nan), (2, inf), (3, 0.5), (3, nan), (3, inf), (3, -4.0), (4, -1.0), (4, nan),
                    (4, inf), (5, -1.0), (5, nan), (5, inf), (6, nan), (6, -inf), (6, 1e5)]:
        args = list(ok)
        args[at] = bad
        assert lib.grail_dyn_design(*args, buf.ctypes.data) == G.ERR_INVALID_ARG, args
        assert np.all(buf == 77.0)
    assert lib.grail_dyn_design(*ok, None) == G.ERR_INVALID_ARG
    assert lib.grail_dyn_design(*ok, buf.ctypes.data) == G.OK and np.all(buf[M.POINTS:] == 77.0) and np.all(buf[:M.POINTS] != 77.0)
    al = np.full(4, 77.0, np.float64)
    for args in [(0, 1.0, 1.0), (48000, -1.0, 1.0), (48000, 1.0, -1.0), (48000, nan, 1.0), (48000, 1.0, inf), (48000, 1e300, 1.0)]:
        assert lib.grail_dyn_ballistics(*args, al.ctypes.data) == G.ERR_INVALID_ARG, args
        assert np.all(al == 77.0)
    assert lib.grail_dyn_ballistics(48000, 1.0, 1.0, None) == G.ERR_INVALID_ARG
    assert lib.grail_dyn_ballistics(48000, 1.0, 0.0, al.ctypes.data) == G.OK and np.all(al[2:] == 77.0) and al[1] == 0.0 < al[0] < 1.0


def test_argument_errors_come_before_the_device(built):
    lib = G.load()
    out = C.c_void_p(0x77)
    po = C.addressof(out)
    gain = np.tile(np.linspace(1.0, 0.0, M.POINTS), 17)
    alpha = np.tile([0.5, 0.9], 17)
    det = np.tile(np.array([0, 1], np.uint32), 9)

    def create(g, a, d, n, where=po):
        return lib.grail_dyn_create(None, None if g is None else g.ctypes.data, None if a is None else a.ctypes.data,
                                    None if d is None else d.ctypes.data, n, where)

    for case, word in [((gain, alpha, det, 1, None), b"NULL"), ((None, alpha, det, 1), b"NULL"), ((gain, None, det, 1), b"NULL"),
                       ((gain, alpha, None, 1), b"NULL"), ((gain, alpha, det, 0), b"outside 1 .. 16"),
                       ((gain, alpha, det, 17), b"outside 1 .. 16")]:
        assert create(*case) == G.ERR_INVALID_ARG and out.value == 0x77, word
        assert b"grail_dyn_create" in lib.grail_last_error() and word in lib.grail_last_error(), lib.grail_last_error()
    for at, what, word in ((0, np.nan, b"not finite"), (M.POINTS - 1, np.inf, b"not finite"), (M.POINTS, -1e-300, b"negative"),
                           (2 * M.POINTS - 1, -np.inf, b"not finite")):
        bad = gain.copy()
        bad[at] = what
        assert create(bad, alpha, det, 2) == G.ERR_INVALID_ARG and word in lib.grail_last_error(), (at, lib.grail_last_error())
    for at, what in ((0, 1.0), (1, -0.25), (2, np.nan), (3, 1.5)):
        bad = alpha.copy()
        bad[at] = what
        assert create(gain, bad, det, 2) == G.ERR_INVALID_ARG and b"alpha" in lib.grail_last_error()
    bad = det.copy()
    bad[1] = 2
    assert create(gain, alpha, bad, 2) == G.ERR_INVALID_ARG and b"detector" in lib.grail_last_error()
    bad = gain.copy()
    bad[2 * M.POINTS] = np.nan                                                  # past the set's curves: not looked at
    a, b, k, ln, fake = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000      # addresses nobody looks behind
    # (ctx, set, rows, row_stride, len, n_rows, curve, key, key_stride, key_len, n_keys, key_row, out, out_stride, 3 results)
    cases = [
        ((None, None, a, 64, ln, 1, None, None, 0, None, 0, None, b, 64, None, None, None), b"set is NULL"),
        ((None, None, a, 64, ln, 0, None, None, 0, None, 0, None, b, 64, None, None, None), b"set is NULL"),
        ((None, fake, a, 64, None, 1, None, None, 0, None, 0, None, b, 64, None, None, None), b"NULL buffer"),
        ((None, fake, None, 64, ln, 1, None, None, 0, None, 0, None, b, 64, None, None, None), b"NULL buffer"),
        ((None, fake, a, 64, ln, 1, None, None, 0, None, 0, None, None, 64, None, None, None), b"NULL buffer"),
        ((None, fake, a, 64, ln, 2, None, None, 0, None, 0, None, a + 4 * 64, 64, None, None, None), b"overlaps rows_dev"),
        ((None, fake, a, 64, ln, 1, None, None, 0, None, 0, None, a, 64, None, None, None), b"overlaps rows_dev"),
        ((None, fake, a, 2 ** 32, ln, 1, None, None, 0, None, 0, None, 2 ** 50, 2 ** 32, None, None, None), b"2^32 output samples"),
        ((None, fake, a, 2 ** 59, ln, 4, None, None, 0, None, 0, None, 2 ** 62, 64, None, None, None), b"2^60 samples"),
        ((None, fake, a, 64, ln, 2, None, k, 64, None, 0, None, b, 64, None, None, None), b"n_keys = 0"),
        ((None, fake, a, 64, ln, 2, None, k, 64, None, 1, None, b, 64, None, None, None), b"n_keys < n_rows"),
        ((None, fake, a, 64, ln, 2, None, k, 2 ** 59, None, 4, None, b, 64, None, None, None), b"2^60 samples"),
        ((None, fake, a, 64, ln, 2, None, b + 4 * 127, 64, None, 2, None, b, 64, None, None, None), b"overlaps key_dev"),
        ((None, fake, a, 64, ln, 2, None, b - 4 * 64 + 4, 64, None, 1, ln, b, 64, None, None, None), b"overlaps key_dev"),
    ]
    for args, word in cases:
        assert lib.grail_dyn_async(*args) == G.ERR_INVALID_ARG, args
        assert word in lib.grail_last_error() and b"grail_dyn_async" in lib.grail_last_error(), (args, lib.grail_last_error())
    assert lib.grail_dyn_free(None, fake) == G.ERR_INVALID_ARG and lib.grail_dyn_free(None, None) == G.OK
    # streams: no context, no stream; a stream nobody looks into
    assert lib.grail_dyn_stream_open(None, fake, 1, None, 0, None, po) == G.ERR_INVALID_ARG and out.value == 0x77
    assert lib.grail_dyn_stream_close(None, fake) == G.ERR_INVALID_ARG and lib.grail_dyn_stream_close(None, None) == G.OK
    # (ctx, stream, in, in_stride, in_len, key, key_stride, out, out_stride, 3 results)
    stream_cases = [
        ((None, None, a, 64, ln, None, 0, b, 64, None, None, None), b"the stream is NULL"),
        ((None, fake, a, 64, ln, None, 0, b, 63, None, None, None), b"out_stride < in_stride"),
        ((None, fake, a, 64, ln, k, 63, b, 64, None, None, None), b"key_stride < in_stride"),
        ((None, fake, a, 64, None, None, 0, b, 64, None, None, None), b"NULL buffer"),
        ((None, fake, None, 64, ln, None, 0, b, 64, None, None, None), b"NULL buffer"),
        ((None, fake, a, 64, ln, None, 0, None, 64, None, None, None), b"NULL buffer"),
        ((None, fake, a, 64, ln, None, 0, a + 4 * 63, 64, None, None, None), b"overlaps in_dev"),
        ((None, fake, a, 64, ln, b + 4 * 63, 64, b, 64, None, None, None), b"overlaps key_dev"),
    ]
    for args, word in stream_cases:
        assert lib.grail_dyn_stream_next_async(*args) == G.ERR_INVALID_ARG, args
        assert word in lib.grail_last_error() and b"grail_dyn_stream_next_async" in lib.grail_last_error(), (args, lib.grail_last_error())
    if G.device_count() == 0:        # no context can exist: the valid calls say why, they do not compute on the CPU
        assert create(bad, alpha, det, 2) == G.ERR_NO_DEVICE and out.value == 0x77
        assert b"no usable HIP device" in lib.grail_last_error()
        assert lib.grail_dyn_async(None, fake, a, 64, ln, 2, None, k, 64, None, 1, ln, b, 64, None, None, None) == G.ERR_NO_DEVICE
        assert lib.grail_dyn_async(None, fake, None, 0, None, 0, None, None, 0, None, 0, None, None, 0, None, None, None) == G.ERR_NO_DEVICE
        assert lib.grail_dyn_stream_next_async(None, fake, a, 64, ln, k, 64, b, 64, None, None, None) == G.ERR_NO_DEVICE


def test_stream_checks_of_the_plan(built):
    """What grail_dyn_stream_open and a keyed or self-keyed stream's `next` refuse needs a live set and stream to be reached
    through the C ABI (tests/test_dyn_stream_gpu.py does); the checks themselves are dyn_plan.cpp's and run under the sanitizers
    in tests/test_dyn_sanitize.py.  Here: the binding refuses to open a stream on a set that is no set."""
    lib = G.load()
    out = C.c_void_p(0x77)
    assert lib.grail_dyn_stream_open(None, None, 1, None, 0, None, C.addressof(out)) == G.ERR_INVALID_ARG
    assert b"grail_dyn_stream_open" in lib.grail_last_error() and out.value == 0x77


def test_header_python_and_rust_name_the_same_functions_and_constants(built):
    hdr = open(os.path.join(ROOT, "include", "grail_hip.h")).read()
    assert "levels, continued: dynamics" in hdr and "levels, continued: dynamics of streams" in hdr
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(set(re.findall(r"\b(grail_dyn_[a-z0-9_]+)\s*\(", code))) == FUNCTIONS
    assert sorted(n for n in G.EXPORTS if n.startswith("grail_dyn")) == FUNCTIONS
    sys_rs = open(os.path.join(ROOT, "grail-rs_amd", "rust", "grail-hip-sys", "src", "lib.rs")).read()
    assert sorted(set(re.findall(r"pub fn (grail_dyn_[a-z0-9_]+)\s*\(", sys_rs))) == FUNCTIONS
    constants = dict(re.findall(r"#define (GRAIL_DYN_[A-Z0-9_]+)\s+\(?(-?\d+)\)?", hdr))
    assert constants == {"GRAIL_DYN_STEPS_PER_OCTAVE": "16", "GRAIL_DYN_LOG2_LO": "-32", "GRAIL_DYN_LOG2_HI": "8",
                         "GRAIL_DYN_POINTS": "641", "GRAIL_DYN_CURVES_MAX": "16", "GRAIL_DYN_PEAK": "0", "GRAIL_DYN_SQUARE": "1",
                         "GRAIL_DYN_COMPRESS": "0", "GRAIL_DYN_EXPAND": "1"}
    assert dict(re.findall(r"pub const (GRAIL_DYN_[A-Z0-9_]+): (?:u32|i32|c_int) = (-?\d+);", sys_rs)) == constants
    mine = {"GRAIL_DYN_STEPS_PER_OCTAVE": G.DYN_STEPS_PER_OCTAVE, "GRAIL_DYN_LOG2_LO": G.DYN_LOG2_LO, "GRAIL_DYN_LOG2_HI": G.DYN_LOG2_HI,
            "GRAIL_DYN_POINTS": G.DYN_POINTS, "GRAIL_DYN_CURVES_MAX": G.DYN_CURVES_MAX, "GRAIL_DYN_PEAK": G.DYN_PEAK,
            "GRAIL_DYN_SQUARE": G.DYN_SQUARE, "GRAIL_DYN_COMPRESS": G.DYN_COMPRESS, "GRAIL_DYN_EXPAND": G.DYN_EXPAND}
    assert {k: str(v) for k, v in mine.items()} == constants
    assert (M.STEPS, M.LOG2_LO, M.LOG2_HI, M.POINTS, M.CURVES_MAX) == (G.DYN_STEPS_PER_OCTAVE, G.DYN_LOG2_LO, G.DYN_LOG2_HI,
                                                                      G.DYN_POINTS, G.DYN_CURVES_MAX)
    assert (M.PEAK, M.SQUARE, M.COMPRESS, M.EXPAND, M.REFUSED) == (G.DYN_PEAK, G.DYN_SQUARE, G.DYN_COMPRESS, G.DYN_EXPAND, G.LIMIT_REFUSED)
    safe_rs = open(os.path.join(ROOT, "grail-rs_amd", "rust", "grail-hip", "src", "lib.rs")).read()
    lib = G.load()
    for name in FUNCTIONS:
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None, name
        assert ("sys::" + name) in safe_rs, name
    for method in ("dyn_create", "dyn_free", "dyn_async", "dyn", "dyn_stream_open", "dyn_stream_next_async", "dyn_stream_next",
                   "dyn_stream_close"):
        assert callable(getattr(G.Context, method)), method


def test_dialogue_example_knows_the_compress_option(built):
    import subprocess
    exe = os.path.join(ROOT, "grail-rs_amd", "lib", "grail_dialogue")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "[--compress T:R[:KNEE[:ATTACK_MS:RELEASE_MS]] [--makeup DB]]" in r.stderr
    for bad in (["--compress"], ["--compress", "-24"], ["--compress", "-24:3:6:5"], ["--compress", "-24:0.5"], ["--compress", "-24:3:-1"],
                ["--compress", "x:3"], ["--compress", "-24:3:"], ["--compress", "-24:3:6:5:120:7"], ["--compress", "-24:nan"],
                ["--compress", "-24:3:6:-5:120"], ["--makeup", "3"], ["--compress", "-24:3", "--makeup"], ["--compress", "-24:3", "--makeup", "x"],
                ["--compress", "-24:3", "--compress", "-20:2"], ["--compress", "-24:3", "--makeup", "1e5"]):
        r = subprocess.run([exe] + bad + ["a", "e"], capture_output=True, text=True)
        assert r.returncode == 2 and "usage" in r.stderr, bad
    if G.device_count() == 0:
        r = subprocess.run([exe, "-o", os.devnull, "--lufs", "-23", "--compress", "-24:3:6:5:120", "--makeup", "2", "--ceiling", "-1", "--limit",
                            "a", "e"], capture_output=True, text=True)
        assert r.returncode == 1 and "no HIP device" in r.stderr
