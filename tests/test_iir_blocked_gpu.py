"""Recursive filtering parallel in time on the device (grail_biquad_blocked_async) against the numpy model of
tests/iir_blocked_model.py, bit for bit in the filtered samples (NaN positions compared as NaN), the lengths and the
non-finite counts: rows that end at, before and after a block's edge and the edge of a workgroup's 64 blocks, filters of one,
three and eight sections in one launch, tails that stay inside a block and that cross one, the scalar path against the
aligned one, out_stride cutting inside a row, counts without outputs, non-finite samples in several blocks and past a cut,
refused rows, scratch left by a longer call, a row of over a thousand blocks, the section bounds below eight on both paths,
and a workgroup that starts past its row's stride.  Against grail_iir_async on the device:
the same bits over rows of one block and over every row's first block, and within the contract's bound elsewhere.  Every
output buffer holds a canary wherever nothing may be written, and is checked there."""
import ctypes as C
import os
import re
import subprocess
import wave

import numpy as np
import pytest

import grail_hip as G
from iir_blocked_model import BLOCK, iir_blocked_model
from iir_model import REFUSED
from test_iir_blocked_host import BOUND, butterworth
from test_iir_gpu import BOUNDS, bound_of, noise, random_filter, same_samples
from test_levels_gpu import CANARY, Dev, dev  # noqa: F401  (dev is a fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# either side of a block's edge, of two blocks', and of a workgroup's 64 blocks
LENGTHS = [0, 1, 1023, 1024, 1025, 2048, 2049, 65536, 65537, 70000]


def launch(ctx, dev, iir_set, rows, which=None, tail=0, stride=None, out_stride=None, in_offset=0, out_offset=0, guard=64,
           call="iir_blocked"):
    """rows[i] as row i of a buffer that holds NaN everywhere else, filtered by `call` with filter which[i] of the set (None:
    filter_dev NULL) into a buffer that holds CANARY between the rows' outputs, with `guard` floats of it before and after
    -> (out [n_rows, out_stride] as it lies on the device afterwards, out_len, nonfinite)"""
    longest = max([len(x) for x in rows] + [1])
    stride = stride or (longest + 63) // 64 * 64
    out_stride = (longest + tail + 63) // 64 * 64 if out_stride is None else out_stride
    host = np.full(len(rows) * stride + in_offset, np.nan, np.float32)
    for i, x in enumerate(rows):
        host[in_offset + i * stride:in_offset + i * stride + len(x)] = x
    d_in = dev.up(host)
    before = guard + out_offset
    d_out = dev.up(np.full(before + len(rows) * out_stride + guard, CANARY, np.float32))
    d_len = dev.up(np.array([len(x) for x in rows], np.uint32))
    d_which = None if which is None else dev.up(np.array(which, np.uint32))
    out_len, bad = getattr(ctx, call)(iir_set, C.c_void_p(d_in.value + in_offset * 4), stride, d_len, len(rows), d_which, tail,
                                      C.c_void_p(d_out.value + before * 4) if out_stride else None, out_stride)
    out = dev.down(d_out, before + len(rows) * out_stride + guard, np.float32)
    assert np.all(out[:before] == CANARY) and np.all(out[before + len(rows) * out_stride:] == CANARY), "written outside out"
    return out[before:before + len(rows) * out_stride].reshape(len(rows), out_stride), out_len, bad


def same(want, got, what):
    """the device's (out, out_len, nonfinite) against the model's rows; out rows hold the canary past their outputs; a row
    whose index is outside the set holds nothing else"""
    out, out_len, bad = got
    for i, (y, n_out, w_bad) in enumerate(want):
        assert (out_len[i], bad[i]) == (n_out, w_bad), (what, i, out_len[i], n_out, bad[i], w_bad)
        if n_out == REFUSED:
            assert np.all(out[i] == CANARY), (what, i, "a refused row")
            continue
        assert np.all(out[i, n_out:] == CANARY), (what, i, "written past the row's outputs")
        same_samples(out[i, :n_out], y, (what, i))


@pytest.fixture
def sets(gpu_ctx):
    made = []

    def create(filters):
        made.append(gpu_ctx.iir_create(filters))
        return made[-1]
    yield create
    for s in made:
        gpu_ctx.iir_free(s)


# biquad_block_kernel<section bound, VEC, OUT> and biquad_block_propagate_kernel<section bound>: the twenty that
# tests/test_iir_blocked_code_objects.py finds in the library
VARIANTS = ([("block", sb, vec, out) for sb in BOUNDS for vec in (True, False) for out in (False, True)] +
            [("propagate", sb) for sb in BOUNDS])
# the lower bounds' rows: either side of a block's edge and of two blocks', and one sample into a second workgroup
BOUND_LENGTHS = [0, 1, 1023, 1024, 1025, 2049, 65537]
# a tail of 6: the row of one sample is a block of 7 steps and the long row's second workgroup has 7 to do (`extent` below a
# block, all of it in the one-by-one remainder loop); of 1 030: the row of one sample has a second block of tail alone, the row
# of 1 023 a third, and the long row's second workgroup a whole block and one more lane
BOUND_TAILS = (6, 1030)
BOUND_LAYOUTS = {"aligned": {}, "offset-odd": dict(in_offset=1, stride=65539, out_offset=1, out_stride=66577)}
NOTCH = (G.IIR_NOTCH, 44100, 50.0, 30.0)       # poles of radius 0.99988 at 50 Hz: a block matrix with entries of very different size


def variant(bound, in_offset=0, stride=0, out_offset=0, out_stride=0, tail=0):
    """the kernels a call on a set of that bound launches (a row_stride above 0): the rest pass, whose VEC is decided by what it
    loads alone, the output pass (aligned16 over both buffers), and the propagate wherever the grid has two blocks"""
    vec_in = in_offset % 4 == 0 and stride % 4 == 0
    vec_out = vec_in and out_offset % 4 == 0 and out_stride % 4 == 0
    launched = {("block", bound, vec_in, False), ("block", bound, vec_out, True)}
    if -(-(stride + tail) // BLOCK) >= 2:
        launched.add(("propagate", bound))
    return launched


def edge_rows(bound=8):
    """(filters, rows, which) for a set of that section bound: 8 is the rows of every length of LENGTHS on one, three and eight
    sections; below it the rows of BOUND_LENGTHS on two filters, at bound 1 a one-pole section and a notch close to the circle"""
    if bound == 8:
        rng = np.random.default_rng(41)
        filters = [random_filter(S, rng, radius=0.999) for S in (1, 3, 8)]
        rows = [noise(n, rng) for n in LENGTHS]
        rows[4][0] = np.float32(-0.0)
        which = [0, 1, 2, 2, 1, 0, 2, 1, 2, 0]
        return filters, rows, which
    rng = np.random.default_rng(41 + bound)
    if bound == 1:
        filters = [np.array([[1.0, -1.0, 0.0, -0.9995, 0.0]]), np.array([G.iir_design(*NOTCH)])]
    else:
        filters = [random_filter(S, rng, radius=0.999) for S in {2: (2, 1), 4: (4, 3)}[bound]]
    rows = [noise(n, rng) for n in BOUND_LENGTHS]
    rows[4][0] = np.float32(-0.0)
    rows[6][[3, 1024, 65536]] = (np.nan, -np.inf, np.inf)              # (the last in the second workgroup's count)
    which = [0, 1, 1, 0, 1, 0, 1]
    return filters, rows, which


@pytest.fixture(scope="module")
def edges():
    """the rows of every length, and what the model makes of them, computed once per tail"""
    filters, rows, which = edge_rows()
    made = {}

    def want(tail):
        if tail not in made:
            made[tail] = iir_blocked_model(rows, filters, which, tail)
        return made[tail]
    return filters, rows, which, want


# ---- rows, blocks and workgroups ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tail", [0, 7, 1500])
def test_rows_either_side_of_a_block_and_of_a_workgroup(gpu_ctx, dev, sets, edges, tail):
    """one launch, filters of one, three and eight sections mixed by filter_dev; a tail of 1 500 crosses a block's edge (and
    gives the row of one sample a second block of +0.0 input)"""
    filters, rows, which, want = edges
    w = want(tail)
    assert [r[1] for r in w] == [n + tail if n else 0 for n in LENGTHS] and not np.signbit(w[4][0][0])
    same(w, launch(gpu_ctx, dev, sets(filters), rows, which, tail=tail), tail)


def test_the_scalar_path_gives_the_aligned_paths_bits(gpu_ctx, dev, sets, edges):
    """the base one float off 16-byte alignment and odd strides, on either side and on each alone"""
    filters, rows, which, want = edges
    iir_set = sets(filters)
    for kw in (dict(in_offset=1, stride=70001, out_offset=1, out_stride=70011), dict(in_offset=1), dict(stride=70003),
               dict(out_offset=3), dict(out_stride=70009)):
        same(want(7), launch(gpu_ctx, dev, iir_set, rows, which, tail=7, **kw), kw)


# ---- the lower section bounds -----------------------------------------------------------------------------------------------------
_BOUND_MODEL = {}


def bound_model(bound, tail):
    """the rows of a lower bound and what the model makes of them, computed once"""
    if (bound, tail) not in _BOUND_MODEL:
        filters, rows, which = edge_rows(bound)
        _BOUND_MODEL[bound, tail] = (filters, rows, which, iir_blocked_model(rows, filters, which, tail))
    return _BOUND_MODEL[bound, tail]


@pytest.mark.parametrize("layout", sorted(BOUND_LAYOUTS))
@pytest.mark.parametrize("bound", [1, 2, 4])
def test_the_lower_section_bounds_on_both_paths(gpu_ctx, dev, sets, bound, layout):
    """biquad_block_kernel<bound, VEC, OUT> for both VEC and both passes and biquad_block_propagate_kernel<bound>, bit for bit
    against the model: rows that end either side of a block's edge, a row one sample into a second workgroup (whose one lane
    of the rest pass and two of the output pass are the only active ones), blocks of tail alone, rows of fewer blocks than the
    grid (their second workgroup leaves at once, the row of no samples' first one too).  At bound 1 also against
    grail_iir_async on the device, as test_against_the_serial_call_on_the_device does: the first block identical, the rest
    within BOUND of the row's peak and half a unit in the last place of each."""
    kw = BOUND_LAYOUTS[layout]
    stride, out_stride = kw.get("stride", 65600), kw.get("out_stride", 66624)
    offsets = {k: v for k, v in kw.items() if k.endswith("offset")}
    vec = layout == "aligned"
    # (the arithmetic of the lines this case is named for in tests/KERNEL_PATHS.md)
    steps = {tail: [n + tail if n else 0 for n in BOUND_LENGTHS] for tail in BOUND_TAILS}
    assert [-(-k // BLOCK) for k in steps[6]] == [0, 1, 2, 2, 2, 3, 65] and [-(-k // BLOCK) for k in steps[1030]] == [0, 2, 3, 3, 3, 4, 66]
    assert steps[6][1] == 7 and steps[6][6] - 64 * BLOCK == 7 and 7 % 4                           # an extent of 7: the remainder loop
    assert steps[1030][1] > BLOCK >= 1 and steps[1030][2] > 2 * BLOCK >= 1023                      # blocks of tail alone
    for tail in BOUND_TAILS:
        filters, rows, which, want = bound_model(bound, tail)
        assert bound_of(filters) == bound and -(-(stride + tail) // BLOCK) > 64                    # two workgroups a row
        assert variant(bound, kw.get("in_offset", 0), stride, kw.get("out_offset", 0), out_stride, tail) == \
            {("block", bound, vec, False), ("block", bound, vec, True), ("propagate", bound)}
        assert [r[1] for r in want] == steps[tail] and want[6][2] == 3
        iir_set = sets(filters)
        blocked = launch(gpu_ctx, dev, iir_set, rows, which, tail=tail, stride=stride, out_stride=out_stride, **offsets)
        same(want, blocked, (bound, layout, tail))
        if bound != 1:
            continue
        serial = launch(gpu_ctx, dev, iir_set, rows, which, tail=tail, stride=stride, out_stride=out_stride, call="iir", **offsets)
        assert np.array_equal(serial[1], blocked[1]) and np.array_equal(serial[2], blocked[2])
        for i in range(len(rows)):
            n_out = int(serial[1][i])
            ys, yb = serial[0][i, :n_out], blocked[0][i, :n_out]
            same_samples(yb[:BLOCK], ys[:BLOCK], (layout, tail, i, "the first block"))
            if n_out <= BLOCK:
                continue
            peak = float(np.max(np.abs(ys)))
            apart = np.abs(yb.astype(np.float64) - ys.astype(np.float64))
            allowed = BOUND * peak + 0.5 * (np.spacing(np.abs(ys)).astype(np.float64) + np.spacing(np.abs(yb)).astype(np.float64))
            worst = int(np.argmax(apart - allowed))
            print(f"\n{layout} tail {tail} row {i} ({len(rows[i])} samples): the largest |blocked - serial| {apart.max() / peak:.3e} of the peak")
            assert apart[worst] <= allowed[worst], (layout, tail, i, worst, ys[worst], yb[worst])


@pytest.mark.parametrize("bound", BOUNDS)
def test_a_workgroup_whose_first_step_lies_past_the_stride(gpu_ctx, dev, sets, bound):
    """a row that fills its stride of 65 536 samples and rings out for 7 more: block 64 is the second workgroup's, it starts at
    or past the row's last group (sample) of four, so `start_in` is held at row_last and every load of the workgroup reads that
    one.  No other case has a workgroup start past row_last (the rows of 65 537 and 70 000 samples lie in longer strides)."""
    filters = edge_rows(bound)[0] if bound != 8 else edge_rows(8)[0][1:]
    assert bound_of(filters) == bound
    rng = np.random.default_rng(46 + bound)
    rows = [noise(65536, rng), noise(1, rng)]
    rows[0][[65535, 1024]] = (np.nan, np.float32(-0.0))
    want = iir_blocked_model(rows, filters, [0, 1], 7)
    assert [w[1:] for w in want] == [(65543, 1), (8, 0)]
    iir_set = sets(filters)
    for in_offset, row_last in ((0, 65532), (1, 65535)):
        assert variant(bound, in_offset, 65536, 0, 65600, 7) == {("block", bound, not in_offset, False), ("block", bound, not in_offset, True),
                                                              ("propagate", bound)}
        assert 64 * BLOCK > row_last                                                   # the second workgroup's first step
        same(want, launch(gpu_ctx, dev, iir_set, rows, [0, 1], tail=7, stride=65536, out_stride=65600, in_offset=in_offset), (bound, in_offset))


# ---- cuts, counts, refusals -----------------------------------------------------------------------------------------------------
def test_cuts_counts_refusals_and_canaries(gpu_ctx, dev, sets):
    rng = np.random.default_rng(42)
    filters = [random_filter(2, rng, radius=0.999), random_filter(4, rng, radius=0.999)]
    rows = [noise(n, rng) for n in (5000, 2049, 3000, 0, 1024, 2500)]
    rows[0][[0, 1023, 1024, 2047, 2600, 4999]] = (np.nan, np.inf, -np.inf, np.nan, np.inf, np.nan)   # (two past every cut)
    rows[2][[2048, 2999]] = (-np.inf, np.nan)
    which = [0, 1, 2, 0, 0xFFFFFFFF, 1]
    iir_set = sets(filters)
    for out_stride in (2500, 2049, 1024, 5050):          # below n, at a row's n, at a block's edge, inside the tail
        want = iir_blocked_model(rows, filters, which, 100, out_stride=out_stride)
        same(want, launch(gpu_ctx, dev, iir_set, rows, which, tail=100, out_stride=out_stride), out_stride)
        assert [w[1] for w in want] == [min(5100, out_stride), min(2149, out_stride), REFUSED, 0, REFUSED, min(2600, out_stride)]
        assert [w[2] for w in want] == [6, 0, 0, 0, 0, 0]
    # no outputs at all: the lengths (all 0) and the counts only
    out, out_len, bad = launch(gpu_ctx, dev, iir_set, rows, [0, 1, 0, 0, 1, 1], tail=100, out_stride=0)
    assert out_len.tolist() == [0] * 6 and bad.tolist() == [6, 0, 2, 0, 0, 0]


def test_scratch_left_by_a_longer_call(gpu_ctx, dev, sets):
    """a long call, then at once, on the same stream, a short one with another set: both are right"""
    rng = np.random.default_rng(43)
    long_filters, short_filters = [random_filter(8, rng, radius=0.999)], [random_filter(1, rng, radius=0.999), random_filter(2, rng)]
    long_rows, short_rows = [noise(70000, rng), noise(66000, rng)], [noise(3000, rng), noise(1025, rng), noise(2049, rng)]
    long_rows[0][69000] = short_rows[2][2048] = np.nan
    long_set, short_set = sets(long_filters), sets(short_filters)
    d_in, d_len = dev.up(np.concatenate([np.resize(x, 70016) for x in long_rows])), dev.up(np.array([70000, 66000], np.uint32))
    d_out, d_res = dev.up(np.full(2 * 70016, CANARY, np.float32)), dev.up(np.zeros(4, np.uint32))
    gpu_ctx.iir_blocked_async(long_set, d_in, 70016, d_len, 2, None, 16, d_out, 70016, d_res, C.c_void_p(d_res.value + 8))
    short = launch(gpu_ctx, dev, short_set, short_rows, [0, 1, 1], tail=16)           # (waits for both)
    same(iir_blocked_model(short_rows, short_filters, [0, 1, 1], 16), short, "short")
    res = dev.down(d_res, 4, np.uint32)
    same(iir_blocked_model(long_rows, long_filters, None, 16), (dev.down(d_out, (2, 70016), np.float32), res[:2], res[2:]), "long")
    # ... and the long one again over what the short one left
    same(iir_blocked_model(long_rows, long_filters, None, 16), launch(gpu_ctx, dev, long_set, long_rows, tail=16), "long again")


# ---- against the serial call ----------------------------------------------------------------------------------------------------
def test_against_the_serial_call_on_the_device(gpu_ctx, dev, sets):
    """Rows of at most a block: identical.  The first block of every row: identical.  Whole rows: the two calls' outputs
    before the rounding lie within 1e-9 of the row's peak (tests/test_iir_blocked_host.py), and each call's rounding to
    binary32 moves its own output by at most half a unit in its last place: |blocked - serial| <= 1e-9 peak + half a unit
    of each of the two."""
    rng = np.random.default_rng(44)
    filters = [np.array(butterworth(G.IIR_HIGHPASS, 20.0, 4)), np.array([G.iir_design(G.IIR_NOTCH, 44100, 50.0, 30.0)]),
               np.array(butterworth(G.IIR_LOWPASS, 3400.0, 8)), np.array([[1.0, -1.0, 0.0, -0.9995, 0.0]])]
    t = np.arange(70000)
    hum = (0.5 + 0.4 * np.sin(2.0 * np.pi * 50.0 * t / 44100.0)).astype(np.float32)
    rows = [hum, hum[:66000], noise(70000, rng), hum[:5000], noise(1024, rng), noise(500, rng), hum[:1025], noise(2049, rng)]
    which = [0, 1, 2, 3, 2, 0, 1, 3]
    iir_set = sets(filters)
    for tail in (0, 300):
        serial = launch(gpu_ctx, dev, iir_set, rows, which, tail=tail, call="iir")
        blocked = launch(gpu_ctx, dev, iir_set, rows, which, tail=tail)
        assert np.array_equal(serial[1], blocked[1]) and np.array_equal(serial[2], blocked[2])
        for i, x in enumerate(rows):
            n_out = int(serial[1][i])
            ys, yb = serial[0][i, :n_out], blocked[0][i, :n_out]
            assert np.all(blocked[0][i, n_out:] == CANARY)
            same_samples(yb[:BLOCK], ys[:BLOCK], (tail, i, "the first block"))
            if n_out <= BLOCK:
                continue
            peak = float(np.max(np.abs(ys)))
            apart = np.abs(yb.astype(np.float64) - ys.astype(np.float64))
            allowed = BOUND * peak + 0.5 * (np.spacing(np.abs(ys)).astype(np.float64) + np.spacing(np.abs(yb)).astype(np.float64))
            worst = int(np.argmax(apart - allowed))
            print(f"\ntail {tail} row {i} ({len(x)} samples): {int(np.count_nonzero(ys.view(np.uint32) != yb.view(np.uint32)))} of "
                  f"{n_out} outputs differ, the largest |blocked - serial| {apart.max() / peak:.3e} of the peak")
            assert apart[worst] <= allowed[worst], (tail, i, worst, ys[worst], yb[worst])


# ---- one long row ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [2, 8])
def test_one_long_row(gpu_ctx, dev, sets, S):
    """2^20 + 3 samples: 1 025 blocks, 17 workgroups, one wave's chain of 1 024 entry states"""
    rng = np.random.default_rng(45 + S)
    filters = [random_filter(S, rng, radius=0.9995)]
    rows = [noise((1 << 20) + 3, rng)]
    rows[0][[5, 1 << 19, 1 << 20]] = (np.nan, np.inf, np.float32(-0.0))
    want = iir_blocked_model(rows, filters, None, 5)
    assert want[0][1:] == ((1 << 20) + 8, 2)
    same(want, launch(gpu_ctx, dev, sets(filters), rows, tail=5), S)


# ---- the example ------------------------------------------------------------------------------------------------------------------
def test_grail_dialogue_eq_blocked_option(gpu_ctx, tmp_path):
    """the same --eq options through either call: WAVs of equal length whose samples differ by at most one step of the 16-bit
    scale (the two calls lie within 1e-9 of full scale of one another before the rounding, which can only move a sample that
    sits on a rounding boundary), and each run says which call it used"""
    exe = os.path.join(ROOT, "grail-rs_amd", "lib", "grail_dialogue")
    args = ["--eq", "highpass:100:0.707", "--eq", "peak:3000:1.5:4", "--eq", "notch:50:30", "hello there", "a fine day to you"]
    frames = {}
    for name, extra in (("serial", []), ("blocked", ["--eq-blocked"])):
        r = subprocess.run([exe, "-o", str(tmp_path / f"{name}.wav")] + extra + args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        m = re.search(r"Equalised \((\w+)\), 3 sections: highpass:100:0.707 peak:3000:1.5:4 notch:50:30", r.stdout)
        assert m and m.group(1) == ("grail_biquad_blocked_async" if extra else "grail_iir_async"), r.stdout
        with wave.open(str(tmp_path / f"{name}.wav"), "rb") as w:
            assert w.getnchannels() == 2 and w.getsampwidth() == 2
            frames[name] = np.frombuffer(w.readframes(w.getnframes()), np.int16).astype(np.int32)
    assert len(frames["serial"]) == len(frames["blocked"]) > 2 * 2 * BLOCK
    apart = np.abs(frames["serial"] - frames["blocked"])
    print(f"\n{int(np.count_nonzero(apart))} of {len(apart)} 16-bit samples differ, by {int(apart.max())} at most")
    assert apart.max() <= 1 and np.any(frames["serial"] != 0)
