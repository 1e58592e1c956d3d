"""Recursive filtering on the device (grail_iir_async) against the numpy model of tests/iir_model.py, bit for bit in the
filtered samples (NaN positions compared as NaN), the lengths and the non-finite counts: partial last waves, rows that end at,
before and after a tile's edge and all of them in one wave, a len beyond the stride, the scalar path against the aligned one
under every section bound (and strides of 1 and 4, where every load is clamped),
out_stride cutting inside a row and inside its tail, tails with and without samples before them, a decay through the
denormals of both formats, filters of one to eight sections in one wave, rows on different filters and on none, non-finite
samples, a filter that overflows, and a row's bits wherever it lies in the launch.  Every output buffer holds a canary
wherever nothing may be written, and is checked there."""
import ctypes as C

import numpy as np
import pytest

import grail_hip as G
from iir_model import REFUSED, iir_model
from test_iir_host import NEGATIVE_ZEROS
from test_levels_gpu import CANARY, Dev, dev  # noqa: F401  (dev is a fixture)

pytestmark = pytest.mark.gpu
TILE = 64                                       # the samples of a row that one pass of the kernel's loop takes
LENGTHS = [0, 1, 63, 64, 65, 127, 128, 129, 300]
IDENTITY = [1.0, 0.0, 0.0, 0.0, 0.0]
# iir_kernel<section bound, VEC, STREAM>: the sixteen that tests/test_iir_code_objects.py finds in the library
BOUNDS = (1, 2, 4, 8)
VARIANTS = [(sb, vec, stream) for sb in BOUNDS for vec in (True, False) for stream in (False, True)]


def bound_of(filters):
    """the section bound a set of these filters is launched with: iir_set_image's power of two at or above the largest filter's
    sections, through iir_launch_bound's dispatch (<= 1, == 2, <= 4, else 8)"""
    most = max(len(np.asarray(f, np.float64).reshape(-1, 5)) for f in filters)
    bound = 1
    while bound < most:
        bound <<= 1
    return 1 if bound <= 1 else (2 if bound == 2 else (4 if bound <= 4 else 8))


def variant(bound, in_offset=0, stride=0, out_offset=0, out_stride=0, stream=False):
    """the iir_kernel<SB, VEC, STREAM> that launch_iir starts for a set of that bound: VEC by aligned16 over both buffers (the
    offsets are floats from a 16-byte aligned base; a finishing call has no input: in_offset = stride = 0)"""
    vec = in_offset % 4 == 0 and stride % 4 == 0 and out_offset % 4 == 0 and out_stride % 4 == 0
    return (bound, vec, stream)


def random_filter(S, rng, radius=0.95):
    """S sections, b uniform in +-1, each pole pair (or pair of real poles) inside `radius`"""
    sec = np.zeros((S, 5))
    for j in range(S):
        sec[j, :3] = rng.uniform(-1.0, 1.0, 3)
        r, th = rng.uniform(0.1, radius), rng.uniform(0.0, np.pi)
        sec[j, 3], sec[j, 4] = -2.0 * r * np.cos(th), r * r
    return sec


def noise(n, rng):
    return rng.uniform(-1.0, 1.0, n).astype(np.float32)


def run(ctx, dev, iir_set, rows, which=None, tail=0, stride=None, out_stride=None, in_offset=0, out_offset=0, guard=64, lens=None):
    """rows[i] as row i of a buffer that holds NaN everywhere else, filtered with filter which[i] of the set (None: filter_dev
    NULL) into a buffer that holds CANARY, with `guard` floats of it before and after -> (out [n_rows, out_stride] as it lies on
    the device afterwards, out_len, nonfinite)."""
    longest = max([len(x) for x in rows] + [1])
    stride = stride or (longest + 63) // 64 * 64
    out_stride = (longest + tail + 63) // 64 * 64 if out_stride is None else out_stride
    host = np.full(len(rows) * stride + in_offset, np.nan, np.float32)
    for i, x in enumerate(rows):
        host[in_offset + i * stride:in_offset + i * stride + len(x)] = x
    d_in = dev.up(host)
    before = guard + out_offset
    d_out = dev.up(np.full(before + len(rows) * out_stride + guard, CANARY, np.float32))
    d_len = dev.up(np.array([len(x) for x in rows] if lens is None else lens, np.uint32))
    d_which = None if which is None else dev.up(np.array(which, np.uint32))
    out_len, bad = ctx.iir(iir_set, C.c_void_p(d_in.value + in_offset * 4), stride, d_len, len(rows), d_which, tail,
                           C.c_void_p(d_out.value + before * 4), out_stride)
    out = dev.down(d_out, before + len(rows) * out_stride + guard, np.float32)
    assert np.all(out[:before] == CANARY) and np.all(out[before + len(rows) * out_stride:] == CANARY), "written outside out"
    return out[before:before + len(rows) * out_stride].reshape(len(rows), out_stride), out_len, bad


def same_samples(got, want, what):
    """bit for bit, but where the model holds a NaN any NaN will do"""
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, "NaNs at", np.flatnonzero(np.isnan(got) != nan)[:8])
    differ = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)) & ~nan)
    assert len(differ) == 0, (what, differ[:8], got[differ[:4]], want[differ[:4]])


def same(rows, filters, which, tail, got, what, lens=None):
    """the device's (out, out_len, nonfinite) against the model's; out rows hold the canary past their outputs; a row whose
    index is outside the set holds nothing else"""
    out, out_len, bad = got
    want = iir_model(rows, filters, which, tail, out_stride=out.shape[1], lens=lens)
    for i, (y, n_out, w_bad) in enumerate(want):
        assert (out_len[i], bad[i]) == (n_out, w_bad), (what, i, len(rows[i]), out_len[i], n_out, bad[i], w_bad)
        if n_out == REFUSED:
            assert np.all(out[i] == CANARY), (what, i, "a refused row")
            continue
        assert np.all(out[i, n_out:] == CANARY), (what, i, len(rows[i]), "written past the row's outputs")
        same_samples(out[i, :n_out], y, (what, i, len(rows[i])))
    return want


@pytest.fixture
def sets(gpu_ctx):
    made = []

    def create(filters):
        made.append(gpu_ctx.iir_create(filters))
        return made[-1]
    yield create
    for s in made:
        gpu_ctx.iir_free(s)


# ---- rows and lengths ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 130])
def test_row_counts(gpu_ctx, dev, sets, n_rows):
    """whole and partial last waves: the loads of the rows past the launch's last are clamped, their stores masked"""
    rng = np.random.default_rng(n_rows)
    filters = [random_filter(S, rng) for S in (1, 2, 3)]
    rows = [noise(int(rng.integers(0, 200)), rng) for _ in range(n_rows)]
    rows[-1] = noise(199, rng)
    which = rng.integers(0, 3, n_rows).tolist()
    same(rows, filters, which, 5, run(gpu_ctx, dev, sets(filters), rows, which, tail=5), n_rows)


@pytest.mark.parametrize("n", LENGTHS)
def test_lengths_either_side_of_a_tile(gpu_ctx, dev, sets, n):
    rng = np.random.default_rng(1000 + n)
    filters = [random_filter(2, rng)]
    rows = [noise(n, rng) for _ in range(3)]
    iir_set = sets(filters)
    for tail in (0, 3):
        same(rows, filters, None, tail, run(gpu_ctx, dev, iir_set, rows, tail=tail), (n, tail))


def test_a_wave_of_every_length_and_a_len_beyond_the_stride(gpu_ctx, dev, sets):
    """the wave's trip count is its longest row's; every shorter row stops being stored where it ends.  Then len_dev holds
    more than the stride: the row is the stride long."""
    rng = np.random.default_rng(5)
    filters = [random_filter(3, rng), random_filter(1, rng)]
    rows = [noise(n, rng) for n in LENGTHS * 7][:63] + [noise(300, rng)]
    which = [i % 2 for i in range(64)]
    iir_set = sets(filters)
    same(rows, filters, which, 70, run(gpu_ctx, dev, iir_set, rows, which, tail=70), "all lengths")
    rows = [noise(128, rng), noise(100, rng), noise(128, rng)]
    lens = [5000, 100, 0xFFFFFFFF]
    got = run(gpu_ctx, dev, iir_set, rows, [0, 1, 0], tail=9, stride=128, out_stride=192, lens=lens)
    want = same(rows, filters, [0, 1, 0], 9, got, "len > row_stride", lens=lens)
    assert [w[1] for w in want] == [137, 109, 137]


# the layouts of the scalar-path case: both sides off, then each side's base and each side's stride alone
SCALAR_LAYOUTS = (dict(in_offset=1, stride=301, out_offset=1, out_stride=321), dict(in_offset=1, stride=304, out_stride=384),
                  dict(stride=301, out_stride=384), dict(stride=304, out_offset=3, out_stride=384), dict(stride=304, out_stride=322))
SCALAR_SECTIONS = {1: (1, 1), 2: (2, 1), 4: (4, 3), 8: (8, 5)}             # the two filters of a set, by its largest's sections


@pytest.mark.parametrize("most", BOUNDS)
def test_the_scalar_path_gives_the_aligned_paths_bits(gpu_ctx, dev, sets, most):
    """a base 4 bytes off 16-byte alignment and a stride of 301 on either side, and each side alone, under every section bound:
    iir_kernel<most, false, false> by all five layouts, <most, true, false> by the aligned one.  Then the smallest strides
    there are, 1 (scalar) and 4 (VEC), under rows of 1 and 4 samples that ring out over two tiles: every load of every tile
    is past the stride or past the launch's last row or both, and reads the row's last sample or group."""
    rng = np.random.default_rng(6 + most)
    filters = [random_filter(S, rng) for S in SCALAR_SECTIONS[most]]
    assert bound_of(filters) == most
    rows = [noise(n, rng) for n in (301, 300, 0, 17, 64, 299, 301)]
    which = [0, 1, 1, 0, 1, 0, 1]
    iir_set = sets(filters)
    assert variant(most, 0, 304, 0, 384) == (most, True, False)
    aligned = run(gpu_ctx, dev, iir_set, rows, which, tail=20, stride=304, out_stride=384)
    want = same(rows, filters, which, 20, aligned, "aligned")
    for kw in SCALAR_LAYOUTS:
        assert variant(most, kw.get("in_offset", 0), kw["stride"], kw.get("out_offset", 0), kw["out_stride"]) == (most, False, False)
        out, out_len, bad = run(gpu_ctx, dev, iir_set, rows, which, tail=20, **kw)
        same(rows, filters, which, 20, (out, out_len, bad), kw)
        for i, (y, n_out, _) in enumerate(want):
            same_samples(out[i, :n_out], aligned[0][i, :n_out], (kw, i))
    # strides of 1 and 4: tail 70 makes two tiles (the second one's prefetch lies past the stride as a whole), seven rows
    # leave 57 lanes of the wave on the clamped last row, and 71 and 74 outputs end in a partial group of four
    ones = [noise(n, rng) for n in (1, 1, 0, 1, 1, 1, 1)]
    fours = [noise(n, rng) for n in (4, 1, 0, 4, 3, 4, 1)]
    ones[1][0] = fours[3][3] = np.nan
    for short, kw in ((ones, dict(stride=1, out_stride=75)), (ones, dict(stride=1, out_stride=72)), (fours, dict(stride=4, out_stride=76)),
                      (fours, dict(stride=4, out_stride=75))):
        vec = kw["stride"] == 4 and kw["out_stride"] % 4 == 0
        assert variant(most, 0, kw["stride"], 0, kw["out_stride"]) == (most, vec, False)
        assert 64 < max(len(x) for x in short) + 70 <= 128 and len(short) % 64 != 0
        got = same(short, filters, which, 70, run(gpu_ctx, dev, iir_set, short, which, tail=70, **kw), kw)
        assert [w[1] for w in got] == [len(x) + 70 if len(x) else 0 for x in short]


def test_out_stride_cuts_inside_the_row_and_inside_the_tail(gpu_ctx, dev, sets):
    rng = np.random.default_rng(8)
    filters = [random_filter(2, rng)]
    rows = [noise(n, rng) for n in (200, 90, 100, 0, 130)]
    rows[0][[3, 150, 199]] = (np.nan, np.inf, -np.inf)            # (two of them past the cut: counted all the same)
    iir_set = sets(filters)
    for out_stride in (100, 101, 128, 129, 217):
        want = same(rows, filters, None, 50, run(gpu_ctx, dev, iir_set, rows, tail=50, out_stride=out_stride), out_stride)
        assert want[0][1] == min(250, out_stride) and want[0][2] == 3 and want[1][1] == min(140, out_stride) and want[3][1] == 0
    # no outputs at all: the lengths (all 0) and the counts only
    d_in = dev.up(np.concatenate([np.resize(x, 200) for x in rows]))
    d_len = dev.up(np.array([len(x) for x in rows], np.uint32))
    out_len, bad = gpu_ctx.iir(iir_set, d_in, 200, d_len, len(rows), None, 50, None, 0)
    assert out_len.tolist() == [0] * 5 and bad.tolist() == [3, 0, 0, 0, 0]


# ---- tails --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tail", [0, 1, 64, 200])
def test_tails(gpu_ctx, dev, sets, tail):
    """the loop goes on past the longest row's samples on +0.0; rows of no samples write nothing"""
    rng = np.random.default_rng(2000 + tail)
    filters = [random_filter(2, rng), random_filter(4, rng)]
    rows = [noise(n, rng) for n in (0, 1, 64, 100, 0, 127)]
    which = [0, 1, 0, 1, 1, 0]
    want = same(rows, filters, which, tail, run(gpu_ctx, dev, sets(filters), rows, which, tail=tail), tail)
    assert [w[1] for w in want] == [0, 1 + tail, 64 + tail, 100 + tail, 0, 127 + tail]


def test_a_decay_through_the_denormals_of_both_formats(gpu_ctx, dev, sets):
    """a pole pair of radius 0.5 rings out from an impulse over a tail of 1 200: the outputs pass through binary32's denormals
    (2^-127 ... 2^-149) and the state through binary64's (below 2^-1022, from about the 1 030th step on).  Flushed anywhere,
    the bits differ."""
    filters = [[[1.0, 0.0, 0.0, -2.0 * 0.5 * np.cos(1.0), 0.25]]]
    rows = [np.array([1.0], np.float32), np.array([0.75, -0.5], np.float32)]
    exact = iir_model(rows, filters, None, 1200, exact=True)[0][0]
    tiny64 = np.flatnonzero((np.abs(exact) < 2.2250738585072014e-308) & (exact != 0.0))
    assert len(tiny64) > 30 and tiny64[0] > 1000
    want = same(rows, filters, None, 1200, run(gpu_ctx, dev, sets(filters), rows, tail=1200), "denormals")
    y = want[0][0]
    assert np.count_nonzero((np.abs(y) < np.float32(1.1754944e-38)) & (y != 0)) >= 15 and want[0][1] == 1201
    # ... and a second section behind it takes the binary64 denormals in, unrounded: its state is the first's output
    two = [[filters[0][0], [0.5, 0.25, 0.0, -0.5, 0.0]]]
    same(rows, two, None, 1200, run(gpu_ctx, dev, sets(two), rows, tail=1200), "denormals, two sections")


# ---- sections and filters -------------------------------------------------------------------------------------------------------
def test_one_wave_of_one_to_eight_sections(gpu_ctx, dev, sets):
    """filters of S = 1 .. 8 in one wave, random binary64 coefficients: a contracted multiply-add moves the bits, and so does
    a section run as an identity: the rows of -0.0 and of silence through b0 = 1 and through a section that answers silence
    with -0.0."""
    rng = np.random.default_rng(9)
    filters = [random_filter(S, rng) for S in range(1, 9)] + [[IDENTITY], [NEGATIVE_ZEROS], [NEGATIVE_ZEROS, IDENTITY],
                                                               [IDENTITY] * 3 + [NEGATIVE_ZEROS]]
    rows, which = [], []
    for i in range(64):
        rows.append(noise(int(rng.integers(100, 260)), rng))
        which.append(i % 8)
    minus = np.full(40, -0.0, np.float32)
    for f in (8, 9, 10, 11, 0, 7):
        rows[8 + f] = minus.copy() if f not in (9, 10) else np.zeros(40, np.float32)
        which[8 + f] = f
    want = same(rows, filters, which, 30, run(gpu_ctx, dev, sets(filters), rows, which, tail=30), "sections")
    # (what the cases are there for, in the model: the identity does not copy -0.0, and a section's output followed by an
    # identity is not the section's output)
    assert not np.signbit(want[8 + 8][0][0]) and np.signbit(want[8 + 9][0][2])
    assert not np.array_equal(want[8 + 9][0].view(np.uint32), want[8 + 10][0].view(np.uint32))
    # the same rows through a set whose largest filter has fewer sections (another instantiation): the same bits
    for most in (1, 2, 4):
        few = [i for i in range(64) if which[i] < most]
        got = run(gpu_ctx, dev, sets(filters[:most]), [rows[i] for i in few], [which[i] for i in few], tail=30)
        for k, i in enumerate(few):
            same_samples(got[0][k, :want[i][1]], want[i][0], (most, i))


def test_filter_per_row_none_and_outside_the_set(gpu_ctx, dev, sets):
    rng = np.random.default_rng(10)
    filters = [random_filter(2, rng), random_filter(1, rng), random_filter(3, rng)]
    rows = [noise(n, rng) for n in (100, 64, 129, 7, 100, 65)]
    iir_set = sets(filters)
    same(rows, filters, None, 4, run(gpu_ctx, dev, iir_set, rows, None, tail=4), "filter_dev NULL")
    which = [2, 3, 0, 0xFFFFFFFF, 1, 64]
    want = same(rows, filters, which, 4, run(gpu_ctx, dev, iir_set, rows, which, tail=4), "refused rows")
    assert [w[1] for w in want] == [104, REFUSED, 133, REFUSED, 104, REFUSED]


def test_nonfinite_samples_are_counted_once_and_enter_as_zero(gpu_ctx, dev, sets):
    rng = np.random.default_rng(11)
    filters = [random_filter(2, rng)]
    rows = [noise(n, rng) for n in (130, 64, 65, 1, 200)]
    rows[0][[0, 63, 64, 129]] = (np.nan, np.inf, -np.inf, np.nan)
    rows[1][:] = np.nan
    rows[2][64] = np.inf
    rows[3][0] = -np.inf
    iir_set = sets(filters)
    want = same(rows, filters, None, 10, run(gpu_ctx, dev, iir_set, rows, tail=10), "non-finite")
    assert [w[2] for w in want] == [4, 64, 1, 1, 0] and all(np.all(np.isfinite(w[0])) for w in want)
    cut = same(rows, filters, None, 10, run(gpu_ctx, dev, iir_set, rows, tail=10, out_stride=32), "non-finite, cut")
    assert [w[2] for w in cut] == [4, 64, 1, 1, 0] and [w[1] for w in cut] == [32, 32, 32, 11, 32]


def test_an_unstable_filter_overflows_as_the_model_does(gpu_ctx, dev, sets):
    """a pole at 1.5: the outputs reach +-inf in binary32 after some 220 samples, the state in binary64 after some 1 750, and
    the section behind it, whose b2 is 0, makes 0 * inf = NaN from there on.  The same bits until then and NaNs at the same
    places."""
    filters = [[[1.0, 0.0, 0.0, -1.5, 0.0], [0.5, -0.25, 0.0, 0.1, 0.0]], [[1.0, 0.0, 0.0, -1.5, 0.0]]]
    rows = [np.r_[np.float32(1.0), np.zeros(1899, np.float32)], np.r_[np.float32(-1.0), np.zeros(1899, np.float32)]]
    want = same(rows, filters, [0, 1], 0, run(gpu_ctx, dev, sets(filters), rows, [0, 1]), "unstable")
    y = want[0][0]
    first_inf, first_nan = int(np.flatnonzero(np.isinf(y))[0]), int(np.flatnonzero(np.isnan(y))[0])
    assert 200 < first_inf < 240 and 1700 < first_nan < 1800 and np.all(np.isnan(y[first_nan + 2:]))
    # (the lone section too: its a2 is 0, and 0 * inf is a NaN in s2)
    alone = want[1][0]
    assert np.all(np.isneginf(alone[300:1700])) and 1700 < int(np.flatnonzero(np.isnan(alone))[0]) < 1800


def test_a_rows_bits_do_not_depend_on_where_it_lies(gpu_ctx, dev, sets):
    """the same row and filter alone, as row 0 of 130, as row 129 of 130 and among longer neighbours on other filters"""
    rng = np.random.default_rng(12)
    filters = [random_filter(3, rng), random_filter(8, rng), random_filter(1, rng)]
    row = noise(150, rng)
    row[[5, 70]] = (np.nan, np.float32(-0.0))
    iir_set = sets(filters)
    alone = run(gpu_ctx, dev, iir_set, [row], [0], tail=40)
    want = same([row], filters, [0], 40, alone, "alone")[0]
    for at in (0, 129):
        rows = [noise(int(rng.integers(0, 400)), rng) for _ in range(130)]
        which = rng.integers(0, 3, 130).tolist()
        rows[at], which[at] = row, 0
        out, out_len, bad = run(gpu_ctx, dev, iir_set, rows, which, tail=40)
        assert (out_len[at], bad[at]) == (190, 1)
        same_samples(out[at, :190], alone[0][0, :190], at)
        same_samples(out[at, :190], want[0], at)
        assert np.all(out[at, 190:] == CANARY)
