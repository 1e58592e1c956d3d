"""Post-processing calls queued behind one another with no wait from the host in between: the host-side code that protects a
kernel still queued (DeviceBuffer::reserve waits before a scratch grows, resample_table before the oldest of its four
tables goes, grail_fir_free, grail_iir_free and grail_dyn_free before a set goes; a table's upload from pageable memory, and
a filter set's block matrices; the scratch of the blocked recursive filter; the row indices a stream is opened with) runs with
work in the queue.  Every
input is uploaded and every buffer allocated before a test's first call, every result goes to a device buffer, the test
waits once at the end, and what it then downloads is the models' bits.  A context of its own per test: its scratch and its
table cache start empty."""
import numpy as np
import pytest

import grail_hip as G
from grail_hip import workload as W
import dyn_model as M
from fir_model import fir_model
from iir_blocked_model import iir_blocked_model
from iir_model import iir_model
from resample_model import resample_model
from test_levels_gpu import CANARY, Dev, _awkward, same_bits
from test_levels_host import row_model
from test_dyn_gpu import three_curves
from test_iir_gpu import random_filter
from test_limiter_host import limiter_model
from test_true_peak_host import true_peak_model

pytestmark = pytest.mark.gpu
SMALL = [700, 0, 1024]                                              # a call's rows: three of at most 1 024 samples,
LARGE = [7000, 4097, 1, 6999, 2048, 700, 5000, 7000]                # and eight of up to 7 000: more chunks of every stage


@pytest.fixture
def ctx(built):
    with G.Context(0) as c:
        yield c


@pytest.fixture
def dev(ctx):
    d = Dev(ctx)
    yield d
    d.free()


def _table(pair):
    U, D, P = G.resample_ratio(*pair)
    return G.resample_coefficients(*pair), U, D, P


def _noise(rng, n):
    """noise in +-1 with a NaN, an infinite sample and a -0.0 where there is room"""
    x = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    for at, v in ((n // 3, np.nan), (n // 2, -np.inf), (n - 1, -0.0)):
        if n > 3:
            x[at] = v
    return x


def _hot(rng, n):
    """quiet noise with a hot sample every few hundred and a NaN: something for the limiter to hold down"""
    x = (rng.standard_normal(n) * 0.05).astype(np.float32)
    x[::257] = np.float32(0.9)
    if n > 3:
        x[n // 3] = np.nan
    return x


def _up(dev, rows, stride):
    """rows[i] as row i at `stride`, NaN between a row's samples and the stride -> (rows_dev, len_dev)"""
    host = np.full((len(rows), stride), np.nan, np.float32)
    for i, x in enumerate(rows):
        host[i, :len(x)] = x
    return dev.up(host), dev.up(np.array([len(x) for x in rows], np.uint32))


def _canary(dev, n_rows, stride):
    return dev.up(np.full(n_rows * stride, CANARY, np.float32))


def _rows_equal(out, want, what):
    """out [n_rows, stride] as downloaded against the model's rows; the canary past a row's samples"""
    for i, z in enumerate(want):
        assert same_bits(out[i, :len(z)], z), (what, i)
        assert np.all(out[i, len(z):] == CANARY), (what, i, "written past the row's samples")


# ---- a. the table cache ---------------------------------------------------------------------------------------------------
def test_a_table_is_evicted_with_work_queued_on_it(ctx, dev):
    """five pairs against a cache of four, the first again after it went: six calls queued, each into its own buffers"""
    pairs = [(48000, 16000), (44100, 48000), (2, 3), (3, 2), (48000, 96000), (48000, 16000)]
    assert len(set(pairs)) == 5 and pairs[0] == pairs[5]
    rng = np.random.default_rng(31)
    lens = [700, 3072 + 5, 0, 2500]
    rows = [_noise(rng, n) for n in lens]
    stride = 3136
    d_rows, d_len = _up(dev, rows, stride)
    calls = []
    for pair in pairs:
        _, U, D, _ = _table(pair)
        out_stride = (-(-max(lens) * U // D) + 63) // 64 * 64
        calls.append((pair, out_stride, _canary(dev, len(rows), out_stride), dev.alloc(len(rows) * 4), dev.alloc(len(rows) * 4)))
    for pair, out_stride, d_out, d_out_len, d_bad in calls:
        ctx.resample_async(d_rows, stride, d_len, len(rows), pair[0], pair[1], d_out, out_stride, d_out_len, d_bad)
    ctx.sync()
    got = {}
    for k, (pair, out_stride, d_out, d_out_len, d_bad) in enumerate(calls):
        num, _, D, _ = _table(pair)
        want = [resample_model(x, num, D) for x in rows]
        out = dev.down(d_out, (len(rows), out_stride), np.float32)
        assert np.array_equal(dev.down(d_out_len, len(rows), np.uint32), [w[1] for w in want]), (k, pair)
        assert np.array_equal(dev.down(d_bad, len(rows), np.uint32), [w[2] for w in want]), (k, pair)
        _rows_equal(out, [w[0] for w in want], (k, pair))
        got[k] = out
    assert same_bits(got[0], got[5])


# ---- b. the chunk scratch ---------------------------------------------------------------------------------------------------
def _small_large_small(dev, make, stride_of=lambda n: (n + 63) // 64 * 64):
    """the rows of a small call, of a larger one and of the small one again, uploaded -> [(rows, rows_dev, len_dev, stride)]"""
    rng = np.random.default_rng(41)
    small, large = [make(rng, n) for n in SMALL], [make(rng, n) for n in LARGE]
    placed = []
    for rows in (small, large, small):
        stride = stride_of(max(len(x) for x in rows))
        placed.append((rows,) + _up(dev, rows, stride) + (stride,))
    assert len(large) * placed[1][3] > 8 * len(small) * placed[0][3]        # more chunks of any size a row is cut into
    return placed


def test_the_levels_scratch_grows_with_work_queued_on_it(ctx, dev):
    placed = _small_large_small(dev, _awkward)
    res = [(dev.alloc(len(rows) * 8), dev.alloc(len(rows) * 4), dev.alloc(len(rows) * 4)) for rows, _, _, _ in placed]
    for (rows, d_rows, d_len, stride), r in zip(placed, res):
        ctx.levels_async(d_rows, stride, d_len, len(rows), *r)
    ctx.sync()
    got = []
    for (rows, _, _, _), r in zip(placed, res):
        want = [row_model(x) for x in rows]
        g = (dev.down(r[0], len(rows), np.float64), dev.down(r[1], len(rows), np.float32), dev.down(r[2], len(rows), np.uint32))
        assert same_bits(g[0], np.array([m[0] for m in want], np.float64))
        assert same_bits(g[1], np.array([m[1] for m in want], np.float32))
        assert np.array_equal(g[2], [m[2] for m in want]) and (len(rows) == len(SMALL) or g[2].sum() > 20)
        got.append(g)
    assert all(same_bits(p, q) for p, q in zip(got[0][:2], got[2][:2])) and np.array_equal(got[0][2], got[2][2])


def test_the_true_peak_scratch_grows_with_work_queued_on_it(ctx, dev):
    placed = _small_large_small(dev, _awkward)
    res = [(dev.alloc(len(rows) * 8), dev.alloc(len(rows) * 4)) for rows, _, _, _ in placed]
    for (rows, d_rows, d_len, stride), r in zip(placed, res):
        ctx.true_peak_async(d_rows, stride, d_len, len(rows), *r)
    ctx.sync()
    got = []
    for (rows, _, _, _), r in zip(placed, res):
        want = [true_peak_model(x) for x in rows]
        g = (dev.down(r[0], len(rows), np.float64), dev.down(r[1], len(rows), np.uint32))
        assert same_bits(g[0], np.array([m[0] for m in want], np.float64)) and np.array_equal(g[1], [m[1] for m in want])
        got.append(g)
    assert same_bits(got[0][0], got[2][0]) and np.array_equal(got[0][1], got[2][1]) and got[1][0].max() > 0


def test_the_limiters_scratch_grows_with_work_queued_on_it(ctx, dev):
    c, ell = np.float32(0.5), 5
    placed = _small_large_small(dev, _hot)
    res = [(_canary(dev, len(rows), stride),) + tuple(dev.alloc(len(rows) * 4) for _ in range(3)) for rows, _, _, stride in placed]
    for (rows, d_rows, d_len, stride), r in zip(placed, res):
        ctx.limit_async(d_rows, stride, d_len, len(rows), c, ell, r[0], stride, 1, *r[1:])
    ctx.sync()
    got = []
    for (rows, _, _, stride), r in zip(placed, res):
        w_out, w_gain, w_limited, w_bad = limiter_model(rows, c, ell)
        out = dev.down(r[0], (len(rows), stride), np.float32)
        _rows_equal(out, w_out, "limit")
        assert same_bits(dev.down(r[1], len(rows), np.float32), w_gain)
        assert np.array_equal(dev.down(r[2], len(rows), np.uint32), w_limited) and np.count_nonzero(w_limited) >= 2
        assert np.array_equal(dev.down(r[3], len(rows), np.uint32), w_bad)
        got.append(out)
    assert np.array_equal(got[0].view(np.uint32), got[2].view(np.uint32))


def test_the_resamplers_scratch_grows_with_work_queued_on_it(ctx, dev):
    pair = (48000, 16000)
    num, U, D, _ = _table(pair)
    placed = _small_large_small(dev, _noise)
    res = []
    for rows, _, _, stride in placed:
        out_stride = (-(-stride * U // D) + 63) // 64 * 64
        res.append((out_stride, _canary(dev, len(rows), out_stride), dev.alloc(len(rows) * 4), dev.alloc(len(rows) * 4)))
    for (rows, d_rows, d_len, stride), r in zip(placed, res):
        ctx.resample_async(d_rows, stride, d_len, len(rows), pair[0], pair[1], r[1], r[0], r[2], r[3])
    ctx.sync()
    got = []
    for (rows, _, _, _), r in zip(placed, res):
        want = [resample_model(x, num, D) for x in rows]
        out = dev.down(r[1], (len(rows), r[0]), np.float32)
        _rows_equal(out, [w[0] for w in want], "resample")
        assert np.array_equal(dev.down(r[2], len(rows), np.uint32), [w[1] for w in want])
        assert np.array_equal(dev.down(r[3], len(rows), np.uint32), [w[2] for w in want])
        got.append(out)
    assert np.array_equal(got[0].view(np.uint32), got[2].view(np.uint32))


def test_the_firs_scratch_grows_with_work_queued_on_it(ctx, dev):
    rng = np.random.default_rng(43)
    K, origin = 20, 7
    h = rng.uniform(-1.0, 1.0, K).astype(np.float32)
    placed = _small_large_small(dev, _noise)
    res = []
    for rows, _, _, stride in placed:
        out_stride = stride + 64
        res.append((out_stride, _canary(dev, len(rows), out_stride), dev.alloc(len(rows) * 4), dev.alloc(len(rows) * 4)))
    fir_set = ctx.fir_create([(h, origin)])
    for (rows, d_rows, d_len, stride), r in zip(placed, res):
        ctx.fir_async(fir_set, d_rows, stride, d_len, len(rows), None, r[1], r[0], r[2], r[3])
    ctx.sync()
    ctx.fir_free(fir_set)
    got = []
    for (rows, _, _, _), r in zip(placed, res):
        want = [fir_model(x, h, origin) for x in rows]
        out = dev.down(r[1], (len(rows), r[0]), np.float32)
        _rows_equal(out, [w[0] for w in want], "fir")
        assert np.array_equal(dev.down(r[2], len(rows), np.uint32), [w[1] for w in want])
        assert np.array_equal(dev.down(r[3], len(rows), np.uint32), [w[2] for w in want])
        got.append(out)
    assert np.array_equal(got[0].view(np.uint32), got[2].view(np.uint32))


# ---- c. filter sets ---------------------------------------------------------------------------------------------------------
def test_a_set_is_freed_with_work_queued_on_it_and_another_created(ctx, dev):
    """create, filter, free at once (the call waits for what is queued), create a different set of the same shape (which may
    get the freed set's address), filter: each result is its own taps'"""
    rng = np.random.default_rng(47)
    first = [(rng.uniform(-1.0, 1.0, 33).astype(np.float32), 16), (rng.uniform(-1.0, 1.0, 20).astype(np.float32), 0)]
    second = [(rng.uniform(-1.0, 1.0, 33).astype(np.float32), 16), (rng.uniform(-1.0, 1.0, 20).astype(np.float32), 0)]
    rows = [_noise(rng, n) for n in (700, 2 * G.FIR_CHUNK + 17, 0, 5000)]
    which = [0, 1, 1, 0]
    stride, out_stride = 5056, 5120
    d_rows, d_len = _up(dev, rows, stride)
    d_which = dev.up(np.array(which, np.uint32))
    res = [(_canary(dev, len(rows), out_stride), dev.alloc(len(rows) * 4), dev.alloc(len(rows) * 4)) for _ in range(2)]
    a = ctx.fir_create(first)
    ctx.fir_async(a, d_rows, stride, d_len, len(rows), d_which, out_stride=out_stride, out_dev=res[0][0], out_len_dev=res[0][1],
                  nonfinite_dev=res[0][2])
    ctx.fir_free(a)
    b = ctx.fir_create(second)
    ctx.fir_async(b, d_rows, stride, d_len, len(rows), d_which, out_stride=out_stride, out_dev=res[1][0], out_len_dev=res[1][1],
                  nonfinite_dev=res[1][2])
    ctx.sync()
    ctx.fir_free(b)
    outs = []
    for filters, r in zip((first, second), res):
        want = [fir_model(x, *filters[f]) for x, f in zip(rows, which)]
        out = dev.down(r[0], (len(rows), out_stride), np.float32)
        _rows_equal(out, [w[0] for w in want], "fir")
        assert np.array_equal(dev.down(r[1], len(rows), np.uint32), [w[1] for w in want])
        assert np.array_equal(dev.down(r[2], len(rows), np.uint32), [w[2] for w in want])
        outs.append(out)
    assert not np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))


# ---- d. lengths that stay on the device ---------------------------------------------------------------------------------------
def test_lengths_flow_on_the_device_through_five_stages(ctx, dev):
    """four rendered rows at 48 kHz: rendered, limited, resampled to 16 kHz, band-passed and measured, every stage reading
    the lengths the stage before it wrote on the device; after the one wait every stage's output is the model's of the
    downloaded output of the stage before"""
    rate_in, rate_out, n, K = 48000, 16000, 4, 255
    c, ell = np.float32(0.25), 6
    num, U, D, _ = _table((rate_in, rate_out))
    h = G.fir_design(rate_out, 300.0, 3400.0, K)
    ctx.set_voices(W.single_voice(sample_rate=rate_in))
    segs, offs, vids, seeds = W.make_batch(n, sample_rate=rate_in, length=0.125, blend_length=0.125)
    stride = (W.max_samples(length=0.125, sample_rate=rate_in) + 63) // 64 * 64
    rs_stride = (-(-stride * U // D) + 63) // 64 * 64
    fir_stride = (rs_stride + K + 63) // 64 * 64
    b = ctx.upload(segs, offs, vids, seeds)
    fir_set = ctx.fir_create([(h, K // 2)])
    try:
        d_rows, d_lim, d_rs, d_fir = (_canary(dev, n, s) for s in (stride, stride, rs_stride, fir_stride))
        d_len, d_rs_len, d_fir_len = (dev.alloc(n * 4) for _ in range(3))
        d_gain, d_limited, d_lim_bad, d_rs_bad, d_fir_bad, d_tp_bad, d_peak, d_lv_bad = (dev.alloc(n * 4) for _ in range(8))
        d_tp, d_sumsq = dev.alloc(n * 8), dev.alloc(n * 8)
        b.synthesize_async(d_rows, stride, d_len)
        ctx.limit_async(d_rows, stride, d_len, n, c, ell, d_lim, stride, 1, d_gain, d_limited, d_lim_bad)
        ctx.resample_async(d_lim, stride, d_len, n, rate_in, rate_out, d_rs, rs_stride, d_rs_len, d_rs_bad)
        ctx.fir_async(fir_set, d_rs, rs_stride, d_rs_len, n, None, d_fir, fir_stride, d_fir_len, d_fir_bad)
        ctx.true_peak_async(d_fir, fir_stride, d_fir_len, n, d_tp, d_tp_bad)
        ctx.levels_async(d_fir, fir_stride, d_fir_len, n, d_sumsq, d_peak, d_lv_bad)
        ctx.sync()
    finally:
        b.free()
        ctx.fir_free(fir_set)
    u32 = lambda p: dev.down(p, n, np.uint32)
    lens, rs_len, fir_len = u32(d_len), u32(d_rs_len), u32(d_fir_len)
    rows, lim = dev.down(d_rows, (n, stride), np.float32), dev.down(d_lim, (n, stride), np.float32)
    rs, fir = dev.down(d_rs, (n, rs_stride), np.float32), dev.down(d_fir, (n, fir_stride), np.float32)
    assert lens.min() > 20000
    # the limiter on the rendered rows
    rendered = [rows[i, :lens[i]] for i in range(n)]
    w_out, w_gain, w_limited, w_bad = limiter_model(rendered, c, ell)
    _rows_equal(lim, w_out, "limit")
    assert same_bits(dev.down(d_gain, n, np.float32), w_gain) and np.array_equal(u32(d_limited), w_limited)
    assert np.array_equal(u32(d_lim_bad), w_bad) and not w_bad.any()
    print(f"\nrendered peaks {[float(np.abs(x).max()) for x in rendered]}, limited samples {list(w_limited)} at c = {float(c)}")
    # the resampler on the limited rows, the band-pass on the resampled ones, the measurements on the filtered ones
    tp, sumsq, peak = dev.down(d_tp, n, np.float64), dev.down(d_sumsq, n, np.float64), dev.down(d_peak, n, np.float32)
    for i in range(n):
        y, n_out, bad = resample_model(lim[i, :lens[i]], num, D)
        assert rs_len[i] == n_out == -(-int(lens[i]) * U // D) and u32(d_rs_bad)[i] == bad == 0
        assert same_bits(rs[i, :n_out], y) and np.all(rs[i, n_out:] == CANARY), i
        z, n_fir, bad = fir_model(rs[i, :n_out], h, K // 2)
        assert fir_len[i] == n_fir == n_out + K // 2 and u32(d_fir_bad)[i] == bad == 0
        assert same_bits(fir[i, :n_fir], z) and np.all(fir[i, n_fir:] == CANARY), i
        w_tp, w_tp_bad = true_peak_model(fir[i, :n_fir])
        assert tp[i] == w_tp > 0 and u32(d_tp_bad)[i] == w_tp_bad == 0
        w_sumsq, w_peak, w_lv_bad = row_model(fir[i, :n_fir])
        assert sumsq[i] == w_sumsq > 0 and peak[i] == w_peak and u32(d_lv_bad)[i] == w_lv_bad == 0


# ---- e. recursive filters and dynamics ------------------------------------------------------------------------------------------
def _blocked(ctx, dev, iir_set, rows, tail):
    """a blocked call's buffers, all made here -> what _blocked_check needs once the queue has drained"""
    stride = (max(len(x) for x in rows) + 63) // 64 * 64
    out_stride = stride + (tail + 63) // 64 * 64
    d_rows, d_len = _up(dev, rows, stride)
    return (iir_set, d_rows, stride, d_len, len(rows), None, tail, _canary(dev, len(rows), out_stride), out_stride,
            dev.alloc(len(rows) * 4), dev.alloc(len(rows) * 4))


def _blocked_check(dev, call, rows, filters, what):
    _, _, _, _, n, _, tail, d_out, out_stride, d_out_len, d_bad = call
    want = iir_blocked_model(rows, filters, None, tail)
    _rows_equal(dev.down(d_out, (n, out_stride), np.float32), [w[0] for w in want], what)
    assert np.array_equal(dev.down(d_out_len, n, np.uint32), [w[1] for w in want]), what
    assert np.array_equal(dev.down(d_bad, n, np.uint32), [w[2] for w in want]), what


def test_a_sets_block_matrices_go_up_and_the_blocked_scratch_grows_with_work_queued(ctx, dev):
    """the context's first blocked call is a new set's first: its block matrices are made on the host and uploaded from there
    with nothing waited for.  Behind it a call on another set with longer rows and more of them, for which both the block
    states and the workgroups' counts grow with the first call still queued on them; then the first set again, on a small
    call.  All three are the model's bits."""
    rng = np.random.default_rng(51)
    first, second = [random_filter(2, rng, radius=0.999)], [random_filter(3, rng, radius=0.999)]
    small, large = [_noise(rng, n) for n in (1500, 0, 1025)], [_noise(rng, n) for n in (70000, 4097, 1, 66000)]
    a, b = ctx.iir_create(first), ctx.iir_create(second)
    try:
        calls = [_blocked(ctx, dev, a, small, 9), _blocked(ctx, dev, b, large, 40), _blocked(ctx, dev, a, small[::-1], 2000)]
        # (blocks of states and workgroups of counts: the second call needs more of both than the first left)
        grid = [-(-(c[2] + c[6]) // 1024) for c in calls]
        assert 4 * grid[1] * 2 * 4 > 3 * grid[0] * 2 * 2 and 4 * -(-grid[1] // 64) > 3 * -(-grid[0] // 64) and grid[2] < grid[1]
        for c in calls:
            ctx.iir_blocked_async(*c)
        ctx.sync()
    finally:
        ctx.iir_free(a)
        ctx.iir_free(b)
    _blocked_check(dev, calls[0], small, first, "the set's first blocked call")
    _blocked_check(dev, calls[1], large, second, "the larger call")
    _blocked_check(dev, calls[2], small[::-1], first, "the small call behind it")


def test_an_iir_set_and_a_curve_set_are_freed_with_work_queued_and_others_created(ctx, dev):
    """grail_iir_free and grail_dyn_free at once behind a call of the set's own (they wait for what is queued), a different set
    of the same shape created (which may get the freed one's memory) and used: each result is its own set's"""
    rng = np.random.default_rng(52)
    filters = [[random_filter(3, rng), random_filter(1, rng)] for _ in range(2)]
    comp = [G.dyn_design(G.DYN_COMPRESS, G.DYN_PEAK, t, 4.0, 6.0, 0.0, 0.0) for t in (-30.0, -12.0)]
    curves = [[(comp[k], G.dyn_ballistics(48000, 1.0, 50.0 + 100.0 * k), G.DYN_PEAK), (np.arange(M.POINTS, dtype=np.float64) + k, (0.25, 0.875), G.DYN_SQUARE)]
              for k in range(2)]
    rows = [_noise(rng, n) for n in (700, 129, 0, 1000)]
    which = [0, 1, 1, 0]
    stride, out_stride, tail = 1024, 1088, 40
    d_rows, d_len = _up(dev, rows, stride)
    d_which = dev.up(np.array(which, np.uint32))
    iir_res = [(_canary(dev, 4, out_stride), dev.alloc(16), dev.alloc(16)) for _ in range(2)]
    dyn_res = [(_canary(dev, 4, out_stride), dev.alloc(16), dev.alloc(16), dev.alloc(32)) for _ in range(2)]
    a = ctx.iir_create(filters[0])
    ctx.iir_async(a, d_rows, stride, d_len, 4, d_which, tail, iir_res[0][0], out_stride, iir_res[0][1], iir_res[0][2])
    ctx.iir_free(a)
    b = ctx.iir_create(filters[1])
    ctx.iir_async(b, d_rows, stride, d_len, 4, d_which, tail, iir_res[1][0], out_stride, iir_res[1][1], iir_res[1][2])
    c = ctx.dyn_create(curves[0])
    ctx.dyn_async(c, d_rows, stride, d_len, 4, d_which, dyn_res[0][0], out_stride, *dyn_res[0][1:])
    ctx.dyn_free(c)
    d = ctx.dyn_create(curves[1])
    ctx.dyn_async(d, d_rows, stride, d_len, 4, d_which, dyn_res[1][0], out_stride, *dyn_res[1][1:])
    ctx.sync()
    ctx.iir_free(b)
    ctx.dyn_free(d)
    outs = []
    for k in range(2):
        want = iir_model(rows, filters[k], which, tail)
        out = dev.down(iir_res[k][0], (4, out_stride), np.float32)
        _rows_equal(out, [w[0] for w in want], ("iir", k))
        assert np.array_equal(dev.down(iir_res[k][1], 4, np.uint32), [w[1] for w in want])
        assert np.array_equal(dev.down(iir_res[k][2], 4, np.uint32), [w[2] for w in want])
        outs.append(out)
        want = M.dyn_model(rows, curves[k], which)
        out = dev.down(dyn_res[k][0], (4, out_stride), np.float32)
        _rows_equal(out, [w[0] for w in want], ("dyn", k))
        assert np.array_equal(dev.down(dyn_res[k][1], 4, np.uint32), [w[1] for w in want])
        assert np.array_equal(dev.down(dyn_res[k][2], 4, np.uint32), [w[2] for w in want])
        assert same_bits(dev.down(dyn_res[k][3], 4, np.float64), np.array([w[3] for w in want], np.float64))
        outs.append(out)
    assert not np.array_equal(outs[0].view(np.uint32), outs[2].view(np.uint32))
    assert not np.array_equal(outs[1].view(np.uint32), outs[3].view(np.uint32))


def test_the_rows_of_a_stream_follow_the_indices_given_at_its_opening(ctx, dev):
    """an IIR stream and a dynamics stream opened with the caller's filter, curve and key_row arrays, which are written over the
    moment the open returns, and the streams fed at once: every row runs through what its index said at the opening"""
    rng = np.random.default_rng(53)
    n_rows, n, stride = 70, 150, 192
    filters = [random_filter(S, rng) for S in (1, 2, 3)]
    curves = three_curves()
    rows = [_noise(rng, n) for _ in range(n_rows)]
    keys = [_noise(rng, n) for _ in range(n_rows)]
    which = rng.integers(0, 3, n_rows).astype(np.uint32)
    key_row = rng.permutation(n_rows).astype(np.uint32)
    given = (which.copy(), which.copy(), key_row.copy())
    d_rows, d_len = _up(dev, rows, stride)
    d_keys, _ = _up(dev, keys, stride)
    d_iir, d_dyn = _canary(dev, n_rows, stride), _canary(dev, n_rows, stride)
    res = [dev.alloc(n_rows * 4) for _ in range(4)] + [dev.alloc(n_rows * 8)]
    iir_set, dyn_set = ctx.iir_create(filters), ctx.dyn_create(curves)
    streams = []
    try:
        streams.append(("iir", ctx.iir_stream_open(iir_set, n_rows, given[0], 0)))
        given[0][:] = (given[0] + 1) % 3
        streams.append(("dyn", ctx.dyn_stream_open(dyn_set, n_rows, given[1], n_rows, given[2])))
        given[1][:] = (given[1] + 1) % 3
        given[2][:] = given[2][::-1].copy()
        ctx.iir_stream_next_async(streams[0][1], d_rows, stride, d_len, d_iir, stride, res[0], res[1])
        ctx.dyn_stream_next_async(streams[1][1], d_rows, stride, d_len, d_dyn, stride, res[2], res[3], res[4], key_dev=d_keys, key_stride=stride)
        ctx.sync()
    finally:
        for kind, st in streams:
            (ctx.iir_stream_close if kind == "iir" else ctx.dyn_stream_close)(st)
        ctx.iir_free(iir_set)
        ctx.dyn_free(dyn_set)
    assert not np.array_equal(given[0], which) and not np.array_equal(given[2], key_row)
    want = iir_model(rows, filters, which.tolist())
    _rows_equal(dev.down(d_iir, (n_rows, stride), np.float32), [w[0] for w in want], "iir stream")
    assert np.array_equal(dev.down(res[0], n_rows, np.uint32), [n] * n_rows)
    assert np.array_equal(dev.down(res[1], n_rows, np.uint32), [w[2] for w in want])
    want = M.dyn_model(rows, curves, which.tolist(), keys=keys, key_row=key_row.tolist())
    _rows_equal(dev.down(d_dyn, (n_rows, stride), np.float32), [w[0] for w in want], "dyn stream")
    assert np.array_equal(dev.down(res[3], n_rows, np.uint32), [w[2] for w in want])
    assert same_bits(dev.down(res[4], n_rows, np.float64), np.array([w[3] for w in want], np.float64))


def test_lengths_flow_on_the_device_through_a_recursive_filter_and_a_compressor(ctx, dev):
    """rows band-passed, equalised and compressed, twice (once a lane a row, once a workgroup a row): the recursive filter reads
    the lengths the band-pass wrote on the device and writes its own, with the tail, for both dynamics calls to read; the
    host sees none of them before the one wait"""
    rng = np.random.default_rng(54)
    K, origin, tail, n = 33, 16, 75, 5
    h = rng.uniform(-1.0, 1.0, K).astype(np.float32)
    filters, curves = [random_filter(3, rng)], three_curves()
    rows = [_noise(rng, k) for k in (1200, 64, 0, 777, 1)]
    stride, fir_stride, iir_stride = 1216, 1280, 1344
    d_rows, d_len = _up(dev, rows, stride)
    d_fir, d_iir, d_dyn, d_track = (_canary(dev, n, s) for s in (fir_stride, iir_stride, iir_stride, iir_stride))
    d_fir_len, d_iir_len, d_dyn_len, d_track_len = (dev.alloc(n * 4) for _ in range(4))
    d_bad = [dev.alloc(n * 4) for _ in range(4)]
    d_gain = [dev.alloc(n * 8) for _ in range(2)]
    fir_set, iir_set, dyn_set = ctx.fir_create([(h, origin)]), ctx.iir_create(filters), ctx.dyn_create(curves)
    try:
        ctx.fir_async(fir_set, d_rows, stride, d_len, n, None, d_fir, fir_stride, d_fir_len, d_bad[0])
        ctx.iir_async(iir_set, d_fir, fir_stride, d_fir_len, n, None, tail, d_iir, iir_stride, d_iir_len, d_bad[1])
        ctx.dyn_async(dyn_set, d_iir, iir_stride, d_iir_len, n, None, d_dyn, iir_stride, d_dyn_len, d_bad[2], d_gain[0])
        ctx.track_dyn_async(dyn_set, d_iir, iir_stride, d_iir_len, n, None, d_track, iir_stride, d_track_len, d_bad[3], d_gain[1])
        ctx.sync()
    finally:
        ctx.fir_free(fir_set)
        ctx.iir_free(iir_set)
        ctx.dyn_free(dyn_set)
    u32 = lambda p: dev.down(p, n, np.uint32)
    fir, iir = dev.down(d_fir, (n, fir_stride), np.float32), dev.down(d_iir, (n, iir_stride), np.float32)
    fir_len, iir_len = u32(d_fir_len), u32(d_iir_len)
    want = [fir_model(x, h, origin) for x in rows]
    _rows_equal(fir, [w[0] for w in want], "fir")
    assert np.array_equal(fir_len, [w[1] for w in want]) and np.array_equal(u32(d_bad[0]), [w[2] for w in want])
    assert fir_len.max() > 1200 and 0 in fir_len
    filtered = [fir[i, :fir_len[i]] for i in range(n)]
    want = iir_model(filtered, filters, None, tail)
    _rows_equal(iir, [w[0] for w in want], "iir")
    assert np.array_equal(iir_len, [w[1] for w in want]) and np.array_equal(u32(d_bad[1]), [0] * n)
    assert iir_len.tolist() == [k + tail if k else 0 for k in fir_len]
    equalised = [iir[i, :iir_len[i]] for i in range(n)]
    want = M.dyn_model(equalised, curves)
    for d_out, d_out_len, d_b, d_g, what in ((d_dyn, d_dyn_len, d_bad[2], d_gain[0], "dyn"), (d_track, d_track_len, d_bad[3], d_gain[1], "track dyn")):
        _rows_equal(dev.down(d_out, (n, iir_stride), np.float32), [w[0] for w in want], what)
        assert np.array_equal(u32(d_out_len), iir_len) and np.array_equal(u32(d_b), [0] * n), what
        assert same_bits(dev.down(d_g, n, np.float64), np.array([w[3] for w in want], np.float64)), what
