"""FIR filtering on the device (grail_fir_async) against the numpy model of tests/fir_model.py, bit for bit in the filtered
samples, the lengths and the non-finite counts: filters shorter than, equal to and longer than a block of eight taps, every
origin, rows that end at, before and after a seam of the kernel's chunks, impulses, -0.0 and denormals in samples and
taps, non-finite samples at the rows' ends and at the seams, content whose sums cancel (so that the order of the fold
shows); rows on different filters of one set, an index outside the set; every layout the same bits; nothing written past
a row's outputs; an output cut short by out_stride; sets created, freed and used in turn; rendered speech through a
telephone band."""
import ctypes as C
import os
import re
import subprocess
import wave

import numpy as np
import pytest

import grail_hip as G
from grail_hip import workload as W
from fir_model import cancelling_taps, fir_model, steps
from test_levels_gpu import CANARY, Dev, dev  # noqa: F401  (dev is a fixture)
from test_loudness_host import lufs_model
from test_true_peak_host import db

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = G.FIR_CHUNK
BLOCK = 8                                       # the taps of one step of the kernel's loop, which takes the blocks in pairs
TAPS = [1, 2, 7, 8, 9, 17, 24, 33, 40, 64, 255]   # 17, 24 and 33, 40: the first and the last tap count of 3 and of 5 blocks
REFUSED = 0xFFFFFFFF


def blocks(K):
    """the blocks of eight taps that the kernel walks for K taps"""
    return -(-K // BLOCK)


def origins(K):
    return sorted({0, (K - 1) // 2, K - 1})


def lengths(K):
    """the issue's row lengths, negative ones dropped"""
    return sorted({n for n in (0, 1, 2, K - 1, K, K + 1, CHUNK - K, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 17) if n >= 0})


def random_taps(K, rng):
    """uniform in +-1, some -0.0, some denormal"""
    h = rng.uniform(-1.0, 1.0, K).astype(np.float32)
    h[rng.random(K) < 0.15] = np.float32(-0.0)
    tiny = rng.random(K) < 0.15
    h[tiny] = (rng.integers(1, 1 << 23, int(tiny.sum())).astype(np.uint32) | (rng.integers(0, 2, int(tiny.sum())).astype(np.uint32) << 31)).view(np.float32)
    return h


def seams(n):
    """the input times either side of every chunk seam inside a row of n samples"""
    at = set()
    for c in range(1, n // CHUNK + 2):
        at |= {c * CHUNK - 2, c * CHUNK - 1, c * CHUNK, c * CHUNK + 1}
    return sorted(t for t in at if 0 <= t < n)


def contents(n, rng):
    """noise; impulses at the row's ends; noise with -0.0 and denormals; noise with NaN / +-Inf at the row's ends and either
    side of every seam"""
    noise = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    impulses = np.zeros(n, np.float32)
    small = noise.copy()
    small[rng.random(n) < 0.2] = np.float32(-0.0)
    tiny = rng.random(n) < 0.2
    small[tiny] = (rng.integers(1, 1 << 23, int(tiny.sum())).astype(np.uint32) | (rng.integers(0, 2, int(tiny.sum())).astype(np.uint32) << 31)).view(np.float32)
    holes = noise.copy()
    if n:
        impulses[0] = 1.0
        impulses[n - 1] = -1.0
        for i, t in enumerate([0, n - 1] + seams(n)):
            holes[t] = (np.nan, np.inf, -np.inf)[i % 3]
    return [noise, impulses, small, holes]


def run(ctx, dev, fir_set, rows, which=None, tail=0, stride=None, out_stride=None, in_offset=0, out_offset=0, guard=64, lens=None,
        fill=np.nan):
    """rows[i] as row i of a buffer that holds `fill` (NaN) everywhere else, filtered with filter which[i] of the set (None:
    filter_dev NULL) into a buffer that holds CANARY, with `guard` floats of it before and after -> (out [n_rows, out_stride]
    as it lies on the device afterwards, out_len, nonfinite).  tail: the longest n_taps - 1 - origin, for the default
    out_stride."""
    longest = max([len(x) for x in rows] + [1])
    stride = stride or (longest + 63) // 64 * 64
    out_stride = (longest + tail + 63) // 64 * 64 if out_stride is None else out_stride
    host = np.full(len(rows) * stride + in_offset, fill, np.float32)
    for i, x in enumerate(rows):
        host[in_offset + i * stride:in_offset + i * stride + len(x)] = x
    d_in = dev.up(host)
    before = guard + out_offset
    d_out = dev.up(np.full(before + len(rows) * out_stride + guard, CANARY, np.float32))
    d_len = dev.up(np.array([len(x) for x in rows] if lens is None else lens, np.uint32))
    d_which = None if which is None else dev.up(np.array(which, np.uint32))
    out_len, bad = ctx.fir(fir_set, C.c_void_p(d_in.value + in_offset * 4), stride, d_len, len(rows), d_which,
                           C.c_void_p(d_out.value + before * 4), out_stride)
    out = dev.down(d_out, before + len(rows) * out_stride + guard, np.float32)
    assert np.all(out[:before] == CANARY) and np.all(out[before + len(rows) * out_stride:] == CANARY), "written outside out"
    return out[before:before + len(rows) * out_stride].reshape(len(rows), out_stride), out_len, bad


def same(rows, filters, which, got, what, out_stride=None):
    """the device's (out, out_len, nonfinite) against the model's; out rows hold the canary past their outputs; a row whose
    index is outside the set holds nothing else"""
    out, out_len, bad = got
    for i, x in enumerate(rows):
        f = 0 if which is None else which[i]
        if f >= len(filters):
            assert (out_len[i], bad[i]) == (REFUSED, 0) and np.all(out[i] == CANARY), (what, i, "a refused row")
            continue
        h, o = filters[f]
        y, n_out, w_bad = fir_model(x, h, o, out_stride=out.shape[1] if out_stride is None else out_stride)
        assert (out_len[i], bad[i]) == (n_out, w_bad), (what, i, len(x), len(h), o, out_len[i], n_out, bad[i], w_bad)
        assert np.all(out[i, n_out:] == CANARY), (what, i, len(x), "written past the row's outputs")
        differ = np.flatnonzero(out[i, :n_out].view(np.uint32) != y.view(np.uint32))
        assert len(differ) == 0, (what, i, len(x), len(h), o, n_out, differ[:8], out[i, differ[:4]], y[differ[:4]])


def filters_of(K, rng):
    """the filters of one tap count: random taps at every origin, the cancelling taps at the middle origin, and (K odd, >= 3)
    the designed band-pass at its own"""
    fs = [(random_taps(K, rng), o) for o in origins(K)]
    if K >= 2:
        fs.append((cancelling_taps(K, rng), (K - 1) // 2))
    if K % 2 == 1 and K >= 3:
        fs.append((G.fir_design(8000, 300.0, 3400.0, K), (K - 1) // 2))
    return fs


# ---- 1. bit parity with the model ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", TAPS)
def test_bit_parity_with_the_model(gpu_ctx, dev, K):
    """one call per tap count: a set of its filters, rows of the issue's lengths in the four kinds of content on every filter
    but the cancelling one, which gets the steps"""
    # an odd count of blocks above one (the pair loop runs, then the tail with the windows swapped) is among the cases
    assert [blocks(k) for k in (17, 24, 33, 40)] == [3, 3, 5, 5] and {17, 24, 33, 40} <= set(TAPS)
    rng = np.random.default_rng(100 + K)
    filters = filters_of(K, rng)
    rows, which = [], []
    for f, (h, _) in enumerate(filters):
        cancelling = K >= 2 and f == len(origins(K))
        for n in lengths(K):
            for x in ([steps(n, rng)] if cancelling else contents(n, rng)):
                rows.append(x)
                which.append(f)
    assert sum(int(np.count_nonzero(~np.isfinite(x))) for x in rows) > 20
    fir_set = gpu_ctx.fir_create(filters)
    try:
        got = run(gpu_ctx, dev, fir_set, rows, which, tail=K - 1)
    finally:
        gpu_ctx.fir_free(fir_set)
    same(rows, filters, which, got, K)


@pytest.mark.parametrize("origin", [0, 2047])
def test_the_longest_filter(gpu_ctx, dev, origin):
    """K = 4096 over three rows: a stretch of 6143 samples, 512 blocks of taps"""
    rng = np.random.default_rng(4096 + origin)
    filters = [(random_taps(4096, rng), origin)]
    rows = [contents(n, rng)[3] for n in (1, CHUNK + 1, 2 * CHUNK + 17)]
    fir_set = gpu_ctx.fir_create(filters)
    try:
        got = run(gpu_ctx, dev, fir_set, rows, None, tail=4095 - origin)
    finally:
        gpu_ctx.fir_free(fir_set)
    same(rows, filters, None, got, ("4096", origin))


# ---- 2. filter sets -----------------------------------------------------------------------------------------------------
def test_rows_on_different_filters_of_one_set_and_an_index_outside_it(gpu_ctx, dev):
    """filter_dev given: neighbours on different filters (different tap counts and origins), one row with index = F, which is
    refused (0xFFFFFFFF, 0, canary throughout) while its neighbours are right; filter_dev NULL = all zeros"""
    rng = np.random.default_rng(21)
    filters = [(random_taps(9, rng), 4), (random_taps(64, rng), 0), (random_taps(1, rng), 0), (random_taps(255, rng), 254)]
    rows = [contents(n, rng)[3] for n in (CHUNK + 1, 700, CHUNK + 1, 2 * CHUNK + 17, 5, CHUNK - 1)]
    which = [1, 0, len(filters), 3, 2, 1]
    fir_set = gpu_ctx.fir_create(filters)
    try:
        got = run(gpu_ctx, dev, fir_set, rows, which, tail=254)
        same(rows, filters, which, got, "mixed")
        assert got[1][2] == REFUSED and got[2][2] == 0
        far = run(gpu_ctx, dev, fir_set, rows[:2], [0xFFFFFFFF, 64], tail=254)
        same(rows[:2], filters, [0xFFFFFFFF, 64], far, "far outside")
        null = run(gpu_ctx, dev, fir_set, rows, None, tail=254)
        zeros = run(gpu_ctx, dev, fir_set, rows, [0] * len(rows), tail=254)
        same(rows, filters, None, null, "NULL")
        assert all(np.array_equal(p.view(np.uint32), q.view(np.uint32)) for p, q in zip(null, zeros))
    finally:
        gpu_ctx.fir_free(fir_set)


def test_a_filter_of_three_blocks_between_one_of_two_and_one_of_five(gpu_ctx, dev):
    """K = 20 between K = 9 and K = 33 in one set: neighbouring workgroups leave the pair loop after 1, 1 and 2 turns, two of
    them into the tail for the odd block; rows of CHUNK + 1 and 2 CHUNK + 17 samples on each, in every content"""
    rng = np.random.default_rng(23)
    Ks = (9, 20, 33)
    assert [blocks(K) for K in Ks] == [2, 3, 5] and all(blocks(K) % 2 == 1 and blocks(K) >= 3 for K in Ks[1:])
    filters = [(random_taps(9, rng), 4), (random_taps(20, rng), 0), (random_taps(33, rng), 32), (cancelling_taps(20, rng), 9),
               (random_taps(20, rng), 19)]
    rows, which = [], []
    for n in (CHUNK + 1, 2 * CHUNK + 17):
        for f in (0, 1, 2, 4):
            for x in contents(n, rng):
                rows.append(x)
                which.append(f)
        rows.append(steps(n, rng))
        which.append(3)
    fir_set = gpu_ctx.fir_create(filters)
    try:
        got = run(gpu_ctx, dev, fir_set, rows, which, tail=32)
    finally:
        gpu_ctx.fir_free(fir_set)
    same(rows, filters, which, got, "2, 3 and 5 blocks")


# ---- 3. layout independence ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [7, 20, 64, 255])
def test_every_layout_gives_the_same_bits(gpu_ctx, dev, K):
    """aligned bases and strides that are multiples of 4; bases one float off; odd strides; an out_stride above what the rows
    need.  K = 20: three blocks, so the tail for an odd block runs after the pair loop in the 4-byte variant too"""
    assert blocks(20) % 2 == 1 and blocks(20) >= 3
    rng = np.random.default_rng(7 + K)
    filters = [(random_taps(K, rng), o) for o in origins(K)]
    ns = [K - 1, CHUNK - K, CHUNK, CHUNK + 1, 2 * CHUNK + 17, 3]
    rows = [contents(n, rng)[3] for n in ns]
    which = [i % len(filters) for i in range(len(rows))]
    longest = max(ns)
    fir_set = gpu_ctx.fir_create(filters)
    try:
        a = run(gpu_ctx, dev, fir_set, rows, which, tail=K - 1)
        same(rows, filters, which, a, (K, "aligned"))
        b = run(gpu_ctx, dev, fir_set, rows, which, tail=K - 1, in_offset=1, out_offset=1)
        c = run(gpu_ctx, dev, fir_set, rows, which, stride=longest + 3 - longest % 2, out_stride=(longest + K + 130) | 1)
        d = run(gpu_ctx, dev, fir_set, rows, which, out_stride=longest + K + 1024)
    finally:
        gpu_ctx.fir_free(fir_set)
    for other, what in ((b, "offset"), (c, "odd strides"), (d, "wide")):
        same(rows, filters, which, other, (K, what))
        assert np.array_equal(other[1], a[1]) and np.array_equal(other[2], a[2])
        for i, n_out in enumerate(a[1]):
            assert np.array_equal(other[0][i, :n_out].view(np.uint32), a[0][i, :n_out].view(np.uint32)), (K, what, i)


# ---- 4. the clamp and the footprint ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,origin", [(64, 0), (255, 127), (9, 8)])
def test_an_out_stride_below_the_rows_length_gives_the_prefix(gpu_ctx, dev, K, origin):
    """out_stride cutting the tail at CHUNK - 1, at CHUNK, and at 5 (below n), and 0: out_len = out_stride, the samples the
    prefix of the unclamped result; the non-finite count is that of the whole row, also of the samples whose outputs were
    cut"""
    rng = np.random.default_rng(13 + K)
    filters = [(random_taps(K, rng), origin)]
    rows = [contents(2 * CHUNK + 17, rng)[3], contents(CHUNK - (K - 1 - origin), rng)[0], contents(CHUNK - 1, rng)[3]]
    rows[0][-5] = np.nan
    fir_set = gpu_ctx.fir_create(filters)
    try:
        full = run(gpu_ctx, dev, fir_set, rows, None, tail=K - 1)
        same(rows, filters, None, full, (K, "full"))
        for out_stride in (CHUNK, CHUNK - 1, 5, 0):
            cut = run(gpu_ctx, dev, fir_set, rows, None, out_stride=out_stride)
            same(rows, filters, None, cut, (K, out_stride), out_stride=out_stride)
            assert np.array_equal(cut[2], full[2]) and cut[1][0] == out_stride
            for i in range(len(rows)):
                k = cut[1][i]
                assert k == min(full[1][i], out_stride)
                assert np.array_equal(cut[0][i, :k].view(np.uint32), full[0][i, :k].view(np.uint32))
    finally:
        gpu_ctx.fir_free(fir_set)


def test_nothing_is_written_outside_the_rows_outputs_and_nothing_read_past_their_samples(gpu_ctx, dev):
    """run() keeps guards of the canary around out and NaN between a row's samples and its stride (here also +Inf and
    ordinary numbers: garbage), same() looks at every sample past out_len; len above the stride (the stride bounds the row),
    rows of no samples, no rows"""
    rng = np.random.default_rng(11)
    filters = [(random_taps(64, rng), 31)]
    stride = CHUNK + 64
    rows = [rng.uniform(-1, 1, n).astype(np.float32) for n in (stride, 0, stride, 5, stride)]
    fir_set = gpu_ctx.fir_create(filters)
    try:
        for fill in (np.nan, np.inf, 3.0):
            got = run(gpu_ctx, dev, fir_set, rows, None, stride=stride, out_stride=stride + 64, guard=4096,
                      lens=[0xFFFFFFFF, 0, stride, 5, 2 ** 31], fill=fill)
            same(rows, filters, None, got, ("len above the stride", fill))
            assert list(got[1]) == [stride + 32, 0, stride + 32, 37, stride + 32] and not got[2].any()
        d_len = dev.up(np.zeros(3, np.uint32))
        out_len, bad = gpu_ctx.fir(fir_set, None, 0, d_len, 3, None, None, 0)          # no samples at all: NULL rows are fine
        assert not out_len.any() and not bad.any()
        gpu_ctx.fir_async(fir_set, None, 64, None, 0, None, None, 64)                   # no rows: nothing queued
    finally:
        gpu_ctx.fir_free(fir_set)


# ---- 5. sets, scratch, refusals ---------------------------------------------------------------------------------------------
def test_sets_side_by_side_freed_and_created_and_the_scratch_grown(built):
    """a context of its own: two sets alive at once; one freed and another created, the first's results unchanged; a call,
    a larger call (the scratch grows), the first again: the same bits; a set that is left alive goes with the context"""
    rng = np.random.default_rng(17)
    with G.Context(0) as ctx:
        d = Dev(ctx)
        try:
            fa, fb, fc = [(random_taps(64, rng), 10)], [(random_taps(9, rng), 0), (random_taps(255, rng), 127)], [(random_taps(8, rng), 7)]
            rows = [contents(n, rng)[3] for n in (700, CHUNK + 5)]
            sa, sb = ctx.fir_create(fa), ctx.fir_create(fb)
            a = run(ctx, d, sa, rows, None, tail=63)
            same(rows, fa, None, a, "a")
            b = run(ctx, d, sb, rows, [1, 0], tail=254)
            same(rows, fb, [1, 0], b, "b")
            ctx.fir_free(sb)
            lib = G.load()
            assert lib.grail_fir_free(ctx.handle, sb) == G.ERR_INVALID_ARG            # freed: looked up, not looked into
            sc = ctx.fir_create(fc)
            same(rows, fc, None, run(ctx, d, sc, rows, None, tail=7), "c")
            longer = rows + [contents(5 * CHUNK + 1, rng)[3] for _ in range(6)]
            same(longer, fa, None, run(ctx, d, sa, longer, None, tail=63), "more scratch")
            again = run(ctx, d, sa, rows, None, tail=63)
            assert all(np.array_equal(p.view(np.uint32), q.view(np.uint32)) for p, q in zip(a, again))
            ctx.fir_free(None)
            ctx.fir_free(sc)
        finally:
            d.free()


def test_refusals_that_need_a_set_queue_nothing(gpu_ctx, dev):
    """out overlapping rows, a set of another context, strides that allow 2^32 outputs, more than 2^31 chunks: INVALID_ARG
    and the buffers untouched"""
    lib = G.load()
    rng = np.random.default_rng(19)
    fir_set = gpu_ctx.fir_create([(random_taps(9, rng), 0)])
    try:
        buf = np.full(4 * 256, CANARY, np.float32)
        d_buf, d_len = dev.up(buf), dev.up(np.full(2, 256, np.uint32))
        d_res = dev.up(np.full(4, 77, np.uint32))
        res = (d_res, C.c_void_p(d_res.value + 8))
        for out_at, out_stride in ((256, 256), (511, 256), (0, 256), (128, 64)):
            rc = lib.grail_fir_async(gpu_ctx.handle, fir_set, d_buf, 256, d_len, 2, None, C.c_void_p(d_buf.value + out_at * 4), out_stride,
                                     *res)
            assert rc == G.ERR_INVALID_ARG and b"overlaps" in lib.grail_last_error(), out_at
        a, b = 0x10000000, 2 ** 50
        assert lib.grail_fir_async(gpu_ctx.handle, fir_set, a, 2 ** 33, d_len, 1, None, b, 2 ** 34, *res) == G.ERR_INVALID_ARG
        assert b"2^32" in lib.grail_last_error()
        assert lib.grail_fir_async(gpu_ctx.handle, fir_set, a, 2 ** 32 - 1, d_len, 1024, None, b, 2 ** 32 - 1, *res) == G.ERR_INVALID_ARG
        assert b"2^31 chunks" in lib.grail_last_error()
        with G.Context(0) as other:
            theirs = other.fir_create([(random_taps(3, rng), 1)])
            for ctx, s in ((gpu_ctx, theirs), (other, fir_set)):
                rc = lib.grail_fir_async(ctx.handle, s, d_buf, 256, d_len, 1, None, C.c_void_p(d_buf.value + 2048), 256, *res)
                assert rc == G.ERR_INVALID_ARG and b"not a filter set of this context" in lib.grail_last_error()
            assert lib.grail_fir_free(gpu_ctx.handle, theirs) == G.ERR_INVALID_ARG
        gpu_ctx.sync()
        assert np.all(dev.down(d_buf, 4 * 256, np.float32) == CANARY) and np.all(dev.down(d_res, 4, np.uint32) == 77)
    finally:
        gpu_ctx.fir_free(fir_set)


# ---- 6. the chain -----------------------------------------------------------------------------------------------------------
def test_rendered_speech_through_a_telephone_band(gpu_ctx, dev):
    """four rows of the generic voice, half a second each, through the 300 - 3 400 Hz band-pass (255 taps) at the voices'
    rate: the model's bits on the rendered samples.  Printed (-s) for DESIGN.md §4.14, not asserted: how far the gated
    loudness and the true peak moved."""
    rate, n, K = 48000, 4, 255
    h = G.fir_design(rate, 300.0, 3400.0, K)
    gpu_ctx.set_voices(W.single_voice(sample_rate=rate))
    segs, offs, vids, seeds = W.make_batch(n, sample_rate=rate, length=0.125, blend_length=0.125)
    stride = W.max_samples(length=0.125, sample_rate=rate)
    out_stride = (stride + K + 63) // 64 * 64
    b = gpu_ctx.upload(segs, offs, vids, seeds)
    fir_set = gpu_ctx.fir_create([(h, K // 2)])
    try:
        d_rows, d_len = dev.alloc(n * stride * 4), dev.alloc(n * 4)
        d_out = dev.up(np.full(n * out_stride, CANARY, np.float32))
        b.synthesize_async(d_rows, stride, d_len)
        d_out_len = dev.alloc(n * 4)
        gpu_ctx.fir_async(fir_set, d_rows, stride, d_len, n, None, d_out, out_stride, d_out_len, None)
        tp_out, _ = gpu_ctx.true_peak(d_out, out_stride, d_out_len, n)
        gated_out, _, _ = gpu_ctx.loudness(d_out, out_stride, d_out_len, n, rate)
        tp_in, _ = gpu_ctx.true_peak(d_rows, stride, d_len, n)
        gated_in, _, _ = gpu_ctx.loudness(d_rows, stride, d_len, n, rate)
    finally:
        b.free()
        gpu_ctx.fir_free(fir_set)
    lens = dev.down(d_len, n, np.uint32)
    rows = dev.down(d_rows, (n, stride), np.float32)
    out = dev.down(d_out, (n, out_stride), np.float32)
    out_len = dev.down(d_out_len, n, np.uint32)
    assert lens.min() > 20000
    for i in range(n):
        y, n_out, _ = fir_model(rows[i, :lens[i]], h, K // 2)
        assert out_len[i] == n_out == lens[i] + K // 2 and np.all(out[i, n_out:] == CANARY)
        assert np.array_equal(out[i, :n_out].view(np.uint32), y.view(np.uint32)), i
        assert gated_out[i] > 0 and tp_out[i] > 0
        print(f"\nrow {i}: {lens[i]} samples at {rate} Hz through 300 - 3400 Hz ({K} taps): true peak {db(tp_in[i]):+.4f} -> "
              f"{db(tp_out[i]):+.4f} dBTP ({db(tp_out[i] / tp_in[i]):+.4f} dB), loudness {lufs_model(gated_in[i]):+.4f} -> "
              f"{lufs_model(gated_out[i]):+.4f} LUFS ({lufs_model(gated_out[i]) - lufs_model(gated_in[i]):+.4f} LU)", end="")


# ---- the example -----------------------------------------------------------------------------------------------------------
def test_grail_dialogue_band_option(gpu_ctx, tmp_path):
    """--lufs -23 --ceiling -1 --limit --band 300 3400 --rate 8000 writes an 8 kHz WAV and says what it filtered; without
    --band the line is absent and the file differs"""
    exe = os.path.join(ROOT, "grail-rs_amd", "lib", "grail_dialogue")
    args = ["--lufs", "-23", "--ceiling", "-1", "--limit", "--rate", "8000", "--report", "hello there", "a fine day to you"]
    runs = {}
    for name, extra in (("plain", []), ("band", ["--band", "300", "3400"]), ("short", ["--band", "300", "3400", "--taps", "63"])):
        r = subprocess.run([exe, "-o", str(tmp_path / f"{name}.wav")] + extra + args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        with wave.open(str(tmp_path / f"{name}.wav"), "rb") as w:
            runs[name] = (r.stdout, w.getframerate(), w.getnframes(), w.getnchannels())
    assert runs["band"][1:] == runs["plain"][1:] and runs["band"][1] == 8000 and runs["band"][3] == 2
    m = re.search(r"Filtered 300 - 3400 Hz at 44100 Hz \((\d+) taps\)", runs["band"][0])
    assert m and m.group(1) == "255", runs["band"][0]
    assert "(63 taps)" in runs["short"][0] and "Filtered" not in runs["plain"][0]
    assert (tmp_path / "plain.wav").read_bytes() != (tmp_path / "band.wav").read_bytes()
    print("\n" + m.group(0))
