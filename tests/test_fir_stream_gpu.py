"""Filter streams on the device (grail_filter_stream_*) against the numpy model of tests/fir_stream_model.py, bit for bit in
the samples, the lengths and the non-finite counts of every call and of the tails: the calls' outputs end to end, then the
tail, are what grail_fir_async gives for the whole row, whatever the split.  Every output buffer holds a canary with guards
around it: nothing is written past out_len or outside the buffer."""
import ctypes as C

import numpy as np
import pytest

import grail_hip as G
from grail_hip import workload as W
from fir_model import cancelling_taps, fir_model
from fir_stream_model import splits, stream_model
from test_fir_gpu import CHUNK, REFUSED, origins, random_taps
from test_levels_gpu import CANARY, Dev, dev  # noqa: F401  (dev is a fixture)

pytestmark = pytest.mark.gpu


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def at(ptr, floats):
    return C.c_void_p(ptr.value + 4 * floats)


def noise(n, rng, holes=True):
    """uniform in +-1 with -0.0 and, holes: NaN / +-Inf at the ends and the middle"""
    x = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    x[rng.random(n) < 0.1] = np.float32(-0.0)
    if holes and n:
        for i, t in enumerate((0, n - 1, n // 2)):
            x[t] = (np.nan, np.inf, -np.inf)[i]
    return x


def feed(ctx, dev, fs, chunks, stride=None, out_stride=None, in_offset=0, out_offset=0, guard=64, fill=np.nan):
    """one `next` call: chunks[i] as row i of an input buffer that holds `fill` (NaN) everywhere else, the outputs into a buffer
    of the canary with `guard` floats of it before and after -> (out [n_rows, out_stride] as it lies on the device afterwards,
    out_len, nonfinite)"""
    n_rows = len(chunks)
    longest = max([len(c) for c in chunks] + [1])
    stride = stride or (longest + 63) // 64 * 64
    out_stride = stride if out_stride is None else out_stride
    host = np.full(n_rows * stride + in_offset, fill, np.float32)
    for i, c in enumerate(chunks):
        host[in_offset + i * stride:in_offset + i * stride + len(c)] = c
    d_in = dev.up(host)
    before = guard + out_offset
    d_out = dev.up(np.full(before + n_rows * out_stride + guard, CANARY, np.float32))
    d_len = dev.up(np.array([len(c) for c in chunks], np.uint32))
    out_len, bad = ctx.fir_stream_next(fs, n_rows, at(d_in, in_offset), stride, d_len, at(d_out, before), out_stride)
    out = dev.down(d_out, before + n_rows * out_stride + guard, np.float32)
    assert np.all(out[:before] == CANARY) and np.all(out[before + n_rows * out_stride:] == CANARY), "written outside out"
    return out[before:before + n_rows * out_stride].reshape(n_rows, out_stride), out_len, bad


def ring_out(ctx, dev, fs, n_rows, out_stride, which=None, out_offset=0, guard=64):
    """one `finish` call -> (out, out_len), as feed"""
    before = guard + out_offset
    d_out = dev.up(np.full(before + n_rows * out_stride + guard, CANARY, np.float32))
    out_len = ctx.fir_stream_finish(fs, n_rows, at(d_out, before), out_stride, which)
    out = dev.down(d_out, before + n_rows * out_stride + guard, np.float32)
    assert np.all(out[:before] == CANARY) and np.all(out[before + n_rows * out_stride:] == CANARY), "written outside out"
    return out[before:before + n_rows * out_stride].reshape(n_rows, out_stride), out_len


def same(out, out_len, want, what, bad=None, want_bad=None):
    """a call's rows against the model's: want[i] the samples row i writes, None: a refused row; past them the canary"""
    for i, y in enumerate(want):
        if y is None:
            assert out_len[i] == REFUSED and np.all(out[i] == CANARY) and (bad is None or bad[i] == 0), (what, i, "a refused row")
            continue
        assert out_len[i] == len(y), (what, i, out_len[i], len(y))
        assert np.all(out[i, len(y):] == CANARY), (what, i, "written past the row's outputs")
        differ = np.flatnonzero(bits(out[i, :len(y)]) != bits(y))
        assert len(differ) == 0, (what, i, len(y), differ[:8], out[i, differ[:4]], y[differ[:4]])
        if bad is not None:
            assert bad[i] == want_bad[i], (what, i, bad[i], want_bad[i])


def stream_rows(ctx, dev, fir_set, filters, rows, which, row_splits, tail_stride=None, **layout):
    """rows[i] on filter which[i], fed as row_splits[i] says (shorter splits pause at the end), then finished: every call and
    the tails against the model -> the rows' outputs end to end"""
    n_calls = max(len(s) for s in row_splits)
    assert n_calls <= 60
    row_splits = [list(s) + [0] * (n_calls - len(s)) for s in row_splits]
    models = [stream_model(x, *filters[f], s) for x, f, s in zip(rows, which, row_splits)]
    fs = ctx.fir_stream_open(fir_set, len(rows), which)
    try:
        fed = [0] * len(rows)
        joined = [[] for _ in rows]
        for c in range(n_calls):
            chunks = [x[a:a + s[c]] for x, a, s in zip(rows, fed, row_splits)]
            out, out_len, bad = feed(ctx, dev, fs, chunks, **layout)
            same(out, out_len, [m[0][c][0] for m in models], ("call", c), bad, [m[0][c][1] for m in models])
            for i in range(len(rows)):
                joined[i].append(out[i, :out_len[i]])
                fed[i] += row_splits[i][c]
        longest = max(len(h) for h, _ in filters) - 1
        out, out_len = ring_out(ctx, dev, fs, len(rows), (longest + 7) // 4 * 4 if tail_stride is None else tail_stride,
                                out_offset=layout.get("out_offset", 0))
        same(out, out_len, [m[1] for m in models], "tail")
        for i in range(len(rows)):
            joined[i].append(out[i, :out_len[i]])
    finally:
        ctx.fir_stream_close(fs)
    return [np.concatenate(j) for j in joined]


def whole_rows(joined, filters, rows, which):
    """... and they are the one-shot rows"""
    for i, (x, f) in enumerate(zip(rows, which)):
        y, n_out, _ = fir_model(x, *filters[f])
        assert len(joined[i]) == n_out and np.array_equal(bits(joined[i]), bits(y)), i


# ---- 1. every split gives the one-shot row -----------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 8, 9, 17, 40, 255])
def test_every_split_gives_the_one_shot_row(gpu_ctx, dev, K):
    """one stream per tap count: a row for every origin, total and split"""
    rng = np.random.default_rng(300 + K)
    filters = [(random_taps(K, rng), o) for o in origins(K)]
    rows, which, row_splits = [], [], []
    for f in range(len(filters)):
        for N in sorted({0, 1, K - 1, K, CHUNK + 1, 2 * CHUNK + 17}):
            for split in splits(N, K, CHUNK, rng):
                rows.append(noise(N, rng))
                which.append(f)
                row_splits.append(split)
    fir_set = gpu_ctx.fir_create(filters)
    try:
        joined = stream_rows(gpu_ctx, dev, fir_set, filters, rows, which, row_splits)
    finally:
        gpu_ctx.fir_free(fir_set)
    whole_rows(joined, filters, rows, which)


# ---- 2. one sample per call ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [9, 17])
def test_one_sample_per_call(gpu_ctx, dev, K):
    """N = 40: the start-up (N < origin, no output yet) and every position of the ring are crossed; the cancelling taps on
    steps show the order of the fold"""
    rng = np.random.default_rng(40 + K)
    filters = [(random_taps(K, rng), o) for o in origins(K)] + [(cancelling_taps(K, rng), (K - 1) // 2)]
    rows = [noise(40, rng) for _ in origins(K)] + [np.repeat(rng.uniform(-1, 1, 8).astype(np.float32), 5)]
    which = list(range(len(filters)))
    fir_set = gpu_ctx.fir_create(filters)
    try:
        joined = stream_rows(gpu_ctx, dev, fir_set, filters, rows, which, [[1] * 40] * len(rows))
    finally:
        gpu_ctx.fir_free(fir_set)
    whole_rows(joined, filters, rows, which)


# ---- 3. the ring wraps -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,capacity", [(8, 8), (9, 8), (10, 16)])
def test_the_ring_wraps(gpu_ctx, dev, K, capacity):
    """chunks of 5 to N = 100: the ring (K - 1 rounded up to a power of two) is written across its end many times, with chunks
    shorter than it"""
    cap = 1
    while cap < K - 1:
        cap *= 2
    assert cap == capacity
    rng = np.random.default_rng(60 + K)
    filters = [(random_taps(K, rng), o) for o in origins(K)]
    rows = [noise(100, rng) for _ in filters]
    which = list(range(len(filters)))
    fir_set = gpu_ctx.fir_create(filters)
    try:
        joined = stream_rows(gpu_ctx, dev, fir_set, filters, rows, which, [[5] * 20] * len(rows))
    finally:
        gpu_ctx.fir_free(fir_set)
    whole_rows(joined, filters, rows, which)


# ---- 4. rows side by side --------------------------------------------------------------------------------------------------------
def test_eight_rows_on_four_filters_with_ragged_calls(gpu_ctx, dev):
    """every call feeds the rows different lengths, some 0; the input rows hold NaN past their lengths (feed's fill); a row
    never sees its neighbour's history: filters of 9, 64, 1 and 255 taps side by side in a ring of 256 samples"""
    rng = np.random.default_rng(44)
    filters = [(random_taps(9, rng), 4), (random_taps(64, rng), 0), (random_taps(1, rng), 0), (random_taps(255, rng), 254)]
    which = [1, 0, 3, 2, 3, 1, 0, 3]
    row_splits = [[0 if rng.random() < 0.3 else int(rng.integers(1, 700)) for _ in range(12)] for _ in which]
    for c in range(12):                                                        # every call pauses a row and feeds its neighbour
        row_splits[c % 8][c], row_splits[(c + 1) % 8][c] = 0, 100 + c
    row_splits[4][:3] = [0, 0, 0]                                              # a row that starts late
    assert all(any(s[c] == 0 for s in row_splits) and any(s[c] > 0 for s in row_splits) for c in range(12))
    rows = [noise(sum(s), rng) for s in row_splits]
    fir_set = gpu_ctx.fir_create(filters)
    try:
        joined = stream_rows(gpu_ctx, dev, fir_set, filters, rows, which, row_splits)
    finally:
        gpu_ctx.fir_free(fir_set)
    whole_rows(joined, filters, rows, which)


# ---- 5. non-finite samples at the cuts ---------------------------------------------------------------------------------------------
def test_non_finite_samples_at_the_cuts_are_counted_once(gpu_ctx, dev):
    """NaN and +-Inf as the last sample of one call and the first of the next: counted in the call that fed them, and +0.0
    when the next call meets them in the ring"""
    rng = np.random.default_rng(55)
    filters = [(random_taps(9, rng), 4), (random_taps(17, rng), 0), (random_taps(2, rng), 1)]
    split = [50, 50, 1, 49]
    rows = []
    for _ in filters:
        x = noise(150, rng, holes=False)
        x[[49, 50, 99, 100, 101, 149]] = [np.nan, np.inf, -np.inf, np.nan, np.inf, np.nan]
        rows.append(x)
    which = [0, 1, 2]
    calls = stream_model(rows[0], *filters[0], split)[0]
    assert [b for _, b in calls] == [1, 2, 1, 2]
    fir_set = gpu_ctx.fir_create(filters)
    try:
        joined = stream_rows(gpu_ctx, dev, fir_set, filters, rows, which, [split] * 3)
    finally:
        gpu_ctx.fir_free(fir_set)
    whole_rows(joined, filters, rows, which)


# ---- 6. layout independence ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [20, 255])
def test_every_layout_gives_the_same_bits(gpu_ctx, dev, K):
    """aligned bases and strides that are multiples of 4 (16-byte loads and stores); bases one float off; strides that are
    no multiple of 4 (the 4-byte variant)"""
    rng = np.random.default_rng(70 + K)
    filters = [(random_taps(K, rng), o) for o in origins(K)]
    totals = [2 * CHUNK + 17, CHUNK + 1, 700]
    rows = [noise(n, rng) for n in totals]
    which = [0, 1, 2]
    row_splits = [[CHUNK + 1, 3, CHUNK + 13], [5, CHUNK - 4, 0], [1, 0, 699]]
    stride = CHUNK + 64
    fir_set = gpu_ctx.fir_create(filters)
    try:
        a = stream_rows(gpu_ctx, dev, fir_set, filters, rows, which, row_splits, stride=stride)
        b = stream_rows(gpu_ctx, dev, fir_set, filters, rows, which, row_splits, stride=stride, in_offset=1, out_offset=1)
        c = stream_rows(gpu_ctx, dev, fir_set, filters, rows, which, row_splits, stride=stride + 1, out_stride=stride + 7,
                        tail_stride=(K - 1) | 1)
        d = stream_rows(gpu_ctx, dev, fir_set, filters, rows, which, row_splits, stride=stride, out_stride=stride + 1024, tail_stride=K - 1)
    finally:
        gpu_ctx.fir_free(fir_set)
    whole_rows(a, filters, rows, which)
    for other in (b, c, d):
        assert all(np.array_equal(bits(p), bits(q)) for p, q in zip(a, other))


# ---- 7. finish -------------------------------------------------------------------------------------------------------------------
def test_finish_marks_rows_and_ended_rows_are_refused(gpu_ctx, dev):
    """finish with `which` marking half the rows; the rest carry on and finish later; an ended row that is fed is refused and
    nothing of it changes; an ended row fed nothing writes nothing; finish twice writes nothing the second time"""
    rng = np.random.default_rng(77)
    K, o, n_rows = 17, 8, 6
    filters = [(random_taps(K, rng), o)]
    rows = [noise(160, rng) for _ in range(n_rows)]
    early = [0, 2, 4]
    empty = np.zeros(0, np.float32)
    fir_set = gpu_ctx.fir_create(filters)
    fs = gpu_ctx.fir_stream_open(fir_set, n_rows)
    try:
        models = [stream_model(x[:100], *filters[0], [100]) if i in early else stream_model(x, *filters[0], [100, 60])
                  for i, x in enumerate(rows)]
        out, out_len, bad = feed(gpu_ctx, dev, fs, [x[:100] for x in rows])
        same(out, out_len, [m[0][0][0] for m in models], "first", bad, [m[0][0][1] for m in models])
        out, out_len = ring_out(gpu_ctx, dev, fs, n_rows, K - 1, which=[1, 0, 1, 0, 1, 0])
        same(out, out_len, [models[i][1] if i in early else empty for i in range(n_rows)], "half finished")
        # rows 0 and 4 have ended and are fed: refused; row 2 has ended and is fed nothing; the others carry on
        chunks = [rows[0][100:110], rows[1][100:], empty, rows[3][100:], rows[4][100:105], rows[5][100:]]
        out, out_len, bad = feed(gpu_ctx, dev, fs, chunks)
        want = [None, models[1][0][1][0], empty, models[3][0][1][0], None, models[5][0][1][0]]
        same(out, out_len, want, "second", bad, [0, models[1][0][1][1], 0, models[3][0][1][1], 0, models[5][0][1][1]])
        out, out_len = ring_out(gpu_ctx, dev, fs, n_rows, K - 1, which=[1, 0, 1, 0, 0, 0])      # ended before: nothing
        same(out, out_len, [empty] * n_rows, "ended rows finished again")
        out, out_len = ring_out(gpu_ctx, dev, fs, n_rows, K + 4)                                   # NULL: all that are left
        same(out, out_len, [empty if i in early else models[i][1] for i in range(n_rows)], "the rest")
        out, out_len = ring_out(gpu_ctx, dev, fs, n_rows, K - 1)
        same(out, out_len, [empty] * n_rows, "finish twice")
        out, out_len, bad = feed(gpu_ctx, dev, fs, [x[:7] for x in rows])
        same(out, out_len, [None] * n_rows, "all ended", bad)
    finally:
        gpu_ctx.fir_stream_close(fs)
        gpu_ctx.fir_free(fir_set)


def test_a_row_that_was_fed_nothing_finishes_with_nothing(gpu_ctx, dev):
    """N = 0 at finish: no tail; N below the origin: the tail is all the row ever writes"""
    rng = np.random.default_rng(78)
    filters = [(random_taps(40, rng), 39), (random_taps(40, rng), 0)]
    rows = [noise(0, rng), noise(3, rng), noise(0, rng), noise(3, rng)]
    which = [0, 0, 1, 1]
    fir_set = gpu_ctx.fir_create(filters)
    try:
        joined = stream_rows(gpu_ctx, dev, fir_set, filters, rows, which, [[0, 0], [1, 2], [0], [3]])
    finally:
        gpu_ctx.fir_free(fir_set)
    whole_rows(joined, filters, rows, which)
    assert [len(j) for j in joined] == [0, 3, 0, 42]


# ---- 8. queued calls ---------------------------------------------------------------------------------------------------------------
def test_calls_queued_with_their_input_overwritten_behind_them(gpu_ctx, dev):
    """three `next` calls with results left on the device, a grail_memset_d of the input buffer right behind each: the call
    kept its own copy of the samples the next one needs"""
    rng = np.random.default_rng(88)
    K, o, n_rows, n = 255, 127, 3, 480
    filters = [(random_taps(K, rng), o)]
    rows = [noise(3 * n, rng) for _ in range(n_rows)]
    models = [stream_model(x, *filters[0], [n] * 3) for x in rows]
    stride = 512
    fir_set = gpu_ctx.fir_create(filters)
    fs = gpu_ctx.fir_stream_open(fir_set, n_rows)
    try:
        d_len = dev.up(np.full(n_rows, n, np.uint32))
        d_ins, d_outs, d_res = [], [], []
        for c in range(3):
            host = np.full((n_rows, stride), np.nan, np.float32)
            for i, x in enumerate(rows):
                host[i, :n] = x[c * n:(c + 1) * n]
            d_ins.append(dev.up(host))
            d_outs.append(dev.up(np.full(n_rows * stride, CANARY, np.float32)))
            d_res.append((dev.alloc(n_rows * 4), dev.alloc(n_rows * 4)))
        for c in range(3):
            gpu_ctx.fir_stream_next_async(fs, d_ins[c], stride, d_len, d_outs[c], stride, *d_res[c])
            gpu_ctx.memset(d_ins[c], 0xFF, n_rows * stride * 4)                   # (NaN everywhere)
        gpu_ctx.sync()
        for c in range(3):
            out = dev.down(d_outs[c], (n_rows, stride), np.float32)
            out_len, bad = dev.down(d_res[c][0], n_rows, np.uint32), dev.down(d_res[c][1], n_rows, np.uint32)
            same(out, out_len, [m[0][c][0] for m in models], ("queued", c), bad, [m[0][c][1] for m in models])
    finally:
        gpu_ctx.fir_stream_close(fs)
        gpu_ctx.fir_free(fir_set)


def test_two_finishing_calls_with_marks_queued_back_to_back(gpu_ctx, dev):
    """two `finish` calls with marks, their results left on the device, and no wait between them: the second writes the
    stream's host copy of the marks anew, which the first's upload may not have read yet, so it waits for the event behind that
    upload.  The first unit's tail comes from the first call alone and the others' from the second; behind what the feeding
    call wrote they are the one-shot rows"""
    rng = np.random.default_rng(89)
    K, o, n_rows, n = 17, 8, 3, 40
    filters = [(random_taps(K, rng), o)]
    rows = [noise(n, rng) for _ in range(n_rows)]
    stride, guard, marks = K + 3, 64, ([1, 0, 0], [0, 1, 1])
    fir_set = gpu_ctx.fir_create(filters)
    fs = gpu_ctx.fir_stream_open(fir_set, n_rows)
    try:
        out, out_len, _ = feed(gpu_ctx, dev, fs, rows)
        joined = [[out[i, :out_len[i]]] for i in range(n_rows)]
        d_outs = [dev.up(np.full(guard + n_rows * stride + guard, CANARY, np.float32)) for _ in range(2)]
        d_lens = [dev.up(np.full(n_rows, 77, np.uint32)) for _ in range(2)]
        for d_out, d_len, which in zip(d_outs, d_lens, marks):
            gpu_ctx.fir_stream_finish(fs, n_rows, at(d_out, guard), stride, which, out_len_dev=d_len)
        gpu_ctx.sync()
        lens = [dev.down(p, n_rows, np.uint32) for p in d_lens]
        assert lens[0][0] > 0 and not lens[0][1:].any() and lens[1][0] == 0 and lens[1][1:].all(), lens
        for d_out, out_len in zip(d_outs, lens):
            flat = dev.down(d_out, guard + n_rows * stride + guard, np.float32)
            out = flat[guard:guard + n_rows * stride].reshape(n_rows, stride)
            assert np.all(flat[:guard] == CANARY) and np.all(flat[guard + n_rows * stride:] == CANARY), "written outside out"
            for i in range(n_rows):
                assert np.all(out[i, out_len[i]:] == CANARY), (i, "written past the row's tail")
                joined[i].append(out[i, :out_len[i]])
    finally:
        gpu_ctx.fir_stream_close(fs)
        gpu_ctx.fir_free(fir_set)
    whole_rows([np.concatenate(j) for j in joined], filters, rows, [0] * n_rows)


# ---- 9. streams and their set ------------------------------------------------------------------------------------------------------
def test_two_streams_on_one_set_and_the_set_outlives_them(built):
    """a context of its own: two streams interleaved keep their own histories; grail_fir_free is refused while either is
    open and succeeds after both are closed; a closed stream is refused, as is another context's"""
    rng = np.random.default_rng(99)
    lib = G.load()
    with G.Context(0) as ctx:
        d = Dev(ctx)
        try:
            filters = [(random_taps(33, rng), 16), (random_taps(9, rng), 0)]
            xa, xb = [noise(300, rng), noise(300, rng)], [noise(200, rng)]
            ma = [stream_model(x, *filters[f], [100, 200]) for x, f in zip(xa, (0, 1))]
            mb = [stream_model(xb[0], *filters[1], [150, 50])]
            fir_set = ctx.fir_create(filters)
            sa, sb = ctx.fir_stream_open(fir_set, 2, [0, 1]), ctx.fir_stream_open(fir_set, 1, [1])
            out, out_len, _ = feed(ctx, d, sa, [x[:100] for x in xa])
            same(out, out_len, [m[0][0][0] for m in ma], "a, first")
            out, out_len, _ = feed(ctx, d, sb, [xb[0][:150]])
            same(out, out_len, [mb[0][0][0][0]], "b, first")
            assert lib.grail_fir_free(ctx.handle, fir_set) == G.ERR_INVALID_ARG and b"open filter streams" in lib.grail_last_error()
            out, out_len, _ = feed(ctx, d, sa, [x[100:] for x in xa])
            same(out, out_len, [m[0][1][0] for m in ma], "a, second")
            out, out_len, _ = feed(ctx, d, sb, [xb[0][150:]])
            same(out, out_len, [mb[0][0][1][0]], "b, second")
            out, out_len = ring_out(ctx, d, sa, 2, 32)
            same(out, out_len, [m[1] for m in ma], "a, tail")
            ctx.fir_stream_close(sa)
            assert lib.grail_fir_free(ctx.handle, fir_set) == G.ERR_INVALID_ARG
            assert lib.grail_filter_stream_close(ctx.handle, sa) == G.ERR_INVALID_ARG            # closed: looked up, not looked into
            buf = d.up(np.full(1024, CANARY, np.float32))
            d_len = d.up(np.full(2, 64, np.uint32))
            assert lib.grail_filter_stream_next_async(ctx.handle, sa, buf, 64, d_len, at(buf, 512), 64, None, None) == G.ERR_INVALID_ARG
            assert b"not an open filter stream" in lib.grail_last_error()
            with G.Context(0) as other:
                assert lib.grail_filter_stream_next_async(other.handle, sb, buf, 64, d_len, at(buf, 512), 64, None, None) == G.ERR_INVALID_ARG
                assert lib.grail_filter_stream_finish_async(other.handle, sb, None, buf, 64, None) == G.ERR_INVALID_ARG
                assert lib.grail_filter_stream_close(other.handle, sb) == G.ERR_INVALID_ARG
                out = C.c_void_p(0x77)
                assert lib.grail_filter_stream_open(other.handle, fir_set, 1, None, C.addressof(out)) == G.ERR_INVALID_ARG and out.value == 0x77
            # the refusals that need a stream: an index outside the set, no room for the tails, too many chunks
            out = C.c_void_p(0x77)
            assert lib.grail_filter_stream_open(ctx.handle, fir_set, 2, np.array([0, 2], np.uint32).ctypes.data, C.addressof(out)) == G.ERR_INVALID_ARG
            assert lib.grail_filter_stream_open(ctx.handle, fir_set, 0, None, C.addressof(out)) == G.ERR_INVALID_ARG and out.value == 0x77
            assert lib.grail_filter_stream_finish_async(ctx.handle, sb, None, buf, 31, None) == G.ERR_INVALID_ARG
            assert b"longest n_taps - 1" in lib.grail_last_error()
            assert lib.grail_filter_stream_next_async(ctx.handle, sb, buf, 64, d_len, at(buf, 32), 64, None, None) == G.ERR_INVALID_ARG
            assert b"overlaps" in lib.grail_last_error()
            assert lib.grail_filter_stream_next_async(ctx.handle, sb, buf, 64, d_len, at(buf, 512), 63, None, None) == G.ERR_INVALID_ARG
            ctx.sync()
            assert np.all(d.down(buf, 1024, np.float32) == CANARY)
            out, out_len = ring_out(ctx, d, sb, 1, 32)                                             # ... and none of them touched b
            same(out, out_len, [mb[0][1]], "b, tail")
            ctx.fir_stream_close(sb)
            ctx.fir_stream_close(None)
            ctx.fir_free(fir_set)
            # a stream left open goes with the context, its set with it
            left = ctx.fir_create(filters)
            ctx.fir_stream_open(left, 3)
        finally:
            d.free()


# ---- 10. the chain -----------------------------------------------------------------------------------------------------------------
def test_a_live_stream_pulled_in_chunks_through_the_telephone_band(built):
    """four live rows of half a second, pulled 480 samples at a time (10 ms at 48 kHz) straight into the filter stream (300 -
    3 400 Hz, 255 taps, origin 127), then finished: byte for byte the one-shot rendering through grail_fir_async"""
    rate, n, K, q = 48000, 4, 255, 480
    h = G.fir_design(rate, 300.0, 3400.0, K)
    segs, offs, vids, seeds = W.make_batch(n, sample_rate=rate, length=0.125, blend_length=0.125)
    stride = W.max_samples(length=0.125, sample_rate=rate)
    out_stride = (stride + K + 63) // 64 * 64
    with G.Context(0) as ctx:
        ctx.set_voices(W.single_voice(sample_rate=rate))
        d = Dev(ctx)
        fir_set = ctx.fir_create([(h, K // 2)])
        b = ctx.upload(segs, offs, vids, seeds)
        live = G.LiveStream(ctx, n, vids, seeds, ring_segments=8)
        fs = ctx.fir_stream_open(fir_set, n)
        try:
            # the one-shot rendering, filtered at once
            d_rows, d_len = d.alloc(n * stride * 4), d.alloc(n * 4)
            d_ref, d_ref_len = d.up(np.full(n * out_stride, CANARY, np.float32)), d.alloc(n * 4)
            b.synthesize_async(d_rows, stride, d_len)
            ctx.fir_async(fir_set, d_rows, stride, d_len, n, None, d_ref, out_stride, d_ref_len, None)
            ref = d.down(d_ref, (n, out_stride), np.float32)
            ref_len = d.down(d_ref_len, n, np.uint32)
            lens = d.down(d_len, n, np.uint32)
            assert lens.min() > 20000 and np.array_equal(ref_len, lens + K // 2)
            # the same script live: every pulled chunk goes through the filter before anything leaves the device
            live.append(segs, offs)
            live.finish()
            d_chunk, d_chunk_len = d.alloc(n * q * 4), d.alloc(n * 4)
            d_out, d_out_len = d.alloc(n * q * 4), d.alloc(n * 4)
            got = [[] for _ in range(n)]
            calls = -(-int(lens.max()) // q)
            assert calls <= 60
            for _ in range(calls):
                live.next_async(q, d_chunk, q, d_chunk_len)
                ctx.fir_stream_next_async(fs, d_chunk, q, d_chunk_len, d_out, q, d_out_len, None)
                out, out_len = d.down(d_out, (n, q), np.float32), d.down(d_out_len, n, np.uint32)
                for i in range(n):
                    got[i].append(out[i, :out_len[i]].copy())
            d_tail = d.alloc(n * K * 4)
            tail_len = ctx.fir_stream_finish(fs, n, d_tail, K)
            tail = d.down(d_tail, (n, K), np.float32)
            for i in range(n):
                row = np.concatenate(got[i] + [tail[i, :tail_len[i]]])
                assert len(row) == ref_len[i] and tail_len[i] == K - 1, (i, len(row), ref_len[i], tail_len[i])
                assert row.tobytes() == ref[i, :ref_len[i]].tobytes(), i
        finally:
            ctx.fir_stream_close(fs)
            live.close()
            b.free()
            ctx.fir_free(fir_set)
            d.free()


# ---- the example -----------------------------------------------------------------------------------------------------------------
def test_grail_interactive_band_option(gpu_ctx):
    """the same script with and without --band 300 3400 --taps 63: the same phonemes fed at the same samples; the filtered
    session is the model's filtering of the plain one in one piece, the filter's tail behind it"""
    import os
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "grail-rs_amd", "lib", "grail_interactive")
    script = b"ae\n@0.6 oui\n"
    runs = {}
    for name, extra in (("plain", []), ("band", ["--band", "300", "3400", "--taps", "63"])):
        r = subprocess.run([exe] + extra + ["441", "0.2"], input=script, capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr.decode()
        runs[name] = (np.frombuffer(r.stdout, dtype="<f4"), r.stderr.decode())
    plain, band = runs["plain"][0], runs["band"][0]
    fed = [re.findall(r"fed (\w+) at (\d+)", runs[name][1]) for name in ("plain", "band")]
    assert fed[0] == fed[1] and len(fed[0]) > 4 and len(plain) > 20000
    m = re.search(r"Filtered 300 - 3400 Hz at 44100 Hz \(63 taps\): (\d+) samples written", runs["band"][1])
    assert m and int(m.group(1)) == len(band) == len(plain) + 31, runs["band"][1]
    assert "Filtered" not in runs["plain"][1]
    y, n_out, _ = fir_model(plain, G.fir_design(44100, 300.0, 3400.0, 63), 31)
    assert n_out == len(band) and band.tobytes() == y.tobytes()
