"""Resample streams on the device (grail_resample_stream_*) against the numpy model of tests/resample_stream_model.py, bit
for bit in the samples, the lengths and the non-finite counts of every call and of the tails: the calls' outputs end to end,
then the tail, are what grail_resample_async gives for the whole row, whatever the split.  Every output buffer holds a canary
with guards around it, and the inputs hold NaN outside the rows' samples: nothing is written past out_len or outside the
buffer, nothing is read past a row's samples."""
import ctypes as C

import numpy as np
import pytest

import grail_hip as G
from grail_hip import workload as W
from fir_model import fir_model
from resample_model import resample_model
from resample_stream_model import ceil_div, splits, stream_len, stream_model
from test_levels_gpu import CANARY, Dev, dev  # noqa: F401  (dev is a fixture)

pytestmark = pytest.mark.gpu
CHUNK = G.RESAMPLE_CHUNK
REFUSED = 0xFFFFFFFF
# (48000, 2000) and (50, 3): a chunk's stretch reaches further than LDS holds, so the taps read the ring and the call's
# samples themselves, with one phase and with three
PAIRS = [(2, 3), (3, 2), (48000, 16000), (48000, 96000), (44100, 48000), (48000, 44100), (44100, 16000), (48000, 2000), (50, 3)]
# the issue's three, and the two other ways to the coefficients (test_resample_stream_host.py: every instantiation)
LAYOUT_PAIRS = [(48000, 16000), (44100, 48000), (50, 3), (44100, 16000), (48000, 2000)]
_tables = {}


def table(pair):
    """(numerators int32[U, P], U, D, P), from the library, once per pair"""
    if pair not in _tables:
        U, D, P = G.resample_ratio(*pair)
        _tables[pair] = (G.resample_coefficients(*pair), U, D, P)
    return _tables[pair]


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def at(ptr, floats):
    return C.c_void_p(ptr.value + 4 * floats)


def noise(n, rng, cuts=()):
    """uniform in +-1 with -0.0; NaN / +-Inf at the ends, the middle and either side of every cut"""
    x = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    x[rng.random(n) < 0.1] = np.float32(-0.0)
    for i, t in enumerate([0, n - 1, n // 2] + [c - 1 for c in cuts] + list(cuts)):
        if 0 <= t < n:
            x[t] = (np.nan, np.inf, -np.inf)[i % 3]
    return x


def tail_room(pair):
    _, U, D, P = table(pair)
    return ceil_div(P // 2 * U, D)


def feed(ctx, dev, rs, pair, chunks, stride=None, out_stride=None, in_offset=0, out_offset=0, guard=64):
    """one `next` call: chunks[i] as row i of an input buffer that holds NaN everywhere else, the outputs into a buffer of the
    canary with `guard` floats of it before and after -> (out [n_rows, out_stride] as it lies on the device afterwards,
    out_len, nonfinite)"""
    _, U, D, _ = table(pair)
    n_rows = len(chunks)
    longest = max([len(c) for c in chunks] + [1])
    stride = stride or (longest + 63) // 64 * 64
    out_stride = (ceil_div(stride * U, D) + 3) // 4 * 4 if out_stride is None else out_stride
    host = np.full(n_rows * stride + in_offset, np.nan, np.float32)
    for i, c in enumerate(chunks):
        host[in_offset + i * stride:in_offset + i * stride + len(c)] = c
    d_in = dev.up(host)
    before = guard + out_offset
    d_out = dev.up(np.full(before + n_rows * out_stride + guard, CANARY, np.float32))
    d_len = dev.up(np.array([len(c) for c in chunks], np.uint32))
    out_len, bad = ctx.resample_stream_next(rs, n_rows, at(d_in, in_offset), stride, d_len, at(d_out, before), out_stride)
    out = dev.down(d_out, before + n_rows * out_stride + guard, np.float32)
    assert np.all(out[:before] == CANARY) and np.all(out[before + n_rows * out_stride:] == CANARY), "written outside out"
    return out[before:before + n_rows * out_stride].reshape(n_rows, out_stride), out_len, bad


def flush(ctx, dev, rs, n_rows, out_stride, which=None, out_offset=0, guard=64):
    """one `finish` call -> (out, out_len), as feed"""
    before = guard + out_offset
    d_out = dev.up(np.full(before + n_rows * out_stride + guard, CANARY, np.float32))
    out_len = ctx.resample_stream_finish(rs, n_rows, at(d_out, before), out_stride, which)
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


def stream_rows(ctx, dev, pair, rows, row_splits, tail_stride=None, max_calls=60, **layout):
    """rows[i] fed as row_splits[i] says (shorter splits pause at the end), then finished: every call and the tails against
    the model -> the rows' outputs end to end"""
    num, _, D, _ = table(pair)
    n_calls = max(len(s) for s in row_splits)
    assert n_calls <= max_calls
    row_splits = [list(s) + [0] * (n_calls - len(s)) for s in row_splits]
    models = [stream_model(x, num, D, s) for x, s in zip(rows, row_splits)]
    rs = ctx.resample_stream_open(pair[0], pair[1], len(rows))
    try:
        fed = [0] * len(rows)
        joined = [[] for _ in rows]
        for c in range(n_calls):
            chunks = [x[a:a + s[c]] for x, a, s in zip(rows, fed, row_splits)]
            out, out_len, bad = feed(ctx, dev, rs, pair, chunks, **layout)
            same(out, out_len, [m[0][c][0] for m in models], ("call", c), bad, [m[0][c][1] for m in models])
            for i in range(len(rows)):
                joined[i].append(out[i, :out_len[i]])
                fed[i] += row_splits[i][c]
        room = tail_room(pair)
        out, out_len = flush(ctx, dev, rs, len(rows), (room + 7) // 4 * 4 if tail_stride is None else tail_stride,
                             out_offset=layout.get("out_offset", 0))
        same(out, out_len, [m[1] for m in models], "tail")
        for i in range(len(rows)):
            joined[i].append(out[i, :out_len[i]])
    finally:
        ctx.resample_stream_close(rs)
    return [np.concatenate(j) for j in joined]


def whole_rows(joined, pair, rows):
    """... and they are the one-shot rows, their counts the row's count"""
    num, _, D, _ = table(pair)
    for i, x in enumerate(rows):
        y, n_out, _ = resample_model(x, num, D)
        assert len(joined[i]) == n_out and np.array_equal(bits(joined[i]), bits(y)), (pair, i, len(x))


# ---- 1. every split gives the one-shot row -----------------------------------------------------------------------------------
def every_split_rows(pair):
    """the rows and splits of the test below (tests/test_kernel_paths_host.py walks the same ones for the kernel's variants)"""
    rng = np.random.default_rng(300 + pair[0] % 97 + pair[1] % 89)
    _, U, D, P = table(pair)
    h, Ci = P // 2, ceil_div(CHUNK * D, U)
    rows, row_splits = [], []
    for N in sorted({0, 1, h, h + 1, P - 1, P, Ci + 1, 2 * Ci + 17}):
        for split in splits(N, P, Ci, rng):
            rows.append(noise(N, rng, np.cumsum(split)))
            row_splits.append(split)
    return rows, row_splits


@pytest.mark.parametrize("pair", PAIRS)
def test_every_split_gives_the_one_shot_row(gpu_ctx, dev, pair):
    """one stream per pair: a row for every length and split.  Rows short of h write only a tail; [1, h, h + 1, 0, rest]
    lands a call exactly on the first output; Ci + 1 and 2 Ci + 17 put a chunk seam inside a call; every call but the first
    reads the ring, and the long rows wrap it; (48000, 2000) and (50, 3) are not staged (stream_model asserts that the
    calls' counts add up to the row's and that their non-finite counts do)"""
    _, U, D, P = table(pair)
    rows, row_splits = every_split_rows(pair)
    assert any(max(s) > ceil_div(CHUNK * D, U) for s in row_splits)         # a seam inside a call
    joined = stream_rows(gpu_ctx, dev, pair, rows, row_splits)
    whole_rows(joined, pair, rows)
    # the calls' counts add up to the row's
    num = table(pair)[0]
    for x, s in zip(rows, row_splits):
        assert sum(b for _, b in stream_model(x, num, D, s)[0]) == resample_model(x, num, D)[2]


# ---- 2. one sample per call ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", [(3, 2), (2, 3)])
def test_one_sample_per_call(gpu_ctx, dev, pair):
    """rows of 60 samples in 60 calls, then the tail: the start-up (no output before sample h + 1), calls that write two
    outputs, one and none, every position of the phase; the second row is paused in every other call and ends at 30"""
    rng = np.random.default_rng(40 + pair[0])
    rows = [noise(60, rng), noise(30, rng), noise(60, rng, range(1, 60, 7))]
    row_splits = [[1] * 60, [c % 2 for c in range(60)], [1] * 60]
    joined = stream_rows(gpu_ctx, dev, pair, rows, row_splits)
    whole_rows(joined, pair, rows)


# ---- 3. layout independence ------------------------------------------------------------------------------------------------------
def layout_splits(pair):
    """the splits and the four layouts of the test below (tests/test_kernel_paths_host.py walks the same ones)"""
    _, U, D, P = table(pair)
    Ci = ceil_div(CHUNK * D, U)
    row_splits = [[Ci + 1, 3, Ci // 2 + 13], [5, Ci - 4, 0], [1, 0, 699]]
    stride = (Ci + 1 + 63) // 64 * 64
    need, room = ceil_div(stride * U, D), tail_room(pair)
    return row_splits, [dict(stride=stride),
                        dict(stride=stride, in_offset=1, out_offset=1),
                        dict(stride=stride + 1, out_stride=(ceil_div((stride + 1) * U, D) + 7) | 1, tail_stride=room | 1),
                        dict(stride=stride, out_stride=need, tail_stride=room)]


@pytest.mark.parametrize("pair", LAYOUT_PAIRS)
def test_every_layout_gives_the_same_bits(gpu_ctx, dev, pair):
    """aligned bases and strides that are multiples of 4 (16-byte loads and stores); both bases one float off; odd strides
    with an out_stride above the need (the 4-byte variant)"""
    rng = np.random.default_rng(70 + pair[0] % 97 + pair[1] % 89)
    row_splits, layouts = layout_splits(pair)
    rows = [noise(sum(s), rng, np.cumsum(s)) for s in row_splits]
    a, b, c, d = [stream_rows(gpu_ctx, dev, pair, rows, row_splits, **layout) for layout in layouts]
    whole_rows(a, pair, rows)
    for other in (b, c, d):
        assert all(np.array_equal(bits(p), bits(q)) for p, q in zip(a, other))


# ---- 3b. every count of passes ---------------------------------------------------------------------------------------------------
PASS = 256      # the outputs of one pass of a chunk (resample_kernels.hip's RS_THREADS; tests/test_kernel_paths_host.py)


def pass_calls(pair):
    """calls of 300, 600 and 900 outputs: a chunk of two, of three and of four passes (a chunk of one is everywhere), which the
    splits above reach only where their seeds happen to -> (the samples of each call, the outputs of each).  Where a sample
    brings two outputs a call may write one more than asked."""
    _, U, D, P = table(pair)
    split, counts, N = [], [], 0
    for target in (300, 600, 900):
        n = 0
        while stream_len(N, n, U, D, P) < target:
            n += 1
        split.append(n)
        counts.append(stream_len(N, n, U, D, P))
        N += n
    assert all(t <= c <= t + 1 for t, c in zip((300, 600, 900), counts)) and [ceil_div(c, PASS) for c in counts] == [2, 3, 4]
    return split, counts


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "offset"])
@pytest.mark.parametrize("pair", LAYOUT_PAIRS)
def test_calls_of_two_three_and_four_passes(gpu_ctx, dev, pair, aligned):
    """the five ways to the stretch and the coefficients, with 16-byte and with 4-byte loads and stores: all ten variants of
    the kernel, each under rs_outputs<..., 2>, <..., 3> and <..., 4>"""
    split, _ = pass_calls(pair)
    rng = np.random.default_rng(170 + pair[0] % 97 + pair[1] % 89)
    rows = [noise(sum(split), rng, np.cumsum(split))]
    layout = {} if aligned else dict(in_offset=1, out_offset=1)
    joined = stream_rows(gpu_ctx, dev, pair, rows, [split], **layout)
    whole_rows(joined, pair, rows)


# ---- 4. refusals and state -------------------------------------------------------------------------------------------------------
def test_finish_marks_rows_and_ended_rows_are_refused(gpu_ctx, dev):
    """finish with `which` marking half the rows; the rest carry on and finish later; an ended row that is fed is refused and
    nothing of it changes, its neighbours unaffected; an ended row fed nothing writes nothing; finish twice writes nothing
    the second time"""
    rng = np.random.default_rng(77)
    pair, n_rows = (44100, 48000), 6
    num, U, D, P = table(pair)
    room = tail_room(pair)
    rows = [noise(160, rng) for _ in range(n_rows)]
    early = [0, 2, 4]
    empty = np.zeros(0, np.float32)
    rs = gpu_ctx.resample_stream_open(*pair, n_rows)
    try:
        models = [stream_model(x[:100], num, D, [100]) if i in early else stream_model(x, num, D, [100, 60])
                  for i, x in enumerate(rows)]
        out, out_len, bad = feed(gpu_ctx, dev, rs, pair, [x[:100] for x in rows])
        same(out, out_len, [m[0][0][0] for m in models], "first", bad, [m[0][0][1] for m in models])
        out, out_len = flush(gpu_ctx, dev, rs, n_rows, room, which=[1, 0, 1, 0, 1, 0])
        same(out, out_len, [models[i][1] if i in early else empty for i in range(n_rows)], "half finished")
        # rows 0 and 4 have ended and are fed: refused; row 2 has ended and is fed nothing; the others carry on
        chunks = [rows[0][100:110], rows[1][100:], empty, rows[3][100:], rows[4][100:105], rows[5][100:]]
        out, out_len, bad = feed(gpu_ctx, dev, rs, pair, chunks)
        want = [None, models[1][0][1][0], empty, models[3][0][1][0], None, models[5][0][1][0]]
        same(out, out_len, want, "second", bad, [0, models[1][0][1][1], 0, models[3][0][1][1], 0, models[5][0][1][1]])
        out, out_len = flush(gpu_ctx, dev, rs, n_rows, room, which=[1, 0, 1, 0, 0, 0])          # ended before: nothing
        same(out, out_len, [empty] * n_rows, "ended rows finished again")
        out, out_len = flush(gpu_ctx, dev, rs, n_rows, room + 5)                                 # NULL: all that are left
        same(out, out_len, [empty if i in early else models[i][1] for i in range(n_rows)], "the rest")
        out, out_len = flush(gpu_ctx, dev, rs, n_rows, room)
        same(out, out_len, [empty] * n_rows, "finish twice")
        out, out_len, bad = feed(gpu_ctx, dev, rs, pair, [x[:7] for x in rows])
        same(out, out_len, [None] * n_rows, "all ended", bad)
    finally:
        gpu_ctx.resample_stream_close(rs)


def test_out_stride_bounds_and_streams_that_are_not_this_contexts(built):
    """a context of its own: out_stride one below each bound is refused and exactly at it accepted; a closed stream and
    another context's are refused without being read; none of the refused calls wrote anything or moved the stream"""
    rng = np.random.default_rng(99)
    lib = G.load()
    pair = (48000, 44100)
    num, U, D, P = table(pair)
    room = tail_room(pair)
    with G.Context(0) as ctx:
        d = Dev(ctx)
        try:
            x = noise(300, rng)
            model = stream_model(x, num, D, [128, 172])
            sa, sb = ctx.resample_stream_open(*pair, 1), ctx.resample_stream_open(*pair, 2)
            buf = d.up(np.full(2048, CANARY, np.float32))
            d_len = d.up(np.full(2, 128, np.uint32))
            need = ceil_div(128 * U, D)
            assert need == G.resample_len(128, *pair) == 118
            assert lib.grail_resample_stream_next_async(ctx.handle, sa, buf, 128, d_len, at(buf, 1024), need - 1, None, None) == G.ERR_INVALID_ARG
            assert b"never cuts outputs short" in lib.grail_last_error()
            assert lib.grail_resample_stream_finish_async(ctx.handle, sa, None, at(buf, 1024), room - 1, None) == G.ERR_INVALID_ARG
            assert b"longest tail" in lib.grail_last_error()
            assert lib.grail_resample_stream_next_async(ctx.handle, sa, buf, 128, d_len, at(buf, 64), need, None, None) == G.ERR_INVALID_ARG
            assert b"overlaps" in lib.grail_last_error()
            assert lib.grail_resample_stream_next_async(ctx.handle, sa, buf, 128, None, at(buf, 1024), need, None, None) == G.ERR_INVALID_ARG
            assert lib.grail_resample_stream_finish_async(ctx.handle, sa, None, None, room, None) == G.ERR_INVALID_ARG
            out = C.c_void_p(0x77)
            assert lib.grail_resample_stream_open(ctx.handle, 48000, 48000, 1, C.addressof(out)) == G.ERR_INVALID_ARG
            assert lib.grail_resample_stream_open(ctx.handle, *pair, 0, C.addressof(out)) == G.ERR_INVALID_ARG and out.value == 0x77
            with G.Context(0) as other:
                assert lib.grail_resample_stream_next_async(other.handle, sb, buf, 128, d_len, at(buf, 1024), 128, None, None) == G.ERR_INVALID_ARG
                assert b"not an open resample stream" in lib.grail_last_error()
                assert lib.grail_resample_stream_finish_async(other.handle, sb, None, buf, 64, None) == G.ERR_INVALID_ARG
                assert lib.grail_resample_stream_close(other.handle, sb) == G.ERR_INVALID_ARG
            ctx.resample_stream_close(sb)
            assert lib.grail_resample_stream_close(ctx.handle, sb) == G.ERR_INVALID_ARG           # closed: looked up, not looked into
            assert lib.grail_resample_stream_next_async(ctx.handle, sb, buf, 128, d_len, at(buf, 1024), 128, None, None) == G.ERR_INVALID_ARG
            assert b"not an open resample stream" in lib.grail_last_error()
            ctx.sync()
            assert np.all(d.down(buf, 2048, np.float32) == CANARY)
            # exactly at the bounds, and none of the above moved the stream
            out, out_len, bad = feed(ctx, d, sa, pair, [x[:128]], stride=128, out_stride=need)
            same(out, out_len, [model[0][0][0]], "at the bound", bad, [model[0][0][1]])
            out, out_len, bad = feed(ctx, d, sa, pair, [x[128:]])
            same(out, out_len, [model[0][1][0]], "second", bad, [model[0][1][1]])
            out, out_len = flush(ctx, d, sa, 1, room)
            same(out, out_len, [model[1]], "tail at the bound")
            ctx.resample_stream_close(sa)
            ctx.resample_stream_close(None)
            ctx.resample_stream_open(*pair, 3)          # a stream left open goes with the context
        finally:
            d.free()


# ---- 5. the table outlives the cache ---------------------------------------------------------------------------------------------
def test_the_stream_keeps_its_table_when_the_cache_evicts_the_pair(gpu_ctx, dev):
    """half a row through a stream on (44100, 48000); grail_resample_async on that pair and then on five others, so that the
    context's four tables have all been replaced; the rest of the row and the tail: the one-shot row"""
    rng = np.random.default_rng(123)
    pair = (44100, 48000)
    num, U, D, P = table(pair)
    x = noise(2000, rng, [1000])
    model = stream_model(x, num, D, [1000, 1000])
    rs = gpu_ctx.resample_stream_open(*pair, 1)
    try:
        out, out_len, bad = feed(gpu_ctx, dev, rs, pair, [x[:1000]])
        same(out, out_len, [model[0][0][0]], "first half", bad, [model[0][0][1]])
        d_in, d_len = dev.up(np.ones(256, np.float32)), dev.up(np.array([256], np.uint32))
        d_out = dev.alloc(4 * 4096)
        for other in [pair, (48000, 16000), (48000, 96000), (48000, 44100), (44100, 16000), (3, 2)]:
            out_len, _ = gpu_ctx.resample(d_in, 256, d_len, 1, other[0], other[1], d_out, 4096)
            assert out_len[0] == G.resample_len(256, *other)
        out, out_len, bad = feed(gpu_ctx, dev, rs, pair, [x[1000:]])
        same(out, out_len, [model[0][1][0]], "second half", bad, [model[0][1][1]])
        out, out_len = flush(gpu_ctx, dev, rs, 1, tail_room(pair))
        same(out, out_len, [model[1]], "tail")
    finally:
        gpu_ctx.resample_stream_close(rs)
    whole = np.concatenate([model[0][0][0], model[0][1][0], model[1]])
    assert np.array_equal(bits(whole), bits(resample_model(x, num, D)[0]))


# ---- 6. queued calls ---------------------------------------------------------------------------------------------------------------
def test_calls_queued_with_their_input_overwritten_behind_them(gpu_ctx, dev):
    """three `next` calls with results left on the device, each from a buffer of its own, a grail_memset_d of that buffer
    (NaN everywhere) queued right behind it: the call kept its own copy of the samples the next one needs"""
    rng = np.random.default_rng(88)
    pair, n_rows, n = (48000, 16000), 3, 480
    num, U, D, P = table(pair)
    rows = [noise(3 * n, rng) for _ in range(n_rows)]
    models = [stream_model(x, num, D, [n] * 3) for x in rows]
    stride = 512
    rs = gpu_ctx.resample_stream_open(*pair, n_rows)
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
            gpu_ctx.resample_stream_next_async(rs, d_ins[c], stride, d_len, d_outs[c], stride, *d_res[c])
            gpu_ctx.memset(d_ins[c], 0xFF, n_rows * stride * 4)                   # (NaN everywhere)
        gpu_ctx.sync()
        for c in range(3):
            out = dev.down(d_outs[c], (n_rows, stride), np.float32)
            out_len, bad = dev.down(d_res[c][0], n_rows, np.uint32), dev.down(d_res[c][1], n_rows, np.uint32)
            same(out, out_len, [m[0][c][0] for m in models], ("queued", c), bad, [m[0][c][1] for m in models])
    finally:
        gpu_ctx.resample_stream_close(rs)


def test_two_finishing_calls_with_marks_queued_back_to_back(gpu_ctx, dev):
    """two `finish` calls with marks, their results left on the device, and no wait between them: the second writes the
    stream's host copy of the marks anew, which the first's upload may not have read yet, so it waits for the event behind that
    upload.  The first unit's tail comes from the first call alone and the others' from the second; behind what the feeding
    call wrote they are the one-shot rows"""
    rng = np.random.default_rng(67)
    pair, n_rows, n = (2, 3), 3, 40
    rows = [noise(n, rng) for _ in range(n_rows)]
    stride, guard, marks = (tail_room(pair) + 7) // 4 * 4, 64, ([1, 0, 0], [0, 1, 1])
    rs = gpu_ctx.resample_stream_open(pair[0], pair[1], n_rows)
    try:
        out, out_len, _ = feed(gpu_ctx, dev, rs, pair, rows)
        joined = [[out[i, :out_len[i]]] for i in range(n_rows)]
        d_outs = [dev.up(np.full(guard + n_rows * stride + guard, CANARY, np.float32)) for _ in range(2)]
        d_lens = [dev.up(np.full(n_rows, 77, np.uint32)) for _ in range(2)]
        for d_out, d_len, which in zip(d_outs, d_lens, marks):
            gpu_ctx.resample_stream_finish(rs, n_rows, at(d_out, guard), stride, which, out_len_dev=d_len)
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
        gpu_ctx.resample_stream_close(rs)
    whole_rows([np.concatenate(j) for j in joined], pair, rows)


# ---- 7. the chain ------------------------------------------------------------------------------------------------------------------
def test_a_live_stream_through_the_telephone_band_down_to_8000(built):
    """one live row of a quarter second at 48 kHz, pulled 441 samples at a time straight into the filter stream (300 - 3 400
    Hz, 255 taps, origin 127) and from there into the resample stream to 8 000; the tails in chain order: the filter's tail
    is fed to the resampler, then the resampler's tail.  Byte for byte grail_fir_async then grail_resample_async on the
    one-shot rendering"""
    rate, rate_out, n, K, q = 48000, 8000, 1, 255, 441
    U, D, P = G.resample_ratio(rate, rate_out)
    h = G.fir_design(rate, 300.0, 3400.0, K)
    segs, offs, vids, seeds = W.make_batch(n, sample_rate=rate, length=0.0625, blend_length=0.0625)
    stride = W.max_samples(length=0.0625, sample_rate=rate)
    fir_stride = (stride + K + 63) // 64 * 64
    out_stride = (G.resample_len(fir_stride, rate, rate_out) + 63) // 64 * 64
    q_out = max(G.resample_len(q, rate, rate_out), G.resample_len(K, rate, rate_out), ceil_div(P // 2 * U, D))
    with G.Context(0) as ctx:
        ctx.set_voices(W.single_voice(sample_rate=rate))
        d = Dev(ctx)
        fir_set = ctx.fir_create([(h, K // 2)])
        b = ctx.upload(segs, offs, vids, seeds)
        live = G.LiveStream(ctx, n, vids, seeds, ring_segments=8)
        fs = ctx.fir_stream_open(fir_set, n)
        rs = ctx.resample_stream_open(rate, rate_out, n)
        try:
            # the one-shot rendering, filtered and resampled at once
            d_rows, d_len = d.alloc(n * stride * 4), d.alloc(n * 4)
            d_fir, d_fir_len = d.alloc(n * fir_stride * 4), d.alloc(n * 4)
            d_ref, d_ref_len = d.up(np.full(n * out_stride, CANARY, np.float32)), d.alloc(n * 4)
            b.synthesize_async(d_rows, stride, d_len)
            ctx.fir_async(fir_set, d_rows, stride, d_len, n, None, d_fir, fir_stride, d_fir_len, None)
            ctx.resample_async(d_fir, fir_stride, d_fir_len, n, rate, rate_out, d_ref, out_stride, d_ref_len, None)
            ref = d.down(d_ref, (n, out_stride), np.float32)
            ref_len = d.down(d_ref_len, n, np.uint32)
            lens = d.down(d_len, n, np.uint32)
            assert 10000 < lens.min() and np.array_equal(ref_len, [G.resample_len(int(v) + K // 2, rate, rate_out) for v in lens])
            # the same script live: every pulled chunk goes through both streams before anything leaves the device
            live.append(segs, offs)
            live.finish()
            d_chunk, d_chunk_len = d.alloc(n * q * 4), d.alloc(n * 4)
            d_mid, d_mid_len = d.alloc(n * q * 4), d.alloc(n * 4)
            d_out, d_out_len = d.alloc(n * q_out * 4), d.alloc(n * 4)
            got = [[] for _ in range(n)]

            def take():
                out, out_len = d.down(d_out, (n, q_out), np.float32), d.down(d_out_len, n, np.uint32)
                for i in range(n):
                    got[i].append(out[i, :out_len[i]].copy())

            calls = -(-int(lens.max()) // q)
            assert calls <= 60
            for _ in range(calls):
                live.next_async(q, d_chunk, q, d_chunk_len)
                ctx.fir_stream_next_async(fs, d_chunk, q, d_chunk_len, d_mid, q, d_mid_len, None)
                ctx.resample_stream_next_async(rs, d_mid, q, d_mid_len, d_out, q_out, d_out_len, None)
                take()
            # the filter's tail is fed to the resampler, then the resampler's own
            ctx.fir_stream_finish(fs, n, d_mid, q, out_len_dev=d_mid_len)
            ctx.resample_stream_next_async(rs, d_mid, q, d_mid_len, d_out, q_out, d_out_len, None)
            take()
            ctx.resample_stream_finish(rs, n, d_out, q_out, out_len_dev=d_out_len)
            take()
            for i in range(n):
                row = np.concatenate(got[i])
                assert len(row) == ref_len[i], (i, len(row), ref_len[i])
                assert row.tobytes() == ref[i, :ref_len[i]].tobytes(), i
        finally:
            ctx.resample_stream_close(rs)
            ctx.fir_stream_close(fs)
            live.close()
            b.free()
            ctx.fir_free(fir_set)
            d.free()


def test_grail_interactive_band_and_rate_options(gpu_ctx):
    """the same script plain and with --band 300 3400 --taps 63 --rate 8000: the same phonemes fed at the same samples; the
    session's output is the model's filtering and resampling of the plain one in one piece"""
    import os
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "grail-rs_amd", "lib", "grail_interactive")
    script = b"ae\n@0.6 oui\n"
    runs = {}
    for name, extra in (("plain", []), ("chain", ["--band", "300", "3400", "--taps", "63", "--rate", "8000"]), ("rate", ["--rate", "8000"])):
        r = subprocess.run([exe] + extra + ["441", "0.2"], input=script, capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr.decode()
        runs[name] = (np.frombuffer(r.stdout, dtype="<f4"), r.stderr.decode())
    plain, chain, rate = runs["plain"][0], runs["chain"][0], runs["rate"][0]
    fed = [re.findall(r"fed (\w+) at (\d+)", runs[name][1]) for name in ("plain", "chain", "rate")]
    assert fed[0] == fed[1] == fed[2] and len(fed[0]) > 4 and len(plain) > 20000
    num = G.resample_coefficients(44100, 8000)
    D = G.resample_ratio(44100, 8000)[1]
    y, n_mid, _ = fir_model(plain, G.fir_design(44100, 300.0, 3400.0, 63), 31)
    z, n_out, _ = resample_model(y, num, D)
    m = re.search(r"Resampled 44100 -> 8000 Hz: (\d+) samples written", runs["chain"][1])
    assert m and int(m.group(1)) == len(chain) == n_out == G.resample_len(len(plain) + 31, 44100, 8000), runs["chain"][1]
    assert chain.tobytes() == z.tobytes()
    z, n_out, _ = resample_model(plain, num, D)
    assert len(rate) == n_out and rate.tobytes() == z.tobytes()
    assert "Resampled" not in runs["plain"][1]
