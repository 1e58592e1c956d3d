"""Every waited-for form of the Python binding against its own _async form: the same values, dtypes and shapes.

A waited form allocates its result arrays on the device, runs the _async form on them, copies them back, waits and
releases.  Here the test does the same by hand (`queued`): device arrays it allocates, the _async form, a wait, its own
copies.  Streams change state when fed, so a stream form is held against a second stream fed the same.  Rows are 256
samples at a stride of 320 with lengths 0, 100 and 256; frame_levels and the loudness hop sums must come back holding the
fill where the kernels write nothing."""
import numpy as np
import pytest

import grail_hip as G

pytestmark = pytest.mark.gpu

STRIDE, FILLED, OUT_STRIDE = 320, 256, 512
RATE = G.LOUDNESS_RATE_MIN                      # a hop of 256 samples: one hop a full row, none for the shorter ones
SHAPES = [(1, [256]), (3, [0, 100, 256])]
U32, F32, F64, U64 = np.uint32, np.float32, np.float64, np.uint64


class Dev:
    """device arrays of one test, released together"""

    def __init__(self, ctx):
        self.ctx, self.held = ctx, []

    def alloc(self, nbytes):
        self.held.append(self.ctx.device_alloc(max(nbytes, 8)))
        return self.held[-1]

    def up(self, a):
        a = np.ascontiguousarray(a)
        p = self.alloc(a.nbytes)
        if a.nbytes:
            self.ctx.h2d(p, a, a.nbytes)
        return p

    def down(self, p, shape, dtype):
        a = np.zeros(shape, dtype=dtype)
        if a.nbytes:
            self.ctx.d2h(a, p, a.nbytes)
        return a

    def out(self, n_rows):
        return self.up(np.zeros((max(n_rows, 1), OUT_STRIDE), F32))

    def release(self):
        self.ctx.sync()
        for p in self.held:
            self.ctx.device_free(p)
        self.held = []


@pytest.fixture
def dev(gpu_ctx):
    d = Dev(gpu_ctx)
    yield d
    d.release()


def rows_of(dev, lens, seed=5):
    """(rows_dev, len_dev) of len(lens) rows: FILLED random samples each, the lengths as given"""
    x = np.zeros((max(len(lens), 1), STRIDE), F32)
    x[:, :FILLED] = np.random.default_rng(seed).uniform(-1.0, 1.0, (x.shape[0], FILLED)).astype(F32)
    return dev.up(x), dev.up(np.array(list(lens) + [0], U32)[:max(len(lens), 1)])


def queued(dev, specs, call, fill=0):
    """The _async form by hand: a device array per (shape, dtype), the two-dimensional ones holding `fill` and the others
    zeros, call(*them), a wait, the copies."""
    d = [dev.up(np.full(shape, fill if len(shape) == 2 else 0, dtype)) for shape, dtype in specs]
    call(*d)
    dev.ctx.sync()
    return tuple(dev.down(p, shape, dtype) for p, (shape, dtype) in zip(d, specs))


def same(got, want):
    got = got if isinstance(got, tuple) else (got,)
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        if w is None:
            assert g is None, k
            continue
        assert isinstance(g, np.ndarray) and g.dtype == w.dtype and g.shape == w.shape, (k, g.dtype, g.shape, w.dtype, w.shape)
        assert g.tobytes() == w.tobytes(), (k, g, w)            # bit for bit: NaN fills and refusals included


def same_rows(dev, a_dev, b_dev, n_rows):
    a, b = (dev.down(p, (n_rows, OUT_STRIDE), F32) for p in (a_dev, b_dev))
    assert a.tobytes() == b.tobytes()


# ---- measurements ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,lens", SHAPES)
def test_levels_and_true_peak(gpu_ctx, dev, n, lens):
    ctx = gpu_ctx
    rows, ln = rows_of(dev, lens)
    same(ctx.levels(rows, STRIDE, ln, n),
         queued(dev, [((n,), F64), ((n,), F32), ((n,), U32)], lambda *d: ctx.levels_async(rows, STRIDE, ln, n, *d)))
    same(ctx.true_peak(rows, STRIDE, ln, n),
         queued(dev, [((n,), F64), ((n,), U32)], lambda *d: ctx.true_peak_async(rows, STRIDE, ln, n, *d)))


@pytest.mark.parametrize("fill", [None, 7.5])
@pytest.mark.parametrize("n,lens", SHAPES)
def test_frame_levels_keeps_the_fill_past_a_rows_end(gpu_ctx, dev, n, lens, fill):
    ctx, frame = gpu_ctx, 256                   # the least frame the call takes: two frames a row of 320
    frames = -(-STRIDE // frame)
    rows, ln = rows_of(dev, lens)
    got = ctx.frame_levels(rows, STRIDE, ln, n, frame, fill=fill)
    want = queued(dev, [((n, frames), F64), ((n, frames), F32)],
                  lambda s, p: ctx.frame_levels_async(rows, STRIDE, ln, n, frame, s, p, frames), np.nan if fill is None else fill)
    same(got, want)
    for u, length in enumerate(lens):                   # the kernels wrote the frames a row has and no other
        written = -(-length // frame)
        tail = got[0][u, written:]
        assert tail.size and np.all(np.isnan(tail) if fill is None else tail == fill)
        assert not np.any(np.isnan(got[0][u, :written]))


@pytest.mark.parametrize("fill", [None, -3.0])
@pytest.mark.parametrize("form", ["loudness", "loudness_segmented"])
@pytest.mark.parametrize("n,lens", SHAPES)
def test_loudness_keeps_the_fill_in_hops_a_row_has_not(gpu_ctx, dev, n, lens, form, fill):
    ctx = gpu_ctx
    hs = STRIDE // (RATE // 10)
    rows, ln = rows_of(dev, lens)
    waited, queued_form = getattr(ctx, form), getattr(ctx, form + "_async")
    got = waited(rows, STRIDE, ln, n, RATE, fill=fill)
    gated, bad, hops = queued(dev, [((n,), F64), ((n,), U32), ((n, hs), F64)],
                              lambda g, b, h: queued_form(rows, STRIDE, ln, n, RATE, None, g, h, hs, b),
                              np.nan if fill is None else fill)
    same(got, (gated, hops, bad))
    # the coefficients given as a list (the binding makes the array the library reads) are the library's own for the rate
    same(waited(rows, STRIDE, ln, n, RATE, coef=list(G.kweighting(RATE)), fill=fill), (gated, hops, bad))
    for u, length in enumerate(lens):
        tail = got[1][u, length // (RATE // 10):]
        assert np.all(np.isnan(tail) if fill is None else tail == fill)
    got = waited(rows, STRIDE, ln, n, RATE, hops=False)
    gated, bad = queued(dev, [((n,), F64), ((n,), U32)], lambda g, b: queued_form(rows, STRIDE, ln, n, RATE, None, g, None, 0, b))
    same(got, (gated, None, bad))


# ---- rows in, rows out -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,lens,group", [(1, [256], 1), (3, [0, 100, 256], 1), (3, [256, 256, 256], 3), (3, [0, 100, 256], 3)])
def test_limit(gpu_ctx, dev, n, lens, group):
    ctx = gpu_ctx
    rows, ln = rows_of(dev, lens)
    a, b = dev.out(n), dev.out(n)
    got = ctx.limit(rows, STRIDE, ln, n, 0.5, 4, a, OUT_STRIDE, group)
    want = queued(dev, [((n // group,), F32), ((n // group,), U32), ((n // group,), U32)],
                  lambda *d: ctx.limit_async(rows, STRIDE, ln, n, 0.5, 4, b, OUT_STRIDE, group, *d))
    same(got, want)
    same_rows(dev, a, b, n)


@pytest.fixture
def sets(gpu_ctx):
    """a filter set, a recursive filter set and a curve set on the shared context"""
    ctx = gpu_ctx
    fir = ctx.fir_create([(G.fir_design(48000, 0.0, 6000.0, 9), 4)])
    iir = ctx.iir_create([G.iir_design(G.IIR_LOWPASS, 48000, 3000.0, 0.707)])
    dyn = ctx.dyn_create([(G.dyn_design(G.DYN_COMPRESS, G.DYN_PEAK, -20.0, 4.0), G.dyn_ballistics(48000, 1.0, 50.0), G.DYN_PEAK)])
    yield fir, iir, dyn
    ctx.fir_free(fir)
    ctx.iir_free(iir)
    ctx.dyn_free(dyn)


@pytest.mark.parametrize("n,lens", SHAPES)
def test_resample_fir_iir_dyn(gpu_ctx, dev, sets, n, lens):
    ctx = gpu_ctx
    fir, iir, dyn = sets
    rows, ln = rows_of(dev, lens)
    pair, triple = [((n,), U32), ((n,), U32)], [((n,), U32), ((n,), U32), ((n,), F64)]
    forms = [
        (pair, lambda o: ctx.resample(rows, STRIDE, ln, n, 48000, 24000, o, OUT_STRIDE),
         lambda o, *d: ctx.resample_async(rows, STRIDE, ln, n, 48000, 24000, o, OUT_STRIDE, *d)),
        (pair, lambda o: ctx.fir(fir, rows, STRIDE, ln, n, None, o, OUT_STRIDE),
         lambda o, *d: ctx.fir_async(fir, rows, STRIDE, ln, n, None, o, OUT_STRIDE, *d)),
        (pair, lambda o: ctx.iir(iir, rows, STRIDE, ln, n, None, 8, o, OUT_STRIDE),
         lambda o, *d: ctx.iir_async(iir, rows, STRIDE, ln, n, None, 8, o, OUT_STRIDE, *d)),
        (pair, lambda o: ctx.iir_blocked(iir, rows, STRIDE, ln, n, None, 8, o, OUT_STRIDE),
         lambda o, *d: ctx.iir_blocked_async(iir, rows, STRIDE, ln, n, None, 8, o, OUT_STRIDE, *d)),
        (triple, lambda o: ctx.dyn(dyn, rows, STRIDE, ln, n, None, o, OUT_STRIDE),
         lambda o, *d: ctx.dyn_async(dyn, rows, STRIDE, ln, n, None, o, OUT_STRIDE, *d)),
        (triple, lambda o: ctx.track_dyn(dyn, rows, STRIDE, ln, n, None, o, OUT_STRIDE),
         lambda o, *d: ctx.track_dyn_async(dyn, rows, STRIDE, ln, n, None, o, OUT_STRIDE, *d)),
    ]
    for specs, waited, queued_form in forms:
        a, b = dev.out(n), dev.out(n)
        same(waited(a), queued(dev, specs, lambda *d: queued_form(b, *d)))
        same_rows(dev, a, b, n)


# ---- streams: the waited form on one stream, the _async form on a second fed the same ---------------------------------
@pytest.mark.parametrize("n,lens", SHAPES)
def test_handle_streams(gpu_ctx, dev, sets, n, lens):
    ctx = gpu_ctx
    fir, iir, dyn = sets
    rows, ln = rows_of(dev, lens)
    pair, triple, one = [((n,), U32), ((n,), U32)], [((n,), U32), ((n,), U32), ((n,), F64)], [((n,), U32)]
    marks = ([1, 0, 1] + [1] * n)[:n]
    kinds = [
        (lambda: ctx.fir_stream_open(fir, n), ctx.fir_stream_close, pair, ctx.fir_stream_next, ctx.fir_stream_next_async,
         ctx.fir_stream_finish),
        (lambda: ctx.iir_stream_open(iir, n, tail=8), ctx.iir_stream_close, pair, ctx.iir_stream_next, ctx.iir_stream_next_async,
         ctx.iir_stream_finish),
        (lambda: ctx.resample_stream_open(48000, 24000, n), ctx.resample_stream_close, pair, ctx.resample_stream_next,
         ctx.resample_stream_next_async, ctx.resample_stream_finish),
        (lambda: ctx.dyn_stream_open(dyn, n), ctx.dyn_stream_close, triple, ctx.dyn_stream_next, ctx.dyn_stream_next_async, None),
    ]
    for opener, close, specs, waited_next, queued_next, finish in kinds:
        sa, sb = opener(), opener()
        try:
            a, b = dev.out(n), dev.out(n)
            same(waited_next(sa, n, rows, STRIDE, ln, a, OUT_STRIDE),
                 queued(dev, specs, lambda *d: queued_next(sb, rows, STRIDE, ln, b, OUT_STRIDE, *d)))
            same_rows(dev, a, b, n)
            if finish is None:
                continue
            for which in (marks, None):                 # some rows, then what is left: both modes of the call
                a, b = dev.out(n), dev.out(n)
                tails = finish(sa, n, a, OUT_STRIDE, which)
                (want,) = queued(dev, one, lambda d: finish(sb, n, b, OUT_STRIDE, which, d))
                same(tails, (want,))
                same_rows(dev, a, b, n)
        finally:
            close(sa)
            close(sb)


@pytest.mark.parametrize("n,lens,group", [(1, [256], 1), (3, [0, 100, 256], 1), (3, [256, 256, 256], 3)])
def test_limit_stream(gpu_ctx, dev, n, lens, group):
    ctx, g = gpu_ctx, n // group
    rows, ln = rows_of(dev, lens)
    sa, sb = (ctx.limit_stream_open(n, 0.5, 4, group) for _ in range(2))
    try:
        a, b = dev.out(n), dev.out(n)
        same(sa.next(rows, STRIDE, ln, a, OUT_STRIDE),
             queued(dev, [((g,), U32), ((g,), F32), ((g,), U32), ((g,), U32)],
                    lambda *d: sb.next_async(rows, STRIDE, ln, b, OUT_STRIDE, *d)))
        same_rows(dev, a, b, n)
        for which in (([1, 0, 1] + [1] * g)[:g], None):
            a, b = dev.out(n), dev.out(n)
            same(sa.finish(a, OUT_STRIDE, which),
                 queued(dev, [((g,), U32), ((g,), F32), ((g,), U32)], lambda *d: sb.finish_async(b, OUT_STRIDE, which, *d)))
            same_rows(dev, a, b, n)
    finally:
        sa.close()
        sb.close()


@pytest.mark.parametrize("n,lens", SHAPES)
def test_meter_stream(gpu_ctx, dev, n, lens):
    ctx = gpu_ctx
    rows, ln = rows_of(dev, lens)
    # (the waited stream is given the rate's coefficients as a list, the other takes the library's own: the same numbers)
    sa, sb = ctx.meter_stream_open(n, RATE, 8, coef=list(G.kweighting(RATE))), ctx.meter_stream_open(n, RATE, 8)
    try:
        hs = sa.hops_stride(STRIDE)
        ha, hb = (dev.up(np.full((n, hs), -1.0, F64)) for _ in range(2))
        same(sa.next(rows, STRIDE, ln, ha, hs),
             queued(dev, [((n,), U32), ((n,), F64), ((n,), U32)], lambda *d: sb.next_async(rows, STRIDE, ln, hb, hs, *d)))
        assert dev.down(ha, (n, hs), F64).tobytes() == dev.down(hb, (n, hs), F64).tobytes()
        same(sa.read(), queued(dev, [((n,), F64)] * 4 + [((n,), U64)], sb.read_async))
        for which in (([1, 0, 1] + [1] * n)[:n], None):
            same(sa.finish(which), queued(dev, [((n,), F64)], lambda d: sb.finish_async(which, d)))
    finally:
        sa.close()
        sb.close()


# ---- what the library refuses on the host ----------------------------------------------------------------------------
def test_a_refused_call_raises_and_leaves_the_context_usable(gpu_ctx, dev, sets):
    ctx = gpu_ctx
    rows, ln = rows_of(dev, [0, 100, 256])
    out = dev.out(3)
    with pytest.raises(G.GrailError) as refused:
        ctx.fir(None, rows, STRIDE, ln, 3, None, out, OUT_STRIDE)         # no filter set: refused before anything is queued
    assert refused.value.status == G.ERR_INVALID_ARG
    out_len, bad = ctx.fir(sets[0], rows, STRIDE, ln, 3, None, out, OUT_STRIDE)
    assert list(out_len) == [G.fir_len(k, 9, 4) for k in (0, 100, 256)] and not bad.any()


def no_rows_outcomes(ctx, dev, sets):
    """What every waited form does with n_rows = 0: the dtypes and shapes it returns, or the status it raises.  A stream
    has the rows it was opened with, so the stream forms are asked through an open with no rows."""
    fir, iir, dyn = sets
    rows, ln = rows_of(dev, [])
    out = dev.out(0)

    def outcome(call):
        try:
            got = call()
        except G.GrailError as e:
            return f"GrailError {e.status}"
        got = got if isinstance(got, tuple) else (got,)
        return " ".join("None" if a is None else f"{a.dtype}{list(a.shape)}" for a in got)

    def stream(opener, close, use):
        try:
            st = opener()
        except G.GrailError as e:
            return f"open: GrailError {e.status}"
        try:
            return outcome(lambda: use(st))
        finally:
            close(st)

    return {
        "levels": outcome(lambda: ctx.levels(rows, STRIDE, ln, 0)),
        "frame_levels": outcome(lambda: ctx.frame_levels(rows, STRIDE, ln, 0, 256)),
        "loudness": outcome(lambda: ctx.loudness(rows, STRIDE, ln, 0, RATE)),
        "loudness hops=False": outcome(lambda: ctx.loudness(rows, STRIDE, ln, 0, RATE, hops=False)),
        "loudness_segmented": outcome(lambda: ctx.loudness_segmented(rows, STRIDE, ln, 0, RATE)),
        "true_peak": outcome(lambda: ctx.true_peak(rows, STRIDE, ln, 0)),
        "limit": outcome(lambda: ctx.limit(rows, STRIDE, ln, 0, 0.5, 4, out, OUT_STRIDE)),
        "resample": outcome(lambda: ctx.resample(rows, STRIDE, ln, 0, 48000, 24000, out, OUT_STRIDE)),
        "fir": outcome(lambda: ctx.fir(fir, rows, STRIDE, ln, 0, None, out, OUT_STRIDE)),
        "iir": outcome(lambda: ctx.iir(iir, rows, STRIDE, ln, 0, None, 8, out, OUT_STRIDE)),
        "iir_blocked": outcome(lambda: ctx.iir_blocked(iir, rows, STRIDE, ln, 0, None, 8, out, OUT_STRIDE)),
        "dyn": outcome(lambda: ctx.dyn(dyn, rows, STRIDE, ln, 0, None, out, OUT_STRIDE)),
        "track_dyn": outcome(lambda: ctx.track_dyn(dyn, rows, STRIDE, ln, 0, None, out, OUT_STRIDE)),
        "fir_stream": stream(lambda: ctx.fir_stream_open(fir, 0), ctx.fir_stream_close,
                             lambda st: ctx.fir_stream_next(st, 0, rows, STRIDE, ln, out, OUT_STRIDE)),
        "iir_stream": stream(lambda: ctx.iir_stream_open(iir, 0), ctx.iir_stream_close,
                             lambda st: ctx.iir_stream_next(st, 0, rows, STRIDE, ln, out, OUT_STRIDE)),
        "resample_stream": stream(lambda: ctx.resample_stream_open(48000, 24000, 0), ctx.resample_stream_close,
                                  lambda st: ctx.resample_stream_next(st, 0, rows, STRIDE, ln, out, OUT_STRIDE)),
        "dyn_stream": stream(lambda: ctx.dyn_stream_open(dyn, 0), ctx.dyn_stream_close,
                             lambda st: ctx.dyn_stream_next(st, 0, rows, STRIDE, ln, out, OUT_STRIDE)),
        "LimitStream": stream(lambda: ctx.limit_stream_open(0, 0.5, 4), lambda st: st.close(),
                              lambda st: st.next(rows, STRIDE, ln, out, OUT_STRIDE)),
        "MeterStream": stream(lambda: ctx.meter_stream_open(0, RATE, 8), lambda st: st.close(),
                              lambda st: st.next(rows, STRIDE, ln)),
    }


NO_ROWS = {
    "levels": "float64[0] float32[0] uint32[0]",
    "frame_levels": "float64[0, 2] float32[0, 2]",
    "loudness": "float64[0] float64[0, 1] uint32[0]",
    "loudness hops=False": "float64[0] None uint32[0]",
    "loudness_segmented": "float64[0] float64[0, 1] uint32[0]",
    "true_peak": "float64[0] uint32[0]",
    "limit": "float32[0] uint32[0] uint32[0]",
    "resample": "uint32[0] uint32[0]",
    "fir": "uint32[0] uint32[0]",
    "iir": "uint32[0] uint32[0]",
    "iir_blocked": "uint32[0] uint32[0]",
    "dyn": "uint32[0] uint32[0] float64[0]",
    "track_dyn": "uint32[0] uint32[0] float64[0]",
    "fir_stream": "open: GrailError -1",
    "iir_stream": "open: GrailError -1",
    "resample_stream": "open: GrailError -1",
    "dyn_stream": "open: GrailError -1",
    "LimitStream": "open: GrailError -1",
    "MeterStream": "open: GrailError -1",
}


def test_no_rows(gpu_ctx, dev, sets):
    """n_rows = 0, form by form: NO_ROWS is what the binding did before its waited forms became one helper, observed on the
    device on the commit before, and what it must go on doing."""
    got = no_rows_outcomes(gpu_ctx, dev, sets)
    for form, outcome in got.items():
        print(f"{form}: {outcome}")
    assert got == NO_ROWS
