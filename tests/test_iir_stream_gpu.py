"""IIR streams on the device (grail_iir_stream_*): for any split of the rows' samples into calls, the calls' outputs put end
to end and then the tail are grail_iir_async's row, bit for bit, and the calls' non-finite counts sum to its count.  65 rows
of 300 - 700 samples on filters of one to eight sections, split into calls of 63, 64, 65 samples, of random sizes that
differ from row to row with empty calls in between, and of 1 sample (seventy such calls, across a tile's edge at 64, then the
rest of every row in one call: a row of 700 in calls of one would be 700 launches and as many copies); finish with and without a tail, and on some rows while the others go
on; every section bound on both paths with rows paused inside a call; a row fed after its end; a set that cannot be freed
while a stream is open on it.  Every output buffer holds a canary wherever nothing may be written."""
import numpy as np
import pytest

import grail_hip as G
from iir_model import REFUSED, IirStreamModel, iir_model
from test_iir_gpu import BOUNDS, bound_of, noise, random_filter, same_samples, variant
from test_iir_host import NEGATIVE_ZEROS
from test_levels_gpu import CANARY, Dev, dev  # noqa: F401  (dev is a fixture)

pytestmark = pytest.mark.gpu
ROWS = 65
GUARD = 64


def case(seed):
    """(rows, filters, which): 65 rows of 300 - 700 samples, some of them not finite, on filters of S = 1 .. 8"""
    rng = np.random.default_rng(seed)
    filters = [random_filter(S, rng) for S in range(1, 9)]
    rows = [noise(int(rng.integers(300, 701)), rng) for _ in range(ROWS)]
    rows[0], rows[64] = noise(700, rng), noise(300, rng)
    for x in rows[::5]:
        x[rng.integers(0, len(x), 4)] = (np.nan, np.inf, -np.inf, np.float32(-0.0))
    return rows, filters, [int(i) % 8 for i in rng.permutation(ROWS)]


_MODEL = {}


def whole_rows_model(seed, tail):
    """the model of the case's whole rows, computed once with the longest tail: a shorter tail's outputs are its first"""
    if seed not in _MODEL:
        rows, filters, which = case(seed)
        _MODEL[seed] = iir_model(rows, filters, which, 200)
    return [(y[:n_out - 200 + tail], n_out - 200 + tail, bad) for y, n_out, bad in _MODEL[seed]]


def one_shot(ctx, dev, iir_set, rows, which, tail):
    """grail_iir_async on the whole rows, with an out_stride that cuts nothing -> ([row's outputs], nonfinite)"""
    stride, out_stride = 704, 704 + (tail + 3) // 4 * 4
    host = np.full(len(rows) * stride, np.nan, np.float32)
    for i, x in enumerate(rows):
        host[i * stride:i * stride + len(x)] = x
    d_out = dev.alloc(len(rows) * out_stride * 4)
    out_len, bad = ctx.iir(iir_set, dev.up(host), stride, dev.up(np.array([len(x) for x in rows], np.uint32)), len(rows),
                           dev.up(np.array(which, np.uint32)), tail, d_out, out_stride)
    out = dev.down(d_out, (len(rows), out_stride), np.float32)
    assert out_len.tolist() == [len(x) + tail for x in rows]
    return [out[i, :out_len[i]] for i in range(len(rows))], bad


class Feeder:
    """a stream's device buffers, written again for every call: the inputs lie in NaN, the outputs in the canary"""

    def __init__(self, ctx, dev, stream, n_rows, in_stride, out_stride, in_offset=0, out_offset=0):
        self.ctx, self.stream, self.n_rows, self.in_stride, self.out_stride = ctx, stream, n_rows, in_stride, out_stride
        self.in_offset, self.before = in_offset, GUARD + out_offset
        self.d_in = dev.alloc((n_rows * in_stride + in_offset) * 4)
        self.d_len = dev.alloc(n_rows * 4)
        self.n_out = self.before + n_rows * out_stride + GUARD
        self.d_out = dev.alloc(self.n_out * 4)
        self.dev = dev

    def _out(self):
        import ctypes as C
        canary = np.full(self.n_out, CANARY, np.float32)
        self.ctx.h2d(self.d_out, canary, canary.nbytes)
        return C.c_void_p(self.d_out.value + self.before * 4)

    def _read(self, out_len):
        out = self.dev.down(self.d_out, self.n_out, np.float32)
        assert np.all(out[:self.before] == CANARY) and np.all(out[self.before + self.n_rows * self.out_stride:] == CANARY)
        out = out[self.before:self.before + self.n_rows * self.out_stride].reshape(self.n_rows, self.out_stride)
        got = []
        for r in range(self.n_rows):
            n = 0 if out_len[r] == REFUSED else int(out_len[r])
            assert np.all(out[r, n:] == CANARY), (r, n, "written past the row's outputs")
            got.append(out[r, :n].copy())
        return got

    def next(self, chunks):
        import ctypes as C
        host = np.full(self.n_rows * self.in_stride + self.in_offset, np.nan, np.float32)
        for r, x in enumerate(chunks):
            host[self.in_offset + r * self.in_stride:self.in_offset + r * self.in_stride + len(x)] = x
        self.ctx.h2d(self.d_in, host, host.nbytes)
        lens = np.array([len(x) for x in chunks], np.uint32)
        self.ctx.h2d(self.d_len, lens, lens.nbytes)
        out_len, bad = self.ctx.iir_stream_next(self.stream, self.n_rows, C.c_void_p(self.d_in.value + self.in_offset * 4),
                                                self.in_stride, self.d_len, self._out(), self.out_stride)
        return self._read(out_len), out_len, bad

    def finish(self, which=None):
        out_len = self.ctx.iir_stream_finish(self.stream, self.n_rows, self._out(), self.out_stride, which)
        return self._read(out_len), out_len


def splits(kind, rows, rng):
    """[call][row] -> how many samples the call feeds the row"""
    left = np.array([len(x) for x in rows])
    calls = []
    while left.any():
        if kind == "random":
            n = np.where(rng.random(len(rows)) < 0.3, 0, rng.integers(0, 200, len(rows)))
        elif kind == 1:
            n = np.full(len(rows), 1 if len(calls) < 70 else 700)        # (seventy calls of one sample, then the rest at once)
        else:
            n = np.full(len(rows), kind)
        n = np.minimum(n, left)
        calls.append(n)
        if kind == "random" and len(calls) % 3 == 0:
            calls.append(np.zeros(len(rows), np.int64))                     # a call that feeds nobody
        left = left - n
    return calls


def feed(feeder, rows, calls, fed=None):
    """the calls' outputs per row, and the counts' sums"""
    fed = np.zeros(len(rows), np.int64) if fed is None else fed
    outs, bads = [[] for _ in rows], np.zeros(len(rows), np.int64)
    for n in calls:
        got, out_len, bad = feeder.next([rows[r][fed[r]:fed[r] + n[r]] for r in range(len(rows))])
        assert out_len.tolist() == n.tolist()
        for r in range(len(rows)):
            outs[r].append(got[r])
        bads += bad
        fed += n
    return outs, bads


@pytest.mark.parametrize("kind,tail", [(1, 200), (63, 0), (64, 200), (65, 0), ("random", 200), ("random", 0)])
def test_any_split_gives_the_one_shot_rows(gpu_ctx, dev, kind, tail):
    rows, filters, which = case(31)
    rng = np.random.default_rng((kind if kind != "random" else 999) + tail)
    iir_set = gpu_ctx.iir_create(filters)
    stream = gpu_ctx.iir_stream_open(iir_set, ROWS, which, tail)
    try:
        whole, whole_bad = one_shot(gpu_ctx, dev, iir_set, rows, which, tail)
        model = whole_rows_model(31, tail)
        # (the random split also on the scalar path: a base off 16-byte alignment and odd strides)
        odd = dict(in_offset=1, out_offset=3) if kind == "random" else {}
        feeder = Feeder(gpu_ctx, dev, stream, ROWS, 701 if odd else 704, 703 if odd else 704, **odd)
        outs, bads = feed(feeder, rows, splits(kind, rows, rng))
        tails, tail_len = feeder.finish()
        assert tail_len.tolist() == [tail] * ROWS
        for r in range(ROWS):
            got = np.concatenate(outs[r] + [tails[r]])
            assert len(got) == len(rows[r]) + tail == model[r][1]
            same_samples(got, whole[r], (kind, tail, r, "against grail_iir_async"))
            same_samples(got, model[r][0], (kind, tail, r, "against the model"))
        assert bads.tolist() == whole_bad.tolist() == [m[2] for m in model] and bads.sum() > 0
    finally:
        gpu_ctx.iir_stream_close(stream)
        gpu_ctx.iir_free(iir_set)


def test_finish_on_some_rows_a_row_fed_after_its_end_and_teardown(gpu_ctx, dev):
    rows, filters, which = case(32)
    tail = 37
    rng = np.random.default_rng(33)
    iir_set = gpu_ctx.iir_create(filters[:2])                               # (a set of at most two sections: another instantiation)
    which = [w % 2 for w in which]
    stream = gpu_ctx.iir_stream_open(iir_set, ROWS, which, tail)
    model = IirStreamModel(filters[:2], which, tail)
    try:
        feeder = Feeder(gpu_ctx, dev, stream, ROWS, 704, 704)
        fed = np.zeros(ROWS, np.int64)
        first = [np.full(ROWS, k) for k in (100, 100, 50)]                   # 250 samples of every row in three calls
        outs, bads = feed(feeder, rows, first, fed)
        want = model.next([x[:250] for x in rows])                          # (the model is fed them in one piece)
        # some rows end here
        marks = (np.arange(ROWS) % 4 == 1) | (np.arange(ROWS) == 7)
        tails, tail_len = feeder.finish(marks.astype(np.uint8))
        want_tails = model.finish(marks)
        assert tail_len.tolist() == [tail if m else 0 for m in marks]
        for r in range(ROWS):
            same_samples(np.concatenate(outs[r]), want[r][0], (r, "before the finish"))
            same_samples(tails[r], want_tails[r], (r, "the tails of the marked rows"))
        # the others go on; the ended rows are fed nothing, but for rows 1 and 5, which are refused: nothing written, and
        # their state as it was (a second finish gives them no second tail).  The refused rows' neighbours in the same wave
        # (rows 0, 2, 4, 6 ...) are fed in this very call and finished below, and are held to the model sample by sample:
        # a refusal that touched a state next to its own would show there
        chunks = [rows[r][250:] if not marks[r] or r in (1, 5) else np.zeros(0, np.float32) for r in range(ROWS)]
        got, out_len, bad = feeder.next(chunks)
        want = model.next(chunks)
        for r in range(ROWS):
            assert (out_len[r], bad[r]) == (want[r][1], want[r][2]), r
            assert (out_len[r] == REFUSED) == (r in (1, 5))
            if r not in (1, 5):
                same_samples(got[r], want[r][0], (r, "after the finish"))
        tails, tail_len = feeder.finish(None)
        want_tails = model.finish(None)
        assert tail_len.tolist() == [0 if m else tail for m in marks]
        for r in range(ROWS):
            same_samples(tails[r], want_tails[r], (r, "the tails of the rest"))
        # every row has ended: feeding any of them is refused, an empty call is not
        got, out_len, bad = feeder.next([x[:1] for x in rows])
        assert out_len.tolist() == [REFUSED] * ROWS and bad.tolist() == [0] * ROWS
        got, out_len, bad = feeder.next([x[:0] for x in rows])
        assert out_len.tolist() == [0] * ROWS
        # a set with an open stream cannot be freed; closed, it can
        with pytest.raises(G.GrailError) as ei:
            gpu_ctx.iir_free(iir_set)
        assert ei.value.status == G.ERR_INVALID_ARG and "open IIR streams" in str(ei.value)
    finally:
        gpu_ctx.iir_stream_close(stream)
    with pytest.raises(G.GrailError):
        gpu_ctx.iir_stream_close(stream)                                    # (looked up, not looked into: it is gone)
    gpu_ctx.iir_free(iir_set)
    with pytest.raises(G.GrailError):
        gpu_ctx.iir_free(iir_set)


def test_a_row_fed_nothing_has_no_tail_and_a_stream_without_a_tail_writes_none(gpu_ctx, dev):
    rng = np.random.default_rng(34)
    filters = [random_filter(4, rng)]
    rows = [noise(100, rng), np.zeros(0, np.float32), noise(64, rng)]
    iir_set = gpu_ctx.iir_create(filters)
    try:
        for tail in (9, 0):
            stream = gpu_ctx.iir_stream_open(iir_set, 3, None, tail)
            feeder = Feeder(gpu_ctx, dev, stream, 3, 128, 128)
            got, out_len, bad = feeder.next(rows)
            tails, tail_len = feeder.finish()
            want = iir_model(rows, filters, None, tail)
            assert tail_len.tolist() == [tail, 0, tail] and [w[1] for w in want] == [100 + tail, 0, 64 + tail]
            for r in range(3):
                same_samples(np.concatenate([got[r], tails[r]]), want[r][0], (tail, r))
            gpu_ctx.iir_stream_close(stream)
    finally:
        gpu_ctx.iir_free(iir_set)


# ---- every section bound on both paths ------------------------------------------------------------------------------------------
BOUND_SECTIONS = {1: (1, 1, 1), 2: (2, 1, 2), 4: (4, 3, 1), 8: (8, 5, 2)}        # a set's filters, by its largest's sections
BOUND_LAYOUTS = {"aligned": dict(in_stride=208, out_stride=208), "offset-odd": dict(in_stride=201, out_stride=203, in_offset=1, out_offset=3)}
BOUND_TAIL = 37
MINUS_ROW = 9                                                                     # bound 1: a row of -0.0 through NEGATIVE_ZEROS


def bound_case(most):
    """(rows, filters, which): 65 rows of 60 - 200 samples (a whole wave and a wave of one row), some samples not finite, on a
    set whose largest filter has `most` sections; at bound 1 a section that answers silence with -0.0, fed a row of -0.0"""
    rng = np.random.default_rng(50 + most)
    filters = [random_filter(S, rng) for S in BOUND_SECTIONS[most]]
    rows = [noise(int(rng.integers(60, 201)), rng) for _ in range(ROWS)]
    rows[0], rows[64] = noise(200, rng), noise(60, rng)
    for x in rows[::6]:
        x[rng.integers(0, len(x), 4)] = (np.nan, np.inf, -np.inf, np.float32(-0.0))
    which = [int(f) for f in rng.integers(0, len(filters), ROWS)]
    which[0] = 0                                                                  # (the largest filter is in use)
    if most == 1:
        filters.append(np.array([NEGATIVE_ZEROS]))
        rows[MINUS_ROW], which[MINUS_ROW] = np.full(70, -0.0, np.float32), len(filters) - 1
    return rows, filters, which


def bound_calls(rows):
    """[call][row]: 63 samples (every seventh row paused: its lane keeps its state while the wave runs 63 steps), 1 sample, the
    rest (every fifth row paused while its neighbours run whole tiles), then the rest of those"""
    left = np.array([len(x) for x in rows])
    r = np.arange(len(rows))
    calls = []
    for n in (np.where(r % 7 == 3, 0, 63), np.full(len(rows), 1), np.where(r % 5 == 2, 0, 1000), np.full(len(rows), 1000)):
        calls.append(np.minimum(n, left))
        left = left - calls[-1]
    assert not left.any() and (calls[2][r % 5 != 2] - 64).max() > 64 and calls[3].max() > 64
    return calls


@pytest.mark.parametrize("layout", sorted(BOUND_LAYOUTS))
@pytest.mark.parametrize("most", BOUNDS)
def test_every_section_bound_on_both_paths(gpu_ctx, dev, most, layout):
    """iir_kernel<most, VEC, true> for both VEC, in `next` and in `finish`: call by call against IirStreamModel, and the calls
    put end to end against grail_iir_async.  Some rows are finished by marks while the others are not, then the rest."""
    rows, filters, which = bound_case(most)
    kw = BOUND_LAYOUTS[layout]
    vec = layout == "aligned"
    assert bound_of(filters) == most
    assert variant(most, kw.get("in_offset", 0), kw["in_stride"], kw.get("out_offset", 0), kw["out_stride"], True) == (most, vec, True)
    assert variant(most, 0, 0, kw.get("out_offset", 0), kw["out_stride"], True) == (most, vec, True)            # the finishing calls
    iir_set = gpu_ctx.iir_create(filters)
    stream = gpu_ctx.iir_stream_open(iir_set, ROWS, which, BOUND_TAIL)
    model = IirStreamModel(filters, which, BOUND_TAIL)
    try:
        whole, whole_bad = one_shot(gpu_ctx, dev, iir_set, rows, which, BOUND_TAIL)
        feeder = Feeder(gpu_ctx, dev, stream, ROWS, **kw)
        fed = np.zeros(ROWS, np.int64)
        pieces, bads = [[] for _ in rows], np.zeros(ROWS, np.int64)
        for c, n in enumerate(bound_calls(rows)):
            chunks = [rows[r][fed[r]:fed[r] + n[r]] for r in range(ROWS)]
            got, out_len, bad = feeder.next(chunks)
            want = model.next(chunks)
            for r in range(ROWS):
                assert (out_len[r], bad[r]) == (want[r][1], want[r][2]) and out_len[r] == n[r], (c, r)
                same_samples(got[r], want[r][0], (most, layout, c, r, "against the model"))
                pieces[r].append(got[r])
            bads += bad
            fed += n
        marks = np.arange(ROWS) % 3 == 0
        for which_rows in (marks.astype(np.uint8), None):
            tails, tail_len = feeder.finish(which_rows)
            want_tails = model.finish(None if which_rows is None else marks)
            takes = marks if which_rows is not None else ~marks
            assert tail_len.tolist() == [BOUND_TAIL if m else 0 for m in takes]
            for r in range(ROWS):
                same_samples(tails[r], want_tails[r], (most, layout, r, "the tail against the model"))
                pieces[r].append(tails[r])
        for r in range(ROWS):
            same_samples(np.concatenate(pieces[r]), whole[r], (most, layout, r, "against grail_iir_async"))
        assert bads.tolist() == whole_bad.tolist() and bads.sum() > 0
        if most == 1:
            # what the row of -0.0 is there for: b0 = -1 answers -0.0 with +0.0, which is what leaves; the sample itself, had
            # the select kept it, is -0.0 (and the tail, on +0.0, answers +0.0, +0.0, -0.0 in turn, as the rows' call on silence)
            y = np.concatenate(pieces[MINUS_ROW])
            assert np.all(y[:70].view(np.uint32) == 0) and np.signbit(y[70:76]).tolist() == [False, False, True] * 2
    finally:
        gpu_ctx.iir_stream_close(stream)
        gpu_ctx.iir_free(iir_set)


def test_interactive_example_equalises_what_it_writes(gpu_ctx, dev):
    """grail_interactive --eq ... writes, to the last bit, what grail_iir_async gives for the samples the same session writes
    without --eq, through the sections grail_iir_design makes at the rate that is written, rung out for a tenth of a second:
    the pulls of 441 samples and the tails of the other stages are the stream's calls."""
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "grail-rs_amd", "lib", "grail_interactive")
    chain, script = ["--band", "300", "3400", "--rate", "8000"], b"a e\n@0.3 o i a e\n"
    eq = ["--eq", "highpass:100:0.707", "--eq", "peak:1500:1.5:4.5", "--eq", "highshelf:3000:0.7:-3"]
    plain = subprocess.run([exe] + chain + ["441", "0.4"], input=script, capture_output=True, timeout=120)
    r = subprocess.run([exe] + chain + eq + ["441", "0.4"], input=script, capture_output=True, timeout=120)
    assert plain.returncode == 0 and r.returncode == 0, (plain.stderr, r.stderr)
    before, after = np.frombuffer(plain.stdout, np.float32), np.frombuffer(r.stdout, np.float32)
    assert len(before) > 4000 and len(after) == len(before) + 800
    assert b"Equalised at 8000 Hz, highpass:100:0.707 peak:1500:1.5:4.5 highshelf:3000:0.7:-3: %d samples written" % len(after) in r.stderr
    sections = [G.iir_design(G.IIR_HIGHPASS, 8000, 100.0, 0.707), G.iir_design(G.IIR_PEAK, 8000, 1500.0, 1.5, 4.5),
                G.iir_design(G.IIR_HIGHSHELF, 8000, 3000.0, 0.7, -3.0)]
    iir_set = gpu_ctx.iir_create([np.array(sections)])
    try:
        stride = (len(after) + 63) // 64 * 64
        host = np.zeros(stride, np.float32)
        host[:len(before)] = before
        d_out = dev.alloc(stride * 4)
        out_len, bad = gpu_ctx.iir(iir_set, dev.up(host), stride, dev.up(np.array([len(before)], np.uint32)), 1, None, 800, d_out, stride)
        assert out_len.tolist() == [len(after)] and bad.tolist() == [0]
        same_samples(after, dev.down(d_out, stride, np.float32)[:len(after)], "grail_interactive --eq")
        assert not np.array_equal(after[:len(before)], before)
    finally:
        gpu_ctx.iir_free(iir_set)
