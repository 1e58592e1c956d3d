"""Dynamics streams on the device (grail_dyn_stream_*) against grail_dyn_async on the whole rows, bit for bit: 70 rows (a whole
wave and a partial one) on three curves, fed in calls of 1, 63, 64, 65, 0 and 300 samples with the rows advancing by different
amounts in one call (some paused, some ended early), self-keyed and keyed (two rows on one key among them).  The outputs of
the calls put end to end are the one-shot rows, the calls' non-finite counts add up to its count, the smallest of the calls'
min_gain among those that fed the row something is its min_gain, and a call that feeds a row nothing reads 1.0.  Both are held to the numpy model as well.  Then the
paths that case leaves out: a stream opened where one was just closed, the lookup's edges and alphas of 0 from call to call, an
in_len above in_stride and an out_stride above it, a key misaligned alone, streams and one-shot calls queued with their inputs
overwritten, and a row fed across the tiles of grail_track_dyn_async.  Then what
only a live stream can be asked: a set with an open stream refuses grail_dyn_free, close then free succeeds, and the calls a
keyed or self-keyed stream refuses."""
import ctypes as C

import numpy as np
import pytest

import dyn_model as M
import grail_hip as G
from test_dyn_gpu import audio, edge_curves, edge_samples, run, same, same_bits, three_curves, variant
from test_track_dyn_gpu import T, run as track_run
from test_levels_gpu import CANARY, Dev, dev  # noqa: F401  (dev is a fixture)

pytestmark = pytest.mark.gpu
N_ROWS = 70
STEPS = (1, 63, 64, 65, 0, 300)
GUARD = 64                                                      # floats of canary before and after every out buffer


def corpus(keyed):
    rng = np.random.default_rng(21 + keyed)
    n = [int(v) for v in rng.integers(0, 494, N_ROWS)]
    n[0], n[1], n[2], n[69] = 493, 0, 64, 493                  # (1 + 63 + 64 + 65 + 0 + 300 = 493: the longest a row can be)
    rows = [audio(k, rng) for k in n]
    rows[0][[5, 200]] = (np.nan, np.inf)
    which = [int(v) for v in rng.integers(0, 3, N_ROWS)]
    if not keyed:
        return rows, which, None, None
    # 69 keys: rows 0 and 69, equally long and fed alike, listen to key 0 (the rows on one key advance together: a call's key
    # is read from where the rows it drives stand); every other row has a key of its own
    key_row = [0] + [int(v) for v in rng.permutation(np.arange(1, N_ROWS - 1))] + [0]
    keys = [audio(493, rng) for _ in range(N_ROWS - 1)]
    keys[0][7] = np.nan
    return rows, which, keys, key_row


def chunking_calls(n):
    """[(feed [row], stride)] of the calls below for rows of n[r] samples: the rows advance by different amounts (every third
    row lags a call behind with half a step), the last call feeds the rest (at most 300 + what lagging left), and the strides
    are of every residue mod 4: both paths"""
    at, calls = [0] * len(n), []
    for call, step in enumerate(STEPS):
        feed = [min(step if (r + call) % 3 else step // 2, n[r] - at[r]) for r in range(len(n))]
        if call == len(STEPS) - 1:
            feed = [n[r] - at[r] for r in range(len(n))]
        calls.append((feed, max(max(feed), 1) + call))
        at = [a + f for a, f in zip(at, feed)]
    return calls


@pytest.mark.parametrize("keyed", [False, True], ids=["self-keyed", "keyed"])
def test_any_chunking_gives_the_one_shot_rows(gpu_ctx, dev, keyed):
    rows, which, keys, key_row = corpus(keyed)
    n = [len(x) for x in rows]
    curves = three_curves()
    dyn_set = gpu_ctx.dyn_create(curves)
    # the one shot: on the device and in the model (a stream's key is as long as the row it drives)
    key_lens = None if not keyed else [n[key_row.index(k)] for k in range(N_ROWS - 1)]
    want = M.dyn_model(rows, curves, which, keys=keys, key_row=key_row, key_lens=key_lens)
    whole = run(gpu_ctx, dev, dyn_set, rows, which, keys=keys, key_row=key_row, key_lens=key_lens)
    same(want, whole, "one shot")
    st = gpu_ctx.dyn_stream_open(dyn_set, N_ROWS, which, N_ROWS - 1 if keyed else 0, key_row)
    with pytest.raises(G.GrailError):                           # the set has an open stream
        gpu_ctx.dyn_free(dyn_set)
    at = [0] * N_ROWS
    pieces = [[] for _ in range(N_ROWS)]
    bad = np.zeros(N_ROWS, np.int64)
    mg = np.full(N_ROWS, np.inf)
    for call, (feed, stride) in enumerate(chunking_calls(n)):
        assert feed[69] == feed[0]                              # (the two rows on one key are fed alike)
        host = np.full(N_ROWS * stride, np.nan, np.float32)
        for r in range(N_ROWS):
            host[r * stride:r * stride + feed[r]] = rows[r][at[r]:at[r] + feed[r]]
        d_in, d_len = dev.up(host), dev.up(np.array(feed, np.uint32))
        d_out = dev.up(np.full(GUARD + N_ROWS * stride + GUARD, CANARY, np.float32))
        kw = {}
        if keyed:
            khost = np.full((N_ROWS - 1) * stride, np.nan, np.float32)
            for r in range(N_ROWS):
                khost[key_row[r] * stride:key_row[r] * stride + feed[r]] = keys[key_row[r]][at[r]:at[r] + feed[r]]
            kw = dict(key_dev=dev.up(khost), key_stride=stride)
        out_len, nonfinite, gain = gpu_ctx.dyn_stream_next(st, N_ROWS, d_in, stride, d_len, C.c_void_p(d_out.value + GUARD * 4), stride, **kw)
        out = dev.down(d_out, GUARD + N_ROWS * stride + GUARD, np.float32)
        assert np.all(out[:GUARD] == CANARY) and np.all(out[GUARD + N_ROWS * stride:] == CANARY), (call, "written outside out")
        out = out[GUARD:GUARD + N_ROWS * stride].reshape(N_ROWS, stride)
        for r in range(N_ROWS):
            assert out_len[r] == feed[r], (call, r)
            assert np.all(out[r, feed[r]:] == CANARY), (call, r, "written past the row's outputs")
            assert feed[r] or gain[r] == 1.0, (call, r)
            pieces[r].append(out[r, :feed[r]])
            at[r] += feed[r]
        bad += nonfinite
        mg = np.where(np.array(feed) > 0, np.minimum(mg, gain), mg)      # (over the calls that fed the row something)
    for r in range(N_ROWS):
        y = np.concatenate(pieces[r])
        assert len(y) == n[r] == whole[1][r]
        same_bits(y, whole[0][r, :n[r]], ("stream", r))
        assert bad[r] == whole[2][r] and np.float64(mg[r] if n[r] else 1.0).view(np.uint64) == np.float64(whole[3][r]).view(np.uint64), r
    assert whole[2][0] == 2
    gpu_ctx.dyn_stream_close(st)
    gpu_ctx.dyn_free(dyn_set)                                   # close, then free


class Feeder:
    """a stream's device buffers, allocated once and written again for every call: the inputs (and a keyed stream's keys) lie
    in NaN, the outputs in the canary, with GUARD floats of it before and after"""

    def __init__(self, ctx, dev, st, n_rows, in_stride, out_stride, in_offset=0, out_offset=0, n_keys=0, key_stride=0, key_offset=0):
        self.ctx, self.dev, self.st, self.n_rows, self.n_keys = ctx, dev, st, n_rows, n_keys
        self.in_stride, self.out_stride, self.key_stride = in_stride, out_stride, key_stride
        self.in_offset, self.key_offset, self.before = in_offset, key_offset, GUARD + out_offset
        self.layout = (in_offset, in_stride, out_offset, out_stride, n_keys != 0, key_offset, key_stride)
        self.d_in = dev.alloc((n_rows * in_stride + in_offset) * 4)
        self.d_key = dev.alloc((n_keys * key_stride + key_offset) * 4) if n_keys else None
        self.d_len = dev.alloc(n_rows * 4)
        self.n_out = self.before + n_rows * out_stride + GUARD
        self.d_out = dev.alloc(self.n_out * 4)

    def _fill(self, d_buf, rows, stride, offset):
        host = np.full(len(rows) * stride + offset, np.nan, np.float32)
        for r, x in enumerate(rows):
            host[offset + r * stride:offset + r * stride + len(x)] = x
        self.ctx.h2d(d_buf, host, host.nbytes)
        return C.c_void_p(d_buf.value + offset * 4)

    def next(self, chunks, keys=None, lens=None):
        """chunks[r]: the samples row r is fed (lens: what in_len_dev holds, where it is not their count); keys[j]: the call's
        key j -> ([row r's outputs], out_len, nonfinite, min_gain), the canary checked everywhere else"""
        in_dev = self._fill(self.d_in, chunks, self.in_stride, self.in_offset)
        lens = np.array([len(x) for x in chunks] if lens is None else lens, np.uint32)
        self.ctx.h2d(self.d_len, lens, lens.nbytes)
        canary = np.full(self.n_out, CANARY, np.float32)
        self.ctx.h2d(self.d_out, canary, canary.nbytes)
        kw = {}
        if self.n_keys:
            kw = dict(key_dev=self._fill(self.d_key, keys, self.key_stride, self.key_offset), key_stride=self.key_stride)
        out_len, bad, gain = self.ctx.dyn_stream_next(self.st, self.n_rows, in_dev, self.in_stride, self.d_len,
                                                      C.c_void_p(self.d_out.value + self.before * 4), self.out_stride, **kw)
        out = self.dev.down(self.d_out, self.n_out, np.float32)
        assert np.all(out[:self.before] == CANARY) and np.all(out[self.before + self.n_rows * self.out_stride:] == CANARY), "written outside out"
        out = out[self.before:self.before + self.n_rows * self.out_stride].reshape(self.n_rows, self.out_stride)
        got = []
        for r in range(self.n_rows):
            assert out_len[r] == len(chunks[r]), (r, out_len[r], len(chunks[r]))
            assert np.all(out[r, out_len[r]:] == CANARY), (r, "written past the row's outputs")
            got.append(out[r, :out_len[r]].copy())
        return got, out_len, bad, gain


def feed_in_calls(feeder, rows, sizes, keys=None):
    """the rows (all as long as the sizes' sum, but a row shorter than it ends early) fed in calls of `sizes` samples, key j cut
    as the rows that listen to it -> ([row's outputs put end to end], the counts' sums, the smallest min_gain among the calls
    that fed the row something: the header's rule for a row's min_gain over a stream)"""
    pieces, bads, mg = [[] for _ in rows], np.zeros(len(rows), np.int64), np.full(len(rows), np.inf)
    at = 0
    for size in sizes:
        chunks = [x[at:at + size] for x in rows]
        got, out_len, bad, gain = feeder.next(chunks, keys=None if keys is None else [k[at:at + size] for k in keys])
        for r in range(len(rows)):
            assert len(chunks[r]) or gain[r] == 1.0, (at, r)
            pieces[r].append(got[r])
        bads += bad
        mg = np.where(np.array([len(x) for x in chunks]) > 0, np.minimum(mg, gain), mg)
        at += size
    assert at >= max(len(x) for x in rows)
    return [np.concatenate(p) for p in pieces], bads, mg


def same_as_one_shot(want, whole, streamed, what):
    """the model's rows, the one-shot call's (out, out_len, nonfinite, min_gain) and feed_in_calls' answer: all the same bits"""
    same(want, whole, (what, "one shot"))
    ys, bads, mg = streamed
    for r, (y, n, w_bad, w_mg) in enumerate(want):
        assert len(ys[r]) == n and bads[r] == w_bad, (what, r)
        same_bits(ys[r], y, (what, r, "against the model"))
        same_bits(ys[r], whole[0][r, :n], (what, r, "against grail_dyn_async"))
        assert np.float64(mg[r] if n else 1.0).view(np.uint64) == np.float64(w_mg).view(np.uint64) == np.float64(whole[3][r]).view(np.uint64), (what, r)


# ---- (a) a stream opened over the state of one just closed --------------------------------------------------------------------
def test_a_stream_opened_where_one_was_just_closed_starts_from_rest(gpu_ctx, dev):
    """a stream is opened, fed a loud call and closed with that call still queued; at once a stream of the same shape is opened
    (a device allocator that hands the first one's block back must not hand back its envelopes) and fed quiet rows: they are
    the one-shot rows from e = +0.0"""
    rng = np.random.default_rng(61)
    curves = three_curves()
    which = [r % 3 for r in range(N_ROWS)]
    loud = [(rng.uniform(0.5, 1.0, 256) * rng.choice([-1.0, 1.0], 256)).astype(np.float32) for _ in range(N_ROWS)]
    quiet = [audio(int(rng.integers(1, 200)), rng) for _ in range(N_ROWS)]
    want = M.dyn_model(quiet, curves, which)
    # (what the case is there for, in the model: from the loud call's envelopes the quiet rows come out otherwise)
    carried = M.DynStreamModel(curves, which)
    carried.next(loud)
    assert sum(not np.array_equal(c[0].view(np.uint32), w[0].view(np.uint32)) for c, w in zip(carried.next(quiet), want)) > N_ROWS // 2
    dyn_set = gpu_ctx.dyn_create(curves)
    try:
        whole = run(gpu_ctx, dev, dyn_set, quiet, which)
        d_loud, d_len = dev.up(np.concatenate(loud)), dev.up(np.full(N_ROWS, 256, np.uint32))
        d_out = dev.alloc(N_ROWS * 256 * 4)
        first = gpu_ctx.dyn_stream_open(dyn_set, N_ROWS, which)
        gpu_ctx.dyn_stream_next_async(first, d_loud, 256, d_len, d_out, 256)
        gpu_ctx.dyn_stream_close(first)
        second = gpu_ctx.dyn_stream_open(dyn_set, N_ROWS, which)
        try:
            feeder = Feeder(gpu_ctx, dev, second, N_ROWS, 200, 200)
            same_as_one_shot(want, whole, feed_in_calls(feeder, quiet, [200]), "a stream after a stream")
        finally:
            gpu_ctx.dyn_stream_close(second)
    finally:
        gpu_ctx.dyn_free(dyn_set)


# ---- (b) the lookup's edges from call to call -----------------------------------------------------------------------------------
def edge_calls(n):
    """calls of 1, 2, ... 64 samples in turn until n are fed: the first cycle's calls begin at the triangular numbers 0, 1, 3, 6
    ... 2 016, which are every residue mod 64 once"""
    sizes = []
    while sum(sizes) < n:
        sizes.append(min(len(sizes) % 64 + 1, n - sum(sizes)))
    starts = np.cumsum([0] + sizes[:-1])
    assert {int(s) % 64 for s in starts} == set(range(64)) and set(sizes[:64]) == set(range(1, 65))
    return sizes


def test_the_lookups_edges_from_call_to_call(gpu_ctx, dev):
    """test_dyn_gpu's edge samples through streams on its four settings (two with alphas of 0, one whose release rides below
    2^-32 for many samples), in calls of 1 to 64 samples in turn, so that every position mod 64 (of a tile, and of the four-way
    unrolled loop and its remainder) is a call's first sample once: e is saved to the state and restored from it at every one
    of those, on either side of the lookup's lower edge"""
    x = edge_samples()
    rng = np.random.default_rng(12)
    curves = edge_curves()
    # a row made for the expander's release (alpha 0.5, attack at once): 2^-20 every 97 samples and silence behind it, so e
    # halves its way through 2^-32 twelve samples later and on down, and 2^-40, below the table, on the way
    ride = np.zeros(len(x), np.float32)
    ride[::97], ride[50::97] = np.float32(2.0 ** -20), np.float32(-2.0 ** -40)
    rows = [x, x, x, x, rng.permutation(x), rng.permutation(x), ride]
    which = [0, 1, 2, 3, 0, 1, 2]
    want = M.dyn_model(rows, curves, which)
    # (it does ride below 2^-32 from call to call: the model's envelope of that row at the calls' ends)
    low = M.DynStreamModel(curves, [2])
    below, at = 0, 0
    for size in edge_calls(len(x)):
        low.next([ride[at:at + size]])
        below += bool(0.0 < low.e[0] < 2.0 ** -32)
        at += size
    assert below > 30
    dyn_set = gpu_ctx.dyn_create(curves)
    st = gpu_ctx.dyn_stream_open(dyn_set, len(rows), which)
    try:
        whole = run(gpu_ctx, dev, dyn_set, rows, which)
        feeder = Feeder(gpu_ctx, dev, st, len(rows), 64, 64)
        assert variant(*feeder.layout, stream=True) == (True, False, True)
        same_as_one_shot(want, whole, feed_in_calls(feeder, rows, edge_calls(len(x))), "edges")
    finally:
        gpu_ctx.dyn_stream_close(st)
        gpu_ctx.dyn_free(dyn_set)


# ---- (c) lengths above the stride, outputs wider than the inputs -------------------------------------------------------------------
@pytest.mark.parametrize("second", [dict(in_stride=64, out_stride=96), dict(in_stride=66, out_stride=99, out_offset=1)], ids=["aligned", "odd"])
def test_an_in_len_above_in_stride_is_the_stride_and_out_stride_may_be_wider(gpu_ctx, dev, second):
    """in_len_dev holds more than in_stride (5 000, 2^32 - 1): the row is fed in_stride samples, as grail_dyn_async reads a len
    beyond its stride; and out_stride above in_stride: the rows' outputs lie out_stride apart"""
    rng = np.random.default_rng(63)
    curves = three_curves()
    which = [0, 1, 2, 0, 1]
    s2 = second["in_stride"]
    lens = ([5000, 60, 0xFFFFFFFF, 100, 0], [s2, s2 + 4, 10, 0, 200])
    fed = ([100, 60, 100, 100, 0], [s2, s2, 10, 0, s2])
    rows = [audio(a + b, rng) for a, b in zip(*fed)]
    rows[0][[99, 100]] = (np.nan, np.inf)
    want = M.dyn_model(rows, curves, which)
    dyn_set = gpu_ctx.dyn_create(curves)
    st = gpu_ctx.dyn_stream_open(dyn_set, 5, which)
    try:
        whole = run(gpu_ctx, dev, dyn_set, rows, which)
        feeders = (Feeder(gpu_ctx, dev, st, 5, 100, 128), Feeder(gpu_ctx, dev, st, 5, **second))
        assert variant(*feeders[0].layout, stream=True) == (True, False, True)
        assert variant(*feeders[1].layout, stream=True) == (s2 == 64, False, True)
        pieces, bads, mg = [[] for _ in rows], np.zeros(5, np.int64), np.full(5, np.inf)
        at = [0] * 5
        for feeder, call_lens, call_fed in zip(feeders, lens, fed):
            assert call_fed == [min(n, feeder.in_stride) for n in call_lens]
            got, out_len, bad, gain = feeder.next([rows[r][at[r]:at[r] + call_fed[r]] for r in range(5)], lens=call_lens)
            for r in range(5):
                pieces[r].append(got[r])
                at[r] += call_fed[r]
            bads += bad
            mg = np.where(np.array(call_fed) > 0, np.minimum(mg, gain), mg)
        same_as_one_shot(want, whole, ([np.concatenate(p) for p in pieces], bads, mg), second)
    finally:
        gpu_ctx.dyn_stream_close(st)
        gpu_ctx.dyn_free(dyn_set)


# ---- (d) a keyed stream whose key alone is misaligned, and the converse ----------------------------------------------------------
KEY_LAYOUTS = {"aligned": (dict(in_stride=132, out_stride=136, key_stride=140), True),
               "key base": (dict(in_stride=132, out_stride=136, key_stride=140, key_offset=1), False),
               "key stride": (dict(in_stride=132, out_stride=136, key_stride=141), False),
               "rows base": (dict(in_stride=132, out_stride=136, key_stride=140, in_offset=1), False),
               "out stride": (dict(in_stride=132, out_stride=137, key_stride=140), False)}


@pytest.mark.parametrize("layout", sorted(KEY_LAYOUTS))
def test_a_keyed_stream_whose_key_alone_is_misaligned_and_the_converse(gpu_ctx, dev, layout):
    """launch_dyn's VEC asks the key too: a key one float off 16 bytes, or at an odd stride, with rows and out aligned, takes
    the 4-byte kernel, and so does an aligned key beside rows or outputs that are not; the bits are the aligned call's"""
    kw, vec = KEY_LAYOUTS[layout]
    rng = np.random.default_rng(64)
    curves = three_curves()
    which, key_row = [0, 1, 2, 0, 1], [0, 1, 2, 3, 0]                      # rows 0 and 4 on key 0, equally long
    rows = [audio(n, rng) for n in (200, 131, 64, 199, 200)]
    keys = [audio(200, rng) for _ in range(4)]
    keys[0][[3, 70]], rows[1][69] = (np.nan, np.inf), -np.inf
    key_lens = [200, 131, 64, 199]
    want = M.dyn_model(rows, curves, which, keys=keys, key_row=key_row, key_lens=key_lens)
    dyn_set = gpu_ctx.dyn_create(curves)
    st = gpu_ctx.dyn_stream_open(dyn_set, 5, which, 4, key_row)
    try:
        whole = run(gpu_ctx, dev, dyn_set, rows, which, keys=keys, key_row=key_row, key_lens=key_lens)
        feeder = Feeder(gpu_ctx, dev, st, 5, n_keys=4, **kw)
        assert variant(*feeder.layout, stream=True) == (vec, True, True)
        same_as_one_shot(want, whole, feed_in_calls(feeder, rows, [70, 130], keys=keys), layout)
    finally:
        gpu_ctx.dyn_stream_close(st)
        gpu_ctx.dyn_free(dyn_set)


# ---- (e) streams and one-shot calls queued behind one another --------------------------------------------------------------------
def test_two_streams_and_both_one_shot_calls_queued_with_their_inputs_overwritten_behind_them(gpu_ctx, dev):
    """two streams on one set (one self-keyed, one keyed), three calls each, a grail_dyn_async and a grail_track_dyn_async call
    between them, nothing waited for, every input (and key) buffer set to NaN right behind the call that read it: each call
    read its own samples, each stream's envelopes went from its own call to its next"""
    rng = np.random.default_rng(65)
    curves = three_curves()
    n, stride, calls = 100, 128, 3
    which = ([0, 1, 2], [2, 0, 1])
    key_row = [0, 1, 0]
    rows = [[audio(calls * n, rng) for _ in range(3)] for _ in range(2)]
    keys = [audio(calls * n, rng) for _ in range(2)]
    lane_rows, track_rows = [audio(k, rng) for k in (200, 65, 0, 128)], [audio(k, rng) for k in (T + 5, 300)]
    lane_rows[0][7] = rows[0][1][150] = keys[1][250] = np.nan
    models = (M.DynStreamModel(curves, which[0]), M.DynStreamModel(curves, which[1], key_row))
    want = [[models[0].next([x[c * n:(c + 1) * n] for x in rows[0]]) for c in range(calls)],
            [models[1].next([x[c * n:(c + 1) * n] for x in rows[1]], keys=[k[c * n:(c + 1) * n] for k in keys]) for c in range(calls)]]

    def placed(xs, pitch):
        host = np.full((len(xs), pitch), np.nan, np.float32)
        for i, x in enumerate(xs):
            host[i, :len(x)] = x
        return dev.up(host)

    def results(k):
        return dev.alloc(k * 4), dev.alloc(k * 4), dev.alloc(k * 8)

    # everything is uploaded and allocated before the first call
    d_len = dev.up(np.full(3, n, np.uint32))
    d_in = [[placed([x[c * n:(c + 1) * n] for x in rows[s]], stride) for c in range(calls)] for s in range(2)]
    d_key = [placed([k[c * n:(c + 1) * n] for k in keys], stride) for c in range(calls)]
    d_out = [[dev.up(np.full(3 * stride, CANARY, np.float32)) for _ in range(calls)] for _ in range(2)]
    d_res = [[results(3) for _ in range(calls)] for _ in range(2)]
    lane_stride, track_stride = 256, T + 64
    d_lane, d_lane_len = placed(lane_rows, lane_stride), dev.up(np.array([len(x) for x in lane_rows], np.uint32))
    d_track, d_track_len = placed(track_rows, track_stride), dev.up(np.array([len(x) for x in track_rows], np.uint32))
    d_lane_out, d_track_out = dev.up(np.full(4 * lane_stride, CANARY, np.float32)), dev.up(np.full(2 * track_stride, CANARY, np.float32))
    d_lane_which, d_track_which = dev.up(np.array([0, 1, 2, 1], np.uint32)), dev.up(np.array([1, 0], np.uint32))
    lane_res, track_res = results(4), results(2)
    dyn_set = gpu_ctx.dyn_create(curves)
    streams = (gpu_ctx.dyn_stream_open(dyn_set, 3, which[0]), gpu_ctx.dyn_stream_open(dyn_set, 3, which[1], 2, key_row))
    try:
        for c in range(calls):
            gpu_ctx.dyn_stream_next_async(streams[0], d_in[0][c], stride, d_len, d_out[0][c], stride, *d_res[0][c])
            gpu_ctx.memset(d_in[0][c], 0xFF, 3 * stride * 4)                          # (NaN everywhere)
            if c == 0:
                gpu_ctx.dyn_async(dyn_set, d_lane, lane_stride, d_lane_len, 4, d_lane_which, d_lane_out, lane_stride, *lane_res)
                gpu_ctx.memset(d_lane, 0xFF, 4 * lane_stride * 4)
            gpu_ctx.dyn_stream_next_async(streams[1], d_in[1][c], stride, d_len, d_out[1][c], stride, *d_res[1][c], key_dev=d_key[c],
                                          key_stride=stride)
            gpu_ctx.memset(d_in[1][c], 0xFF, 3 * stride * 4)
            gpu_ctx.memset(d_key[c], 0xFF, 2 * stride * 4)
            if c == 1:
                gpu_ctx.track_dyn_async(dyn_set, d_track, track_stride, d_track_len, 2, d_track_which, d_track_out, track_stride, *track_res)
                gpu_ctx.memset(d_track, 0xFF, 2 * track_stride * 4)
        gpu_ctx.sync()

        def down(d_o, pitch, res, k):
            return (dev.down(d_o, (k, pitch), np.float32), dev.down(res[0], k, np.uint32), dev.down(res[1], k, np.uint32),
                    dev.down(res[2], k, np.float64))
        for s in range(2):
            for c in range(calls):
                same(want[s][c], down(d_out[s][c], stride, d_res[s][c], 3), ("stream", s, "call", c))
        same(M.dyn_model(lane_rows, curves, [0, 1, 2, 1]), down(d_lane_out, lane_stride, lane_res, 4), "grail_dyn_async in between")
        same(M.dyn_model(track_rows, curves, [1, 0]), down(d_track_out, track_stride, track_res, 2), "grail_track_dyn_async in between")
    finally:
        for st in streams:
            gpu_ctx.dyn_stream_close(st)
        gpu_ctx.dyn_free(dyn_set)


# ---- (f) a long row across the tiles of the workgroup-a-row call -------------------------------------------------------------------
def test_a_row_fed_across_the_track_calls_tiles_is_the_track_calls_row(gpu_ctx, dev):
    """5 TRACK_TILE + 1 samples fed in calls that end inside a tile, on a tile's edge and one sample past one: the calls put end to
    end, their counts and their smallest min_gain are grail_track_dyn_async's on the whole row, keyed and not"""
    rng = np.random.default_rng(66)
    curves = three_curves()
    n = 5 * T + 1
    sizes = [T - 24, 24, T + 1, 2 * T - 1, T + 1]
    ends = np.cumsum(sizes)
    assert ends[-1] == n and [int(e) % T for e in ends] == [T - 24, 0, 1, 0, 1]
    rows = [audio(n, rng), audio(n, rng)]
    keys = [audio(n, rng)]
    rows[0][[T - 1, T, 3 * T + 7]], keys[0][2 * T] = (np.nan, np.inf, -np.inf), np.nan
    which = [0, 1]
    dyn_set = gpu_ctx.dyn_create(curves)
    try:
        for keyed in (False, True):
            kw = dict(keys=keys, key_row=[0, 0], key_lens=[n]) if keyed else {}
            track = track_run(gpu_ctx, dev, dyn_set, rows, which, **kw)
            assert track[1].tolist() == [n, n] and track[2].tolist() == [3, 0]
            st = gpu_ctx.dyn_stream_open(dyn_set, 2, which, 1 if keyed else 0, [0, 0] if keyed else None)
            try:
                feeder = Feeder(gpu_ctx, dev, st, 2, 2 * T, 2 * T, n_keys=1 if keyed else 0, key_stride=2 * T)
                ys, bads, mg = feed_in_calls(feeder, rows, sizes, keys=keys if keyed else None)
                for r in range(2):
                    same_bits(ys[r], track[0][r, :n], (keyed, r))
                    assert bads[r] == track[2][r] and np.float64(mg[r]).view(np.uint64) == np.float64(track[3][r]).view(np.uint64), (keyed, r)
            finally:
                gpu_ctx.dyn_stream_close(st)
    finally:
        gpu_ctx.dyn_free(dyn_set)


def test_what_a_live_stream_refuses(gpu_ctx, dev):
    lib = G.load()
    curves = three_curves()
    dyn_set = gpu_ctx.dyn_create(curves)
    for args in [(0, None, 0, None), (2, [0, 3], 0, None), (2, None, 1, None), (2, None, 2, [0, 2])]:
        n_rows, which, n_keys, key_rows = args
        with pytest.raises(G.GrailError):
            gpu_ctx.dyn_stream_open(dyn_set, n_rows, which, n_keys, key_rows)
    plain = gpu_ctx.dyn_stream_open(dyn_set, 2)
    keyed = gpu_ctx.dyn_stream_open(dyn_set, 2, None, 1, [0, 0])
    d_in, d_out, d_key = dev.up(np.zeros(128, np.float32)), dev.up(np.zeros(128, np.float32)), dev.up(np.zeros(64, np.float32))
    d_len = dev.up(np.array([64, 10], np.uint32))
    for st, key, key_stride, word in [(plain, d_key, 64, b"takes no key_dev"), (keyed, None, 64, b"needs key_dev"),
                                      (keyed, d_key, 63, b"key_stride < in_stride"), (keyed, d_out, 64, b"overlaps key_dev")]:
        with pytest.raises(G.GrailError):
            gpu_ctx.dyn_stream_next_async(st, d_in, 64, d_len, d_out, 64, key_dev=key, key_stride=key_stride)
        assert word in lib.grail_last_error(), lib.grail_last_error()
    # a call of no samples needs no key; two rows on the one key, the input its own key's neighbour
    out_len, bad, gain = gpu_ctx.dyn_stream_next(keyed, 2, None, 0, d_len, None, 0)
    assert out_len.tolist() == [0, 0] and gain.tolist() == [1.0, 1.0]
    out_len, bad, gain = gpu_ctx.dyn_stream_next(keyed, 2, d_in, 64, d_len, d_out, 64, key_dev=d_key, key_stride=64)
    assert out_len.tolist() == [64, 10] and bad.tolist() == [0, 0]
    with pytest.raises(G.GrailError):
        gpu_ctx.dyn_free(dyn_set)
    gpu_ctx.dyn_stream_close(plain)
    with pytest.raises(G.GrailError):                           # one stream is still open
        gpu_ctx.dyn_free(dyn_set)
    with pytest.raises(G.GrailError):                           # a closed stream is no stream
        gpu_ctx.dyn_stream_next_async(plain, d_in, 64, d_len, d_out, 64)
    gpu_ctx.dyn_stream_close(keyed)
    gpu_ctx.dyn_free(dyn_set)
    with pytest.raises(G.GrailError):                           # a freed set is no set
        gpu_ctx.dyn_stream_open(dyn_set, 2)
