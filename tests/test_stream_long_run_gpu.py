"""What only a stream has and the three stream suites do not reach (tests/KERNEL_PATHS.md, "streams"): a row that has been fed
2^32 samples or more, and one call of more than 64 chunks.

Rows that cross 2^32: the row is brought to N0 = 2^32 - (C + 100) samples by +0.0 fed through the public calls from one device
buffer (nothing is uploaded, the calls are queued without a wait, every out_len is held to the pure-host grail_*_stream_len
at that fed_before); then data in calls of C + 37, 126, 1, 0 and 2 C + 17 samples and the tail, bit for bit what the numpy
stream models give for a short stand-in row: M zeros as one first call, then the same data in the same calls.  Why M zeros
stand for N0 of them is asserted where M is chosen.  A count that is narrowed to 32 bits on the device takes the row for a
fresh one past 2^32: no history, the start-up paid again, other lengths.

Calls of more than 64 chunks: the advance kernels gather a row's chunk results with one lane per chunk, 64 at a time, and a
wave reduction; what the second lap adds is planted in chunk 64 alone.

The cases (the data, the model's results, the arithmetic of what lies where) are built by functions that need no device;
tests/test_kernel_paths_host.py runs them too."""
import ctypes as C

import numpy as np
import pytest

import grail_hip as G
import limit_stream_model as limit_model
import resample_stream_model as resample_stream
import test_fir_stream_gpu as fir
import test_limit_stream_gpu as limit
import test_resample_stream_gpu as resample
from fir_model import fir_model
from fir_stream_model import stream_model as fir_stream_model
from resample_model import resample_model
from test_fir_gpu import random_taps
from test_levels_gpu import CANARY, Dev, dev  # noqa: F401  (dev is a fixture)
from test_limiter_host import Q, limiter_model

pytestmark = pytest.mark.gpu
CROSSING = 1 << 32
HOLES = (np.nan, np.inf, -np.inf)
LONG_PAIRS = [(48000, 16000), (2, 3)]
LONG_ELLS = [10, 0]
LAPS = 65       # whole chunks of a long call, and a few outputs more: chunk 64 is the first of a lane's second lap


def at(ptr, floats):
    return C.c_void_p(ptr.value + 4 * floats)


def data_calls(chunk_in):
    """the calls behind the prefix, in input samples (chunk_in: those of one chunk of outputs): to 63 below 2^32; across it,
    leaving N odd; one sample; a pause; several chunks, all above -> (N0, the calls)"""
    calls = [chunk_in + 37, 126, 1, 0, 2 * chunk_in + 17]
    N0 = CROSSING - (chunk_in + 100)
    ends = [N0 + sum(calls[:k + 1]) for k in range(len(calls))]
    assert ends[0] == CROSSING - 63 and ends[1] == CROSSING + 63 and ends[1] % 2 == 1 and ends[2] % 4 == 0 and ends[3] == ends[2]
    return N0, calls


def holes_at(N0, calls):
    """the data's indices either side of every cut, of 2^32 and of the data's ends"""
    total = sum(calls)
    cuts = sorted({sum(calls[:k + 1]) for k in range(len(calls) - 1)} | {CROSSING - N0})
    places = sorted({0, total - 1} | {c - 1 for c in cuts} | set(cuts))
    assert CROSSING - 1 - N0 in places and CROSSING - N0 in places and all(0 <= p < total for p in places)
    return places


def plant(x, places):
    x[places] = [HOLES[i % 3] for i in range(len(places))]


def zeros_prefix(ctx, dev, n_rows, n_units, N0, big, out_stride, call, want_len):
    """N0 samples of +0.0 to every row, `big` a call from one buffer and the rest in the last; call(in, in_stride, in_len,
    out, out_stride, out_len) queues one; one wait behind them all.  Every call's out_len is want_len(unit, fed_before, n),
    and the last 4096 outputs of the last call are +0.0 in every bit."""
    assert n_rows * (big + out_stride) * 4 <= 4 << 30
    d_in, d_out = dev.alloc(n_rows * big * 4), dev.alloc(n_rows * out_stride * 4)
    ctx.memset(d_in, 0, n_rows * big * 4)
    n_calls = -(-N0 // big)
    last = N0 - (n_calls - 1) * big
    assert 4096 < last <= big
    d_full, d_last = dev.up(np.full(n_rows, big, np.uint32)), dev.up(np.full(n_rows, last, np.uint32))
    d_lens = dev.up(np.full(n_calls * n_units, 77, np.uint32))
    fed = [(k * big, big if k < n_calls - 1 else last) for k in range(n_calls)]
    assert sum(n for _, n in fed) == N0
    for k in range(n_calls):
        call(d_in, big, d_full if k < n_calls - 1 else d_last, d_out, out_stride, at(d_lens, k * n_units))
    ctx.sync()
    lens = dev.down(d_lens, (n_calls, n_units), np.uint32)
    for k, (before, n) in enumerate(fed):
        for u in range(n_units):
            assert lens[k, u] == want_len(u, before, n), (k, u, before, n, lens[k, u], want_len(u, before, n))
    for row in range(n_rows):
        n_out = int(lens[-1, row * n_units // n_rows])
        assert n_out >= 4096
        assert not dev.down(d_out, 4096, np.uint32, offset=4 * (row * out_stride + n_out - 4096)).any(), row


# ---- A. rows that cross 2^32 samples ---------------------------------------------------------------------------------------------
def long_filter_case():
    """-> (filters, N0, calls, rows, the stand-ins' models)"""
    rng = np.random.default_rng(3201)
    filters = [(random_taps(9, rng), 4), (random_taps(40, rng), 0), (random_taps(255, rng), 127)]
    N0, calls = data_calls(fir.CHUNK)
    rows = []
    for _ in filters:
        x = fir.noise(sum(calls), rng, holes=False)
        plant(x, holes_at(N0, calls))
        rows.append(x)
    # the stand-in: every tap of a data call's outputs reaches back K - 1 samples at most, and the outputs known after N
    # samples are N - origin once N >= origin, so M zeros with both are N0 zeros to everything behind them
    M = 256
    assert all(M >= len(h) - 1 and M >= o for h, o in filters)
    models = [fir_stream_model(np.concatenate([np.zeros(M, np.float32), x]), h, o, [M] + calls) for x, (h, o) in zip(rows, filters)]
    return filters, N0, calls, rows, models


def test_filter_rows_fed_past_2_to_the_32(gpu_ctx):
    """three rows of one stream on (K = 9, origin 4), (K = 40, origin 0) and (K = 255, origin 127).  The third is there because
    the calls leave N at 2^32 + 63 and 2^32 + 64: an N cut to 32 bits reads 63 and 64, which the first two filters cannot
    tell from the truth (63 is above their K - 1 and their origin, and the ring's capacity divides 2^32); the third waits
    for its origin again and loses its history"""
    filters, N0, calls, rows, models = long_filter_case()
    big = 1 << 27
    dev = Dev(gpu_ctx)
    fir_set = gpu_ctx.fir_create(filters)
    fs = gpu_ctx.fir_stream_open(fir_set, 3, [0, 1, 2])
    try:
        zeros_prefix(gpu_ctx, dev, 3, 3, N0, big, big,
                     lambda *a: gpu_ctx.fir_stream_next_async(fs, *a),
                     lambda u, before, n: G.fir_stream_len(before, n, len(filters[u][0]), filters[u][1]))
        dev.free()
        fed = 0
        for c, n in enumerate(calls):
            out, out_len, bad = fir.feed(gpu_ctx, dev, fs, [x[fed:fed + n] for x in rows])
            fir.same(out, out_len, [m[0][1 + c][0] for m in models], ("call", c), bad, [m[0][1 + c][1] for m in models])
            assert all(out_len[u] == G.fir_stream_len(N0 + fed, n, len(h), o) for u, (h, o) in enumerate(filters))
            fed += n
        out, out_len = fir.ring_out(gpu_ctx, dev, fs, 3, 256)
        fir.same(out, out_len, [m[1] for m in models], "tail")
        assert [int(v) for v in out_len] == [G.fir_stream_len(N0 + fed, 0, len(h), o, finishing=True) for h, o in filters] == [8, 39, 254]
    finally:
        gpu_ctx.fir_stream_close(fs)
        gpu_ctx.fir_free(fir_set)
        dev.free()


def long_resample_case(pair):
    """-> (N0, calls, the row, the stand-in's model)"""
    rng = np.random.default_rng(3202 + pair[0] % 97)
    num, U, D, P = resample.table(pair)
    assert (U == 1) == (pair == (48000, 16000))
    N0, calls = data_calls(resample_stream.ceil_div(resample.CHUNK * D, U))
    x = resample.noise(sum(calls), rng)
    plant(x, holes_at(N0, calls))
    # the stand-in: a data call's taps reach back P - 1 samples at most; the first output is known past h = P / 2 samples; and a
    # shift of the input by a multiple of D shifts the outputs by a whole number and keeps every phase
    M = P
    while M % D != N0 % D:
        M += 1
    assert M >= P - 1 and M > P // 2 and (N0 - M) % D == 0
    model = resample_stream.stream_model(np.concatenate([np.zeros(M, np.float32), x]), num, D, [M] + calls)
    return N0, calls, x, model


@pytest.mark.parametrize("pair", LONG_PAIRS)
def test_a_resampled_row_fed_past_2_to_the_32(gpu_ctx, pair):
    """(48000, 16000): one phase, the next output's time i three times the outputs written; (2, 3): up = 3, i and N differ and
    the phase cycles"""
    N0, calls, x, model = long_resample_case(pair)
    _, U, D, _ = resample.table(pair)
    big = 1 << 28
    out_stride = (resample_stream.ceil_div(big * U, D) + 3) // 4 * 4
    dev = Dev(gpu_ctx)
    rs = gpu_ctx.resample_stream_open(pair[0], pair[1], 1)
    try:
        zeros_prefix(gpu_ctx, dev, 1, 1, N0, big, out_stride,
                     lambda *a: gpu_ctx.resample_stream_next_async(rs, *a),
                     lambda u, before, n: G.resample_stream_len(before, n, *pair))
        dev.free()
        fed = 0
        for c, n in enumerate(calls):
            out, out_len, bad = resample.feed(gpu_ctx, dev, rs, pair, [x[fed:fed + n]])
            resample.same(out, out_len, [model[0][1 + c][0]], ("call", c), bad, [model[0][1 + c][1]])
            assert out_len[0] == G.resample_stream_len(N0 + fed, n, *pair)
            fed += n
        out, out_len = resample.flush(gpu_ctx, dev, rs, 1, (resample.tail_room(pair) + 7) // 4 * 4)
        resample.same(out, out_len, [model[1]], "tail")
        assert out_len[0] == G.resample_stream_len(N0 + fed, 0, *pair, finishing=True) > 0
    finally:
        gpu_ctx.resample_stream_close(rs)
        dev.free()


def long_limit_case(ell):
    """-> (N0, calls, the pair's members, the stand-in's calls and tail)"""
    rng = np.random.default_rng(3203 + ell)
    L, c = 1 << ell, limit.CEILING
    N0, calls = data_calls(limit.CHUNK)
    total = sum(calls)
    members = [rng.uniform(-0.3, 0.3, total).astype(np.float32) for _ in range(2)]
    plant(members[0], holes_at(N0, calls))
    hot = sorted({CROSSING - 1 - N0, CROSSING - N0, CROSSING - (L - 1) - N0, CROSSING - L - N0} | {int(t) for t in rng.integers(0, total, 24)})
    members[1][hot] = 4 * c
    # the stand-in: no output of a call needs a sample before N - 3 L - 19 (limit_stream_model asserts it call by call), and
    # the outputs final after N samples are N - (L + 10) once N is above that
    M = 3 * L + 19
    M += (N0 - M) % 4                                                       # (the same N mod 4, for the reader's sake)
    assert M >= 3 * L + 19 and (N0 - M) % 4 == 0
    lead = np.zeros(M, np.float32)
    model_calls, model_tail = limit_model.stream_model([np.concatenate([lead, x]) for x in members], c, ell, [M] + calls)
    assert all(k[2] > 0 and k[1] < 1 for k, n in zip(model_calls[1:], calls) if n > 1), "a call that limits nothing"
    return N0, calls, members, model_calls, model_tail


@pytest.mark.parametrize("ell", LONG_ELLS)
def test_a_limited_pair_fed_past_2_to_the_32(gpu_ctx, ell):
    """group = 2 under a ceiling of 0.5: the first member carries the samples that are not finite, the second samples of four
    times the ceiling at 2^32 - 1, at 2^32 and L - 1 and L before it, so that a look-ahead window and a release lie across the
    crossing; a few more of them anywhere, so that every call limits.  ell = 0 holds the 64-bit arithmetic to the model where
    everything the kernel reaches back for (11 samples of delay, a ring of 32) is nearer than the 63 that an N cut to 32 bits
    would read behind the crossing; ell = 10 (1 034 and 4 096) is the case that tells such a cut"""
    N0, calls, members, model_calls, model_tail = long_limit_case(ell)
    big = 1 << 27
    dev = Dev(gpu_ctx)
    ls = gpu_ctx.limit_stream_open(2, limit.CEILING, ell, group=2)
    try:
        zeros_prefix(gpu_ctx, dev, 2, 1, N0, big, big, ls.next_async, lambda u, before, n: G.limit_stream_len(before, n, ell))
        dev.free()
        fed = 0
        for k, n in enumerate(calls):
            out, res = limit.feed(gpu_ctx, dev, ls, [x[fed:fed + n] for x in members])
            limit.same(out, res, [model_calls[1 + k]], 2, ("call", k))
            assert res[0][0] == G.limit_stream_len(N0 + fed, n, ell)
            fed += n
        out, res = limit.flush(gpu_ctx, dev, ls)
        limit.same(out, res, [model_tail], 2, "tail")
        assert res[0][0] == G.limit_stream_len(N0 + fed, 0, ell, finishing=True) == (1 << ell) + 10
    finally:
        ls.close()
        dev.free()


# ---- B. one call of more than 64 chunks ----------------------------------------------------------------------------------------
def lapped_filter_case():
    """133 125 outputs: chunk c counts the call's samples [c CHUNK, (c + 1) CHUNK), the last chunk to their end
    -> (filters, the row, its outputs in the call, the planted samples)"""
    rng = np.random.default_rng(3211)
    K, o = 9, 4
    filters = [(random_taps(K, rng), o)]
    n_out = LAPS * fir.CHUNK + 5
    n = n_out + o
    chunks = -(-n_out // fir.CHUNK)
    assert n_out == 133125 and chunks == 66 > 64
    planted = [7, 63 * fir.CHUNK + 11, 64 * fir.CHUNK + 1, 64 * fir.CHUNK + 1000, n - 1]
    assert [min(t // fir.CHUNK, chunks - 1) for t in planted] == [0, 63, 64, 64, 65]
    x = fir.noise(n, rng, holes=False)
    x[planted] = [np.nan, np.inf, -np.inf, np.nan, np.inf]
    assert fir_model(x, *filters[0])[2] == len(planted)
    return filters, x, n_out, planted


def test_a_filter_call_of_more_than_64_chunks(gpu_ctx, dev):
    """non-finite samples in chunks 0, 63, 64 (two) and 65: the count is 5, and 2 where the second lap is lost"""
    filters, x, n_out, planted = lapped_filter_case()
    fir_set = gpu_ctx.fir_create(filters)
    fs = gpu_ctx.fir_stream_open(fir_set, 1)
    try:
        out, out_len, bad = fir.feed(gpu_ctx, dev, fs, [x])
        assert out_len[0] == n_out and bad[0] == len(planted), (out_len, bad)
        tail, tail_len = fir.ring_out(gpu_ctx, dev, fs, 1, len(filters[0][0]) - 1)
        joined = np.concatenate([out[0, :out_len[0]], tail[0, :tail_len[0]]])
    finally:
        gpu_ctx.fir_stream_close(fs)
        gpu_ctx.fir_free(fir_set)
    assert np.all(out[0, n_out:] == CANARY)
    fir.whole_rows([joined], filters, [x], [0])


def lapped_resample_case():
    """66 563 outputs at (2, 3): chunk c counts the call's samples from its first output's time, ceil(c CHUNK D / U), to the
    next chunk's, the last chunk to their end -> (pair, the row, its outputs in the call, the planted samples)"""
    rng = np.random.default_rng(3212)
    pair = (2, 3)
    num, U, D, P = resample.table(pair)
    n_out = LAPS * resample.CHUNK + 3
    n = P // 2 + n_out * D // U
    chunks = -(-n_out // resample.CHUNK)
    assert resample_stream.known(n, U, D, P) == n_out == 66563 and chunks == 66 > 64
    starts = [resample_stream.ceil_div(c * resample.CHUNK * D, U) for c in range(chunks)]
    planted = [3, starts[63] + 5, starts[64], starts[64] + 300, n - 1]
    assert [max(c for c in range(chunks) if starts[c] <= t) for t in planted] == [0, 63, 64, 64, 65] and starts[65] < n - 1
    x = resample.noise(n, rng)
    x[[0, n // 2]] = 0.25                                                    # (noise's own holes: only the planted ones count)
    x[planted] = [np.nan, np.inf, -np.inf, np.nan, np.inf]
    assert resample_model(x, num, D)[2] == len(planted)
    return pair, x, n_out, planted


def test_a_resample_call_of_more_than_64_chunks(gpu_ctx, dev):
    """non-finite samples in chunks 0, 63, 64 (two) and 65: the count is 5, and 2 where the second lap is lost"""
    pair, x, n_out, planted = lapped_resample_case()
    rs = gpu_ctx.resample_stream_open(pair[0], pair[1], 1)
    try:
        out, out_len, bad = resample.feed(gpu_ctx, dev, rs, pair, [x])
        assert out_len[0] == n_out and bad[0] == len(planted), (out_len, bad)
        tail, tail_len = resample.flush(gpu_ctx, dev, rs, 1, (resample.tail_room(pair) + 7) // 4 * 4)
        joined = np.concatenate([out[0, :out_len[0]], tail[0, :tail_len[0]]])
    finally:
        gpu_ctx.resample_stream_close(rs)
    assert np.all(out[0, n_out:] == CANARY)
    resample.whole_rows([joined], pair, [x])


LAPPED_HOT = {"64": {64: 0.9}, "2 and 64": {2: 2.0, 64: 0.9}, "0 and 64": {0: 2.0, 64: 0.9}}


def lapped_limit_case(hot):
    """266 269 outputs of a pair at ell = 3: quiet noise, non-finite samples in chunks 0, 63, 64 (two) and 65, and one sample of
    hot[k] in the middle of chunk k; outputs [k T, (k + 1) T) are chunk k's -> (ell, the members, the model's call and tail)"""
    rng = np.random.default_rng(3213)
    ell, c, T = 3, limit.CEILING, limit.CHUNK
    L = 1 << ell
    n_out = LAPS * T + 29
    n = n_out + limit_model.delay(ell)
    chunks = -(-n_out // T)
    assert n_out == 266269 and chunks == 66 > 64
    planted = [5, 63 * T + 9, 64 * T + 2, 64 * T + 3000, n - 1]
    assert [min(t // T, chunks - 1) for t in planted] == [0, 63, 64, 64, 65]
    members = [rng.uniform(-0.1, 0.1, n).astype(np.float32) for _ in range(2)]
    members[0][planted] = [np.nan, np.inf, -np.inf, np.nan, np.inf]
    for k, level in hot.items():
        members[1][k * T + T // 2] = level
    (call,), tail = limit_model.check_against_one_shot(members, c, ell, [n])
    # which chunks limit, and how far, from the model's curves
    _, _, _, _, ((_, S, g),) = limiter_model(members, c, ell, group=2, curves=True)
    per_chunk = [(g[k * T:min((k + 1) * T, n_out)].min(), int(np.count_nonzero(S[k * T:min((k + 1) * T, n_out)] < L * Q)))
                 for k in range(chunks)]
    assert [k for k, (_, limited) in enumerate(per_chunk) if limited] == sorted(hot)
    assert all((gain < 1) == (k in hot) for k, (gain, _) in enumerate(per_chunk))
    assert call[2] == sum(limited for _, limited in per_chunk) > 0
    assert call[1] == min(gain for gain, _ in per_chunk) == per_chunk[min(hot)][0] < 1
    assert len(hot) == 1 or per_chunk[64][0] > call[1]                       # the last chunk read is not the answer
    assert call[3] == len(planted) and tail[2] == 0
    return ell, members, call, tail


@pytest.mark.parametrize("hot", list(LAPPED_HOT.values()), ids=list(LAPPED_HOT))
def test_a_limit_call_of_more_than_64_chunks(gpu_ctx, dev, hot):
    """samples above the ceiling in chunk 64 alone: min_gain < 1 and n_limited > 0 come from the second lap; or the lowest gain
    from chunk 2 (another lane of the first lap) or chunk 0 (the same lane's first lap) and a milder one from chunk 64: the
    maximum over both laps, not the last read"""
    ell, members, call, tail = lapped_limit_case(hot)
    ls = gpu_ctx.limit_stream_open(2, limit.CEILING, ell, group=2)
    try:
        out, res = limit.feed(gpu_ctx, dev, ls, members)
        limit.same(out, res, [call], 2, "the call")
        out, res = limit.flush(gpu_ctx, dev, ls)
        limit.same(out, res, [tail], 2, "tail")
    finally:
        ls.close()
