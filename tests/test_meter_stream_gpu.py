"""Meter streams on the device (grail_meter_stream_*) against the numpy model of tests/meter_stream_model.py, bit for bit in the
hop sums, the counts, the true peaks of every call and of the finish, and in what `read` shows after every call: the calls' hop
sums end to end are what grail_loudness_async gives for the whole row, the largest of the true peaks is grail_true_peak_async's,
whatever the split.  The harness is that of tests/test_limit_stream_gpu.py: the inputs hold NaN outside the rows' samples and
are overwritten as soon as the call is queued, the hop sums go into a buffer of a canary with guards around it: nothing is
written past n_hops or outside the buffer, nothing is read past a row's samples or after the call.
Rate 2560 (H = 256, the smallest hop) with the 48 kHz coefficients, as the segmented tests do: the filter forgets only 0.28 a
hop, so a state that is one sample or one bit off shows in every later hop."""
import ctypes as C

import numpy as np
import pytest

import grail_hip as G
from meter_stream_model import REFUSED, RowModel, bits, check_against_one_shot, random_split
from test_levels_gpu import Dev, dev, same_bits  # noqa: F401  (dev is a fixture)
from test_loudness_host import kweighting_model

pytestmark = pytest.mark.gpu
RATE = 2560
H = RATE // 10
COEF = kweighting_model(48000)
CANARY = -7.25
READ_TYPES = (np.float64, np.float64, np.float64, np.float64, np.uint64)


def at(ptr, nbytes):
    return C.c_void_p(ptr.value + nbytes)


def noise(n, seed, amplitude=0.5):
    return np.random.default_rng(seed).uniform(-amplitude, amplitude, n).astype(np.float32)


def feed(ctx, dev, ms, chunks, stride=None, in_offset=0, hops_stride=None, guard=8):
    """one `next` call: chunks[i] as row i of an input buffer that holds NaN everywhere else and is overwritten as soon as the
    call is queued, the hop sums into a buffer of the canary with `guard` doubles of it before and after
    -> (hops [n_rows, hops_stride] as they lie on the device afterwards, (n_hops, true_peak, nonfinite) per row)"""
    n_rows = len(chunks)
    longest = max([len(c) for c in chunks] + [1])
    stride = stride or (longest + 63) // 64 * 64
    hops_stride = ms.hops_stride(stride) if hops_stride is None else hops_stride
    host = np.full(n_rows * stride + in_offset, np.nan, np.float32)
    for i, c in enumerate(chunks):
        host[in_offset + i * stride:in_offset + i * stride + len(c)] = c
    d_in = dev.up(host)
    d_hops = dev.up(np.full(guard + n_rows * hops_stride + guard, CANARY, np.float64))
    d_len = dev.up(np.array([len(c) for c in chunks], np.uint32))
    types = (np.uint32, np.float64, np.uint32)
    d_res = [dev.up(np.full(n_rows, 77, t)) for t in types]
    ms.next_async(at(d_in, 4 * in_offset), stride, d_len, at(d_hops, 8 * guard), hops_stride, *d_res)
    ctx.memset(d_in, 0x7F, host.nbytes)                 # (3.4e38 everywhere: a late read would show)
    res = tuple(dev.down(p, n_rows, t) for p, t in zip(d_res, types))
    out = dev.down(d_hops, guard + n_rows * hops_stride + guard, np.float64)
    assert np.all(out[:guard] == CANARY) and np.all(out[guard + n_rows * hops_stride:] == CANARY), "written outside the hop sums"
    dev.free()
    return out[guard:guard + n_rows * hops_stride].reshape(n_rows, hops_stride), res


def same(out, res, want, what):
    """a call's rows against the model's: want[u] = (hops, true_peak, nonfinite), None: a refused row, "idle": a row the call
    leaves alone (0, +0.0, 0); past the hops the canary"""
    for u, w in enumerate(want):
        if w is None:
            assert res[0][u] == REFUSED and np.isnan(res[1][u]) and res[2][u] == 0 and np.all(out[u] == CANARY), (what, u, "refused")
            continue
        if isinstance(w, str):
            w = (np.zeros(0), 0.0, 0)
        n = len(w[0])
        assert res[0][u] == n, (what, u, res[0][u], n)
        assert np.all(out[u, n:] == CANARY), (what, u, "written past the row's hops")
        assert np.array_equal(bits(out[u, :n]), bits(w[0])), (what, u, out[u, :n], w[0])
        assert bits(res[1][u]) == bits(w[1]), (what, u, "true peak", res[1][u], w[1])
        assert res[2][u] == w[2], (what, u, "nonfinite", res[2][u], w[2])


def same_reading(got, want, what):
    """ms.read() against the models' read() per row"""
    for u, w in enumerate(want):
        for k, name in enumerate(("integrated", "momentary", "short-term", "true peak")):
            assert bits(got[k][u]) == bits(w[k]), (what, u, name, got[k][u], w[k])
        assert got[4][u] == w[4], (what, u, "hops", got[4][u], w[4])


_MODELS = {}


def model_of(x, split):
    """check_against_one_shot(x, split), computed once: the layouts and the lone runs ask for the same rows again"""
    key = (np.asarray(x, np.float32).tobytes(), tuple(split))
    if key not in _MODELS:
        _MODELS[key] = check_against_one_shot(x, split, RATE, COEF)
    return _MODELS[key]


def stream_rows(ctx, dev, rows, row_splits, finishes=(None,), max_hops=64, read_every_call=True, **layout):
    """rows[u] fed as row_splits[u] says (shorter splits pause at the end), then finished in the calls `finishes` (each a list
    of marks, None: every row): every call, every read and the finishes against the model, which is held to the one-shot
    models -> per row (the hops end to end, the largest true peak, the sum of the counts)"""
    n_rows = len(rows)
    n_calls = max(len(s) for s in row_splits)
    row_splits = [list(s) + [0] * (n_calls - len(s)) for s in row_splits]
    models = [model_of(x, s) for x, s in zip(rows, row_splits)]
    ms = ctx.meter_stream_open(n_rows, RATE, max_hops, COEF)
    try:
        fed = [0] * n_rows
        joined = [[np.zeros(0)] for _ in rows]
        peaks = [[0.0] for _ in rows]
        bad = [0] * n_rows
        for k in range(n_calls):
            chunks = [x[fed[u]:fed[u] + row_splits[u][k]] for u, x in enumerate(rows)]
            out, res = feed(ctx, dev, ms, chunks, **layout)
            same(out, res, [m[0][k] for m in models], ("call", k))
            for u in range(n_rows):
                joined[u].append(out[u, :res[0][u]])
                peaks[u].append(res[1][u])
                bad[u] += int(res[2][u])
                fed[u] += row_splits[u][k]
            if read_every_call:
                same_reading(ms.read(), [m[1][k] for m in models], ("read after call", k))
        ended = [False] * n_rows
        for which in finishes:
            marked = [not ended[u] and (which is None or bool(which[u])) for u in range(n_rows)]
            tails = ms.finish(which)
            for u in range(n_rows):
                assert bits(tails[u]) == bits(models[u][2] if marked[u] else 0.0), ("finish", which, u, tails[u])
                peaks[u].append(tails[u])
                ended[u] = ended[u] or marked[u]
            same_reading(ms.read(), [m[3] if ended[u] else m[1][-1] for u, m in enumerate(models)], ("read after finish", which))
        assert all(ended)
        ledger = ms.ledger_rows()
        for u in range(n_rows):
            assert np.array_equal(bits(ledger[u]), bits(np.concatenate(joined[u]))), ("ledger", u)
    finally:
        ms.close()
    return [(np.concatenate(j), max(p), b) for j, p, b in zip(joined, peaks, bad)]


def one_shot_on_device(ctx, dev, rows):
    """grail_loudness_async and grail_true_peak_async on the whole rows -> per row (gated, hops, true peak, nonfinite)"""
    longest = max([len(x) for x in rows] + [1])
    stride = (longest + 63) // 64 * 64
    host = np.full((len(rows), stride), np.nan, np.float32)
    for i, x in enumerate(rows):
        host[i, :len(x)] = x
    d_rows, d_len = dev.up(host), dev.up(np.array([len(x) for x in rows], np.uint32))
    gated, hops, bad = ctx.loudness(d_rows, stride, d_len, len(rows), RATE, COEF)
    peak, bad_tp = ctx.true_peak(d_rows, stride, d_len, len(rows))
    assert np.array_equal(bad, bad_tp)
    dev.free()
    return [(gated[i], hops[i, :len(x) // H], peak[i], int(bad[i])) for i, x in enumerate(rows)]


def held_to_the_device(ctx, dev, rows, got, what):
    for u, ((gated, hops, peak, bad), (joined, largest, count)) in enumerate(zip(one_shot_on_device(ctx, dev, rows), got)):
        assert np.array_equal(bits(joined), bits(hops)), (what, u, "hops")
        assert bits(largest) == bits(peak) and count == bad, (what, u, largest, peak, count, bad)


def fit(parts, N):
    """parts cut to what is left of N samples, then the rest (as limit_stream_model.splits cuts its parts)"""
    out, left = [], N
    for p in parts:
        p = min(p, left)
        out.append(p)
        left -= p
    return out + [left]


# ---- 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hops", [5, 8])
def test_lockstep(gpu_ctx, dev, hops):
    """3 rows fed the same chunks: the wave-uniform walk (the lanes past the launch's last row walk along).  At 5 H + 17 samples
    the chunks (64, 65, H - 1, H, H + 1, 2 H + 3) sum to more than the row and the last is cut to what is left; at 8 H + 17 all
    of them fit, a call of two hops among them, and the rest follows"""
    N = hops * H + 17
    rows = [noise(N, 800 + 10 * hops + u) for u in range(3)]
    rows[1][[0, 64, N - 1]] = [np.nan, np.inf, -np.inf]
    split = fit([64, 65, H - 1, H, H + 1, 2 * H + 3], N)
    assert sum(split) == N and (hops == 5 or split[5:] == [2 * H + 3, N - 5 * H - 132])
    got = stream_rows(gpu_ctx, dev, rows, [split] * 3)
    held_to_the_device(gpu_ctx, dev, rows, got, "lockstep")
    assert got[1][2] == 3 and all(len(g[0]) == hops for g in got)


def test_lockstep_in_a_full_wave_and_a_partial_one(gpu_ctx, dev):
    """70 rows in lockstep: both waves take the uniform walk, the second with 58 lanes that are no row"""
    N = 2 * H + 70
    rows = [noise(N, 820 + u) for u in range(70)]
    got = stream_rows(gpu_ctx, dev, rows, [[63, 1, 64, H, N - H - 128]] * 70, read_every_call=False)
    held_to_the_device(gpu_ctx, dev, rows, got, "70 rows in lockstep")


# ---- 2 ---------------------------------------------------------------------------------------------------------------------
def test_ragged(gpu_ctx, dev):
    """70 rows (a full wave and a partial one), each with its own length between 0 and 6 H and its own random split, with calls
    of 0 samples and chunks of 1; no two neighbouring lanes share N mod H after the first call; rows are finished in three
    `finish` calls through `which`.  The predicated walk: the case the one-shot kernel never meets"""
    rng = np.random.default_rng(830)
    lengths = [0, 1, H - 1, H, H + 1, 6 * H, 6 * H - 1, 64, 63, 65, 3 * H + 32] + [int(rng.integers(2, 6 * H)) for _ in range(59)]
    rows = [noise(n, 831 + u) for u, n in enumerate(lengths)]
    rows[5][[0, 700, 6 * H - 1]] = [np.inf, np.nan, np.nan]
    splits = []
    for u, n in enumerate(lengths):
        first = min(n, 1 + (u * 37) % 251)                # neighbours start their second call at different places in the hop
        ones = [1, 0, 1] if u % 7 == 0 and n - first >= 2 else []
        splits.append([first] + ones + random_split(n - first - sum(ones), rng, most=2 * H))
        assert sum(splits[-1]) == n
    for a, b in zip(splits, splits[1:]):
        assert a[0] % H != b[0] % H or a[0] == 0 or b[0] == 0
    finishes = ([u % 3 == 0 for u in range(70)], [u % 3 != 2 for u in range(70)], None)
    got = stream_rows(gpu_ctx, dev, rows, splits, finishes=finishes, read_every_call=False)
    held_to_the_device(gpu_ctx, dev, rows, got, "ragged")
    assert got[5][2] == 3


# ---- 3 ---------------------------------------------------------------------------------------------------------------------
def test_hop_ends_at_every_edge(gpu_ctx, dev):
    """a hop's end on a chunk's last sample and no tile's (row 0: the chunk starts at N mod H = 10, its 246th sample ends the
    hop), on a tile's last sample inside a chunk (row 1: the chunk starts at N mod H = 192, so the hop ends on its 64th
    sample, t = 63 mod 64), on both (row 2: a chunk of 64 from there), and on a chunk's first sample (row 3); the rows differ
    in where they stand, so the wave takes the predicated walk, and the same splits one row at a time take the uniform one:
    same bits"""
    N = 3 * H
    rows = [noise(N, 840 + u) for u in range(4)]
    splits = [[10, H - 10, N - H], [192, 128, N - 320], [192, 64, N - 256], [H - 1, 50, N - H - 49]]
    got = stream_rows(gpu_ctx, dev, rows, splits)
    held_to_the_device(gpu_ctx, dev, rows, got, "edges")
    for x, s, g in zip(rows, splits, got):
        (alone,) = stream_rows(gpu_ctx, dev, [x], [s], read_every_call=False)
        assert np.array_equal(bits(alone[0]), bits(g[0])) and bits(alone[1]) == bits(g[1])


def test_a_hop_in_calls_of_one_sample(gpu_ctx, dev):
    x = noise(H, 845)
    x[[10, H - 1]] = [np.nan, np.inf]
    got = stream_rows(gpu_ctx, dev, [x], [[1] * H], read_every_call=False)
    held_to_the_device(gpu_ctx, dev, [x], got, "H calls of 1")
    assert len(got[0][0]) == 1 and got[0][2] == 2


# ---- 4 ---------------------------------------------------------------------------------------------------------------------
def test_a_mixed_wave(gpu_ctx, dev):
    """one wave holding a paused row, an ended row and a live row: after twenty calls the paused row reads what it read before
    them, and fed again its hops continue as the model says"""
    x = [noise(2 * H + 40, 850), noise(100, 851), noise(20 * 70 + 2 * H, 852)]
    models = [RowModel(RATE, COEF) for _ in x]
    ms = gpu_ctx.meter_stream_open(3, RATE, 16, COEF)
    try:
        first = [x[0][:H + 40], x[1], x[2][:2 * H]]
        out, res = feed(gpu_ctx, dev, ms, first)
        same(out, res, [m.next(c) for m, c in zip(models, first)], "first call")
        tails = ms.finish([0, 1, 0])
        assert bits(tails[1]) == bits(models[1].finish()) and bits(tails[0]) == bits(0.0) and bits(tails[2]) == bits(0.0)
        before = ms.read()
        same_reading(before, [m.read() for m in models], "before the pause")
        for k in range(20):
            chunk = x[2][2 * H + 70 * k:2 * H + 70 * (k + 1)]
            out, res = feed(gpu_ctx, dev, ms, [x[0][:0], x[1][:0], chunk])
            same(out, res, ["idle", "idle", models[2].next(chunk)], ("paused", k))
        after = ms.read()
        for k in range(5):
            assert bits(after[k][0]) == bits(before[k][0]) and bits(after[k][1]) == bits(before[k][1]), ("the paused and the ended row", k)
        rest = x[0][H + 40:]
        out, res = feed(gpu_ctx, dev, ms, [rest, x[1][:0], x[2][:0]])
        same(out, res, [models[0].next(rest), "idle", "idle"], "the paused row fed again")
        assert res[0][0] == 1
        same_reading(ms.read(), [m.read() for m in models], "at the end")
    finally:
        ms.close()


# ---- 5 ---------------------------------------------------------------------------------------------------------------------
LAYOUTS = {"aligned": dict(stride=1024), "odd stride": dict(stride=1023), "off by one float": dict(stride=1024, in_offset=1),
           "both": dict(stride=1021, in_offset=3)}


@pytest.mark.parametrize("n_rows", [1, 65])
def test_alignment(gpu_ctx, dev, n_rows):
    """a base one float off and an odd stride take the 4-byte form of both kernels: the same bits as the aligned run"""
    N = 3 * H + 90
    rows = [noise(N, 860 + u) for u in range(n_rows)]
    split = [400, 401, N - 801]
    want = None
    for name, layout in LAYOUTS.items():
        got = stream_rows(gpu_ctx, dev, rows, [split] * n_rows, read_every_call=False, **layout)
        mid = got[n_rows // 2]
        want = mid if want is None else want
        assert np.array_equal(bits(mid[0]), bits(want[0])) and bits(mid[1]) == bits(want[1]), name
    held_to_the_device(gpu_ctx, dev, rows[:1], [stream_rows(gpu_ctx, dev, rows[:1], [split], stride=1023, in_offset=1)[0]], "4-byte loads")


# ---- 6 ---------------------------------------------------------------------------------------------------------------------
def test_non_finite_samples(gpu_ctx, dev):
    """NaN and +-Inf as a chunk's first and last sample and inside the eleven that go into the ring: counted in the call that
    fed them and only there, +0.0 in both meters"""
    N = 2 * H + 50
    x = noise(N, 870)
    split = [100, 30, 5, N - 135]
    hot = [0, 99, 100, 129, 130, 134, 135, 125, 93, N - 1, N - 6]
    x[hot] = [np.nan, np.inf, -np.inf, np.nan, np.inf, np.nan, -np.inf, np.nan, np.inf, np.nan, np.inf]
    clean = x.copy()
    clean[hot] = 0.0
    models = check_against_one_shot(x, split, RATE, COEF)
    assert [c[2] for c in models[0]] == [3, 3, 2, 3]
    (got,) = stream_rows(gpu_ctx, dev, [x], [split])
    (zeros,) = stream_rows(gpu_ctx, dev, [clean], [split], read_every_call=False)
    assert np.array_equal(bits(got[0]), bits(zeros[0])) and bits(got[1]) == bits(zeros[1]) and got[2] == 11 and zeros[2] == 0
    held_to_the_device(gpu_ctx, dev, [x], [got], "non-finite")


# ---- 7 ---------------------------------------------------------------------------------------------------------------------
def test_true_peak_across_calls(gpu_ctx, dev):
    """the header's own example: a row [0, ..., 0, 1.0] whose 1.0 is a chunk's last sample reads 7964 / 8192 only from `finish`;
    as a chunk's first sample, from the call after it; and a row whose largest output needs samples of three calls of 5"""
    x = np.zeros(40, np.float32)
    x[-1] = 1.0
    ms = gpu_ctx.meter_stream_open(1, RATE, 4, COEF)
    try:
        peaks = [feed(gpu_ctx, dev, ms, [c])[1][1][0] for c in (x[:25], x[25:])]
        assert peaks == [0.0, 239 / 8192] and ms.read()[3][0] == 239 / 8192
        assert ms.finish()[0] == 7964 / 8192 == ms.read()[3][0]
    finally:
        ms.close()
    y = np.concatenate([x, np.zeros(30, np.float32)])
    (got,) = stream_rows(gpu_ctx, dev, [y], [[39, 1, 5, 25]])
    assert got[1] == 7964 / 8192
    (got,) = stream_rows(gpu_ctx, dev, [y], [[39, 7, 24]])             # the 1.0 as a chunk's first sample, the crest as its last
    assert got[1] == 7964 / 8192
    # calls of 5: every output's twelve samples come from three or four successive calls, the largest one's too
    z = noise(60, 875)
    z[48:] = 0.0
    split = [5] * 12
    calls, _, tail, last = model_of(z, split)
    assert max(c[1] for c in calls) == last[3] > tail
    (got,) = stream_rows(gpu_ctx, dev, [z], [split])
    held_to_the_device(gpu_ctx, dev, [y, z], [stream_rows(gpu_ctx, dev, [y], [[40, 30]])[0], got], "true peak")


# ---- 8 ---------------------------------------------------------------------------------------------------------------------
def test_read_in_mid_stream(gpu_ctx, dev):
    """after every call of a 40-hop row the numbers equal the model's (stream_rows) and the one-shot device calls on the prefix
    fed so far; rows of 3, 4, 29 and 30 hops beside it cover where each window begins; the ledger equals the hops"""
    lengths = [40 * H + 9, 3 * H + 5, 4 * H + 5, 29 * H + 5, 30 * H + 5]
    rows = [noise(n, 880 + u) for u, n in enumerate(lengths)]
    step = 3 * H + 7
    splits = [fit([step] * (n // step), n) for n in lengths]
    got = stream_rows(gpu_ctx, dev, rows, splits)
    held_to_the_device(gpu_ctx, dev, rows, got, "read")
    ms = gpu_ctx.meter_stream_open(len(rows), RATE, 40, COEF)
    try:
        fed = [0] * len(rows)
        for k in range(len(splits[0])):
            chunks = [x[fed[u]:fed[u] + (splits[u][k] if k < len(splits[u]) else 0)] for u, x in enumerate(rows)]
            feed(gpu_ctx, dev, ms, chunks)
            fed = [f + len(c) for f, c in zip(fed, chunks)]
            reading = ms.read()
            for u, (gated, hops, _, _) in enumerate(one_shot_on_device(gpu_ctx, dev, [x[:f] for x, f in zip(rows, fed)])):
                assert bits(reading[0][u]) == bits(gated) and reading[4][u] == len(hops) == fed[u] // H, (k, u)
                if len(hops) >= 4:
                    assert bits(reading[1][u]) == bits(G.loudness_window_max(hops[-4:], H, 4)), (k, u)
                if len(hops) >= 30:
                    assert bits(reading[2][u]) == bits(G.loudness_window_max(hops[-30:], H, 30)), (k, u)
        final = ms.read()
        assert [int(h) for h in final[4]] == [40, 3, 4, 29, 30]
        assert [v > 0 for v in final[0]] == [True, False, True, True, True] and [v > 0 for v in final[2]] == [True, False, False, False, True]
    finally:
        ms.close()


# ---- 9 ---------------------------------------------------------------------------------------------------------------------
def test_refusals_on_the_device(gpu_ctx, dev):
    """an ended row fed again, and a row carried past max_hops = 5: REFUSED, NaN and 0 come back, nothing is written, `read` is
    as it was, the other rows of the wave are unaffected, and a correct call may follow"""
    x = [noise(8 * H, 890 + u) for u in range(3)]
    models = [RowModel(RATE, COEF, max_hops=5) for _ in x]
    ms = gpu_ctx.meter_stream_open(3, RATE, 5, COEF)
    try:
        first = [x[0][:4 * H + 100], x[1][:300], x[2][:5 * H]]             # (row 2 fills its ledger to the brim)
        out, res = feed(gpu_ctx, dev, ms, first)
        same(out, res, [m.next(c) for m, c in zip(models, first)], "first call")
        tails = ms.finish([0, 1, 0])
        assert bits(tails[1]) == bits(models[1].finish())
        before = ms.read()
        # row 0 would complete hops 5 and 6; row 1 has ended; row 2 would complete hop 6
        second = [x[0][4 * H + 100:6 * H + 100], x[1][300:310], x[2][5 * H:6 * H]]
        want = [m.next(c) for m, c in zip(models, second)]
        assert want == [None, None, None]
        out, res = feed(gpu_ctx, dev, ms, second)
        same(out, res, want, "all refused")
        same_reading(ms.read(), [m.read() for m in models], "after the refusals")
        after = ms.read()
        assert all(np.array_equal(a.view(np.uint64), b.view(np.uint64)) for a, b in zip(before, after))
        # a correct call follows: row 0 to the brim, row 1 paused, row 2 short of a hop; row 0's neighbour refusals changed nothing
        third = [x[0][4 * H + 100:5 * H + 100], x[1][:0], x[2][5 * H:6 * H - 1]]
        want = [m.next(c) for m, c in zip(models, third)]
        assert want[0] is not None and len(want[0][0]) == 1 and len(want[2][0]) == 0
        out, res = feed(gpu_ctx, dev, ms, third)
        same(out, res, want, "the correct call")
        # one refused row beside live ones
        fourth = [x[0][5 * H + 100:5 * H + 110], x[1][:0], x[2][6 * H - 1:6 * H]]
        want = [m.next(c) for m, c in zip(models, fourth)]
        assert want[0] is not None and want[2] is None
        out, res = feed(gpu_ctx, dev, ms, fourth)
        same(out, res, want, "one refused")
        same_reading(ms.read(), [m.read() for m in models], "at the end")
        (whole,) = one_shot_on_device(gpu_ctx, dev, [x[0][:5 * H + 110]])
        assert np.array_equal(bits(ms.ledger_rows()[0]), bits(whole[1]))
    finally:
        ms.close()


def test_invalid_arguments_leave_the_stream_as_it_was(gpu_ctx, dev):
    lib = G.load()
    x = noise(2 * H, 895)
    ms = gpu_ctx.meter_stream_open(1, RATE, 4, COEF)
    other = gpu_ctx.meter_stream_open(1, RATE, 4, COEF)
    try:
        feed(gpu_ctx, dev, ms, [x[:H + 3]])
        d_in, d_len, d_hops = dev.up(x[H + 3:]), dev.up(np.array([H - 3], np.uint32)), dev.up(np.full(8, CANARY, np.float64))
        h, s = gpu_ctx.handle, ms.handle
        nothing = (None, None, None)
        bad = [lib.grail_meter_stream_next_async(h, None, d_in, 256, d_len, d_hops, 1, *nothing),
               lib.grail_meter_stream_next_async(h, C.c_void_p(0x1234), d_in, 256, d_len, d_hops, 1, *nothing),
               lib.grail_meter_stream_next_async(h, s, None, 256, d_len, d_hops, 1, *nothing),
               lib.grail_meter_stream_next_async(h, s, d_in, 256, None, d_hops, 1, *nothing),
               lib.grail_meter_stream_next_async(h, s, d_in, 257, d_len, d_hops, 1, *nothing),
               lib.grail_meter_stream_read_async(h, C.c_void_p(0x1234), None, None, None, None, None),
               lib.grail_meter_stream_finish_async(h, C.c_void_p(0x1234), None, None),
               lib.grail_meter_stream_ledger(h, s, None, None),
               lib.grail_meter_stream_close(h, C.c_void_p(0x1234))]
        assert all(rc == G.ERR_INVALID_ARG for rc in bad), bad
        for args in ((0, RATE, 4), (1, 2559, 4), (1, RATE, 0), (2, RATE, 2 ** 60)):
            handle = C.c_void_p(0x77)
            assert lib.grail_meter_stream_open(h, args[0], args[1], None, args[2], C.addressof(handle)) == G.ERR_INVALID_ARG
            assert handle.value == 0x77
        gpu_ctx.sync()
        assert np.all(dev.down(d_hops, 8, np.float64) == CANARY)
        out, res = feed(gpu_ctx, dev, ms, [x[H + 3:]])
        (want,) = one_shot_on_device(gpu_ctx, dev, [x])
        assert res[0][0] == 1 and bits(out[0, 0]) == bits(want[1][1])
    finally:
        ms.close()
        other.close()


# ---- the example -----------------------------------------------------------------------------------------------------------
def test_interactive_example_meters_what_it_writes(gpu_ctx, dev):
    """grail_interactive --band 300 3400 --ceiling -1 --rate 8000 --meter prints a report whose gated mean square and true peak
    are, to the last bit, what grail_loudness_async and grail_true_peak_async give for the track it wrote"""
    import os
    import re
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "grail-rs_amd", "lib", "grail_interactive")
    r = subprocess.run([exe, "--band", "300", "3400", "--ceiling", "-1", "--rate", "8000", "--meter", "441", "0.6"],
                       input=b"a e\n@0.3 o i a e\n", capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    track = np.frombuffer(r.stdout, np.float32)
    err = r.stderr.decode()
    m = re.search(r"Metered at 8000 Hz: (\d+) hops, gated mean square (\S+), true peak (\S+)\n", err)
    assert m and re.search(r"Track 1: integrated -?\d+\.\d\d LUFS, range .*, max momentary -?\d+\.\d\d LUFS, max short-term .*, "
                           r"true peak -?\d+\.\d\d dBTP\n", err), err
    stride = (len(track) + 63) // 64 * 64
    host = np.zeros(stride, np.float32)
    host[:len(track)] = track
    d_rows, d_len = dev.up(host), dev.up(np.array([len(track)], np.uint32))
    gated, hops, _ = gpu_ctx.loudness(d_rows, stride, d_len, 1, 8000)
    peak, _ = gpu_ctx.true_peak(d_rows, stride, d_len, 1)
    assert int(m.group(1)) == len(track) // 800 >= 4
    assert bits(float.fromhex(m.group(2))) == bits(gated[0]) and gated[0] > 0
    assert bits(float.fromhex(m.group(3))) == bits(peak[0]) and peak[0] > 0
    print(f"\n{len(track)} samples at 8 kHz: {G.loudness_lufs(gated[0]):.2f} LUFS, {G.true_peak_db(peak[0]):.2f} dBTP")


# ---- 10 --------------------------------------------------------------------------------------------------------------------
def test_interplay_with_the_other_kinds_and_with_destroy(gpu_ctx, dev):
    """a meter stream opened and closed while a limit stream is open on the same context; closing waits for queued work (the
    results of a call queued right before it are there); streams still open at grail_destroy go with the context"""
    x = noise(H + 50, 899)
    (want,) = one_shot_on_device(gpu_ctx, dev, [x])
    ls = gpu_ctx.limit_stream_open(1, 0.5, 3)
    try:
        ms = gpu_ctx.meter_stream_open(1, RATE, 4, COEF)
        d_in, d_len = dev.up(x), dev.up(np.array([len(x)], np.uint32))
        d_hops, d_n = dev.up(np.full(2, CANARY, np.float64)), dev.up(np.full(1, 77, np.uint32))
        ms.next_async(d_in, len(x), d_len, d_hops, 2, d_n)
        ms.close()
        assert dev.down(d_n, 1, np.uint32)[0] == 1 and bits(dev.down(d_hops, 2, np.float64)[0]) == bits(want[1][0])
        assert G.load().grail_meter_stream_close(gpu_ctx.handle, ls.handle) == G.ERR_INVALID_ARG       # another kind's stream
        d_out = dev.up(np.zeros(512, np.float32))
        assert ls.next(d_in, len(x), d_len, d_out, 512)[0][0] == len(x) - ls.delay
    finally:
        ls.close()
    with G.Context(gpu_ctx.device) as ctx:
        ms = ctx.meter_stream_open(2, RATE, 4)
        d = Dev(ctx)
        d_in, d_len = d.up(np.concatenate([x, x])), d.up(np.array([len(x)] * 2, np.uint32))
        n_hops, _, _ = ms.next(d_in, len(x), d_len)
        assert list(n_hops) == [1, 1]
        d.free()
