"""Limit streams on the device (grail_limit_stream_*) against the numpy model of tests/limit_stream_model.py, bit for bit in
the samples, the lengths and the three numbers of every call and of the tails: the calls' outputs end to end, then the tail,
are what grail_limit_async gives for the whole group, whatever the split.  Every output buffer holds a canary with guards
around it, the inputs hold NaN outside the rows' samples and are overwritten as soon as the call is queued: nothing is
written past out_len or outside the buffer, nothing is read past a row's samples or after the call."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import grail_hip as G
from limit_stream_model import bits, check_against_one_shot, delay, splits, stream_model
from test_levels_gpu import CANARY, Dev, dev, same_bits  # noqa: F401  (dev is a fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = G.LIMIT_CHUNK
REFUSED = 0xFFFFFFFF
CEILING = np.float32(0.5)


def at(ptr, floats):
    return C.c_void_p(ptr.value + 4 * floats)


def feed(ctx, dev, ls, chunks, stride=None, out_stride=None, in_offset=0, out_offset=0, guard=64):
    """one `next` call: chunks[i] as row i of an input buffer that holds NaN everywhere else and is overwritten as soon as the
    call is queued, the outputs into a buffer of the canary with `guard` floats of it before and after -> (out [n_rows,
    out_stride] as it lies on the device afterwards, (out_len, min_gain, n_limited, nonfinite) per group)"""
    n_rows = len(chunks)
    longest = max([len(c) for c in chunks] + [1])
    stride = stride or (longest + 63) // 64 * 64
    out_stride = stride if out_stride is None else out_stride
    host = np.full(n_rows * stride + in_offset, np.nan, np.float32)
    for i, c in enumerate(chunks):
        host[in_offset + i * stride:in_offset + i * stride + len(c)] = c
    d_in = dev.up(host)
    before = guard + out_offset
    d_out = dev.up(np.full(before + n_rows * out_stride + guard, CANARY, np.float32))
    d_len = dev.up(np.array([len(c) for c in chunks], np.uint32))
    types = (np.uint32, np.float32, np.uint32, np.uint32)
    d_res = [dev.up(np.full(ls.n_groups, 77, t)) for t in types]
    ls.next_async(at(d_in, in_offset), stride, d_len, at(d_out, before), out_stride, *d_res)
    ctx.memset(d_in, 0x7F, host.nbytes)                 # (3.4e38 everywhere: a late read would show)
    res = tuple(dev.down(p, ls.n_groups, t) for p, t in zip(d_res, types))
    out = dev.down(d_out, before + n_rows * out_stride + guard, np.float32)
    assert np.all(out[:before] == CANARY) and np.all(out[before + n_rows * out_stride:] == CANARY), "written outside out"
    return out[before:before + n_rows * out_stride].reshape(n_rows, out_stride), res


def flush(ctx, dev, ls, out_stride=None, which=None, out_offset=0, guard=64):
    """one `finish` call -> (out, (out_len, min_gain, n_limited) per group), as feed"""
    out_stride = (ls.delay + 3) // 4 * 4 if out_stride is None else out_stride
    before = guard + out_offset
    d_out = dev.up(np.full(before + ls.n_rows * out_stride + guard, CANARY, np.float32))
    res = ls.finish(at(d_out, before), out_stride, which)
    out = dev.down(d_out, before + ls.n_rows * out_stride + guard, np.float32)
    assert np.all(out[:before] == CANARY) and np.all(out[before + ls.n_rows * out_stride:] == CANARY), "written outside out"
    return out[before:before + ls.n_rows * out_stride].reshape(ls.n_rows, out_stride), res


def same(out, res, want, group, what):
    """a call's groups against the model's: want[g] = ([z per member], min_gain, n_limited[, nonfinite]), None: a refused
    group, "idle": a group the call leaves alone (0, 1.0f, 0, 0); past the outputs the canary"""
    for g, w in enumerate(want):
        rows = out[g * group:(g + 1) * group]
        if w is None:
            assert res[0][g] == REFUSED and np.isnan(res[1][g]) and res[2][g] == 0 and np.all(rows == CANARY), (what, g, "refused")
            assert len(res) < 4 or res[3][g] == 0, (what, g)
            continue
        if isinstance(w, str):
            w = ([np.zeros(0, np.float32)] * group, np.float32(1.0), 0, 0)
        n = len(w[0][0])
        assert res[0][g] == n, (what, g, res[0][g], n)
        assert np.all(rows[:, n:] == CANARY), (what, g, "written past the group's outputs")
        for j, y in enumerate(w[0]):
            differ = np.flatnonzero(bits(rows[j, :n]) != bits(y))
            assert len(differ) == 0, (what, g, j, n, differ[:8], rows[j, differ[:4]], y[differ[:4]])
        assert bits(res[1][g]) == bits(w[1]) and res[2][g] == w[2], (what, g, res[1][g], w[1], res[2][g], w[2])
        if len(res) == 4:
            assert res[3][g] == w[3], (what, g, res[3][g], w[3])


def stream_groups(ctx, dev, groups, group_splits, ell, c=CEILING, tail_stride=None, max_calls=100, **layout):
    """groups[g]: the member rows of group g, fed as group_splits[g] says (shorter splits pause at the end), then finished:
    every call and the tails against the model -> per group the members' outputs end to end"""
    group = len(groups[0])
    n_calls = max(len(s) for s in group_splits)
    assert n_calls <= max_calls
    group_splits = [list(s) + [0] * (n_calls - len(s)) for s in group_splits]
    models = [check_against_one_shot(m, c, ell, s) for m, s in zip(groups, group_splits)]
    ls = ctx.limit_stream_open(len(groups) * group, c, ell, group)
    try:
        fed = [0] * len(groups)
        joined = [[[] for _ in m] for m in groups]
        for k in range(n_calls):
            chunks = [x[fed[g]:fed[g] + group_splits[g][k]] for g, m in enumerate(groups) for x in m]
            out, res = feed(ctx, dev, ls, chunks, **layout)
            same(out, res, [m[0][k] for m in models], group, ("call", k))
            for g, m in enumerate(groups):
                for j in range(group):
                    joined[g][j].append(out[g * group + j, :res[0][g]])
                fed[g] += group_splits[g][k]
        out, res = flush(ctx, dev, ls, tail_stride, out_offset=layout.get("out_offset", 0))
        same(out, res, [m[1] for m in models], group, "tail")
        for g, m in enumerate(groups):
            for j in range(group):
                joined[g][j].append(out[g * group + j, :res[0][g]])
    finally:
        ls.close()
    return [[np.concatenate(j) for j in g] for g in joined]


def one_shot_on_device(ctx, dev, rows, c, ell, group=1):
    n = len(rows[0])
    stride = (n + 63) // 64 * 64
    host = np.full((len(rows), stride), np.nan, np.float32)
    for i, x in enumerate(rows):
        host[i, :n] = x
    d_rows, d_out = dev.up(host), dev.up(np.full((len(rows), stride), CANARY, np.float32))
    d_len = dev.up(np.full(len(rows), n, np.uint32))
    res = ctx.limit(d_rows, stride, d_len, len(rows), c, ell, d_out, group=group)
    return dev.down(d_out, (len(rows), stride), np.float32)[:, :n], res


# ---- 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ell", [0, 3, 8, 10])
def test_any_split_gives_the_one_shot_bits(gpu_ctx, dev, ell):
    """noise at 0.6 of full scale over a ceiling of 0.5, so most windows are limited, with holes; also against
    grail_limit_async itself on the device"""
    rng = np.random.default_rng(700 + ell)
    N = 2 * CHUNK + 37
    x = rng.uniform(-0.6, 0.6, N).astype(np.float32)
    x[[0, N // 2, N - 1]] = [np.nan, np.inf, -np.inf]
    device, (g1, l1, b1) = one_shot_on_device(gpu_ctx, dev, [x], CEILING, ell)
    for split in splits(N, 1 << ell, rng):
        (joined,), = stream_groups(gpu_ctx, dev, [[x]], [split], ell)
        assert same_bits(joined, device[0]), (ell, split)
    assert b1[0] == 3 and l1[0] > N // 2 and g1[0] < 1


# ---- 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ell", [0, 5, 10])
def test_hot_samples_where_the_state_can_go_wrong(gpu_ctx, dev, ell):
    """a quiet row, a call boundary at N, one sample of 0.9 at a time either side of what the detector, the known outputs and
    the ring must get right; every place is a group of its own, so one stream runs them all"""
    L, lam = 1 << ell, delay(ell)
    rng = np.random.default_rng(710 + ell)
    N = 3 * L + 64
    total = N + lam + 50
    places = [N - 12, N - 11, N - 1, N, N - lam - 1, N - lam, N - 3 * L - 19, N - 3 * L - 20]
    quiet = rng.uniform(-0.02, 0.02, total).astype(np.float32)
    rows = []
    for p in places:
        x = quiet.copy()
        x[p] = 0.9
        rows.append([x])
    # the row's end: the last sample and the sample eleven before the end hot, which shapes the tail (asserted on the model:
    # the case is not vacuous).  The issue behind this test expected the tail to differ from what feeding LAMBDA zeros and
    # cutting gives; it cannot (tests/test_limit_stream_host.py, test_the_tail_against_fed_zeros, has the argument)
    end = quiet.copy()
    end[[total - 1, total - 12]] = 0.9
    rows.append([end])
    _, tail = stream_model([end], CEILING, ell, [total])
    _, quiet_tail = stream_model([quiet], CEILING, ell, [total])
    assert tail[2] > 0 and quiet_tail[2] == 0 and tail[1] < 0.6
    joined = stream_groups(gpu_ctx, dev, rows, [[N, total - N]] * len(rows), ell)
    for (z,), (x,) in zip(joined, rows):
        assert len(z) == total and np.abs(z).max() <= CEILING and np.count_nonzero(bits(z) != bits(x)) >= 1


# ---- 3 ---------------------------------------------------------------------------------------------------------------------
def test_calls_shorter_than_the_delay(gpu_ctx, dev):
    ell, N = 5, 600
    rng = np.random.default_rng(720)
    x = rng.uniform(-0.6, 0.6, N).astype(np.float32)
    split = [7] * (N // 7) + [N % 7]
    calls, _ = stream_model([x], CEILING, ell, split)
    lens = [len(c[0][0]) for c in calls]
    assert lens[:6] == [0] * 6 and set(lens[7:-1]) == {7}
    stream_groups(gpu_ctx, dev, [[x]], [split], ell)


# ---- 4 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ell", [0, 6])
def test_short_groups(gpu_ctx, dev, ell):
    lam = delay(ell)
    rng = np.random.default_rng(730 + ell)
    lengths = [0, 1, lam - 1, lam, lam + 1]
    rows = [[rng.uniform(-0.6, 0.6, n).astype(np.float32)] for n in lengths]
    # all five as groups of one stream: each is fed its samples in the first call, the others pause
    joined = stream_groups(gpu_ctx, dev, rows, [[n] for n in lengths], ell)
    assert [len(z) for (z,) in joined] == lengths
    # a group fed nothing: out_len 0 and min_gain 1.0f from finish
    ls = gpu_ctx.limit_stream_open(1, CEILING, ell)
    try:
        out, res = flush(gpu_ctx, dev, ls)
        assert res[0][0] == 0 and bits(res[1][0]) == bits(np.float32(1.0)) and res[2][0] == 0 and np.all(out == CANARY)
    finally:
        ls.close()


def pair_short_of_its_delay():
    """-> (ell, the pair's members, the split): two calls that leave the pair short of its delay, each with a sample that is not
    finite in either member, then the rest"""
    ell = 4
    rng = np.random.default_rng(735)
    split = [10, 12, 100]
    assert split[0] + split[1] < delay(ell) < sum(split)
    members = [rng.uniform(-0.6, 0.6, sum(split)).astype(np.float32) for _ in range(2)]
    members[0][[3, 9, 10]] = [np.nan, np.inf, -np.inf]
    members[1][[0, 21, 22]] = [np.inf, np.nan, np.nan]
    return ell, members, split


def test_a_pair_fed_less_than_its_delay_counts_both_members(gpu_ctx, dev):
    """group = 2 and calls that write no output: chunk 0 runs all the same and counts what is not finite in both members (the
    `count == 0` loop over the group), which no other case reaches with more than one member"""
    ell, members, split = pair_short_of_its_delay()
    calls, _ = stream_model(members, CEILING, ell, split)
    assert [(len(k[0][0]), k[3]) for k in calls[:2]] == [(0, 3), (0, 2)] and len(calls[2][0][0]) > 0
    stream_groups(gpu_ctx, dev, [members], [split], ell)


# ---- 5 ---------------------------------------------------------------------------------------------------------------------
def test_a_window_held_at_gain_zero_across_calls(gpu_ctx, dev):
    ell = 8
    rng = np.random.default_rng(740)
    x = rng.uniform(-0.1, 0.1, 2400).astype(np.float32)
    x[1000] = 1e30
    split = [700, 200, 200, 200, 1100]          # the dip (2 L - 1 + 22 samples around 1000) spans three calls' outputs
    calls, _ = stream_model([x], CEILING, ell, split)
    assert sum(1 for c in calls if c[2] > 0) >= 3 and min(c[1] for c in calls) < 1e-6
    (joined,), = stream_groups(gpu_ctx, dev, [[x]], [split], ell)
    assert joined[1000] == 0 and np.abs(joined).max() <= CEILING          # q = 0 in every window under S[1000]


# ---- 6 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ell", [0, 6])
def test_linked_pairs_refusals_and_finishing_one_group(gpu_ctx, dev, ell):
    lam = delay(ell)
    rng = np.random.default_rng(750 + ell)
    N = 3 * lam + 200
    left = rng.uniform(-0.02, 0.02, N).astype(np.float32)
    right = left[::-1].copy()
    for p in (lam + 5, 2 * lam + 100):
        right[p] = 0.9                                                      # only the second member is hot
    other = [rng.uniform(-0.6, 0.6, N).astype(np.float32) for _ in range(2)]
    a = N // 2
    model = [check_against_one_shot(m, CEILING, ell, [a, N - a]) for m in ([left, right], other)]
    assert np.count_nonzero(bits(np.concatenate([model[0][0][0][0][0], model[0][0][1][0][0], model[0][1][0][0]])) != bits(left)) > 2
    ls = gpu_ctx.limit_stream_open(4, CEILING, ell, group=2)
    try:
        out, res = feed(gpu_ctx, dev, ls, [left[:a], right[:a], other[0][:a], other[1][:a]])
        same(out, res, [model[0][0][0], model[1][0][0]], 2, "first call")
        # group 0's members are fed different n: refused, group 1 proceeds
        out, res = feed(gpu_ctx, dev, ls, [left[a:], right[a:-1], other[0][a:], other[1][a:]])
        same(out, res, [None, model[1][0][1]], 2, "unequal members")
        # finish marks group 1 and leaves group 0 running
        out, res = flush(gpu_ctx, dev, ls, which=[0, 1])
        same(out, res, ["idle", model[1][1]], 2, "finish of group 1")
        # the correct call continues group 0 to the one-shot bits; group 1 has ended: fed, it is refused
        out, res = feed(gpu_ctx, dev, ls, [left[a:], right[a:], other[0][:5], other[1][:5]])
        same(out, res, [model[0][0][1], None], 2, "the correct call; an ended group fed")
        # ... and paused, it is left alone; a second finish ends group 0 only
        out, res = feed(gpu_ctx, dev, ls, [left[:0], right[:0], other[0][:0], other[1][:0]])
        same(out, res, ["idle", "idle"], 2, "both paused")
        out, res = flush(gpu_ctx, dev, ls)
        same(out, res, [model[0][1], "idle"], 2, "finish of the rest")
    finally:
        ls.close()


# ---- 7 ---------------------------------------------------------------------------------------------------------------------
def test_paused_groups(gpu_ctx, dev):
    ell = 4
    rng = np.random.default_rng(760)
    N = 900
    rows = [[rng.uniform(-0.6, 0.6, N).astype(np.float32)] for _ in range(2)]
    steady = [100] * 9
    halting = [0, 200, 0, 200, 0, 200, 0, 300, 0]
    stream_groups(gpu_ctx, dev, rows, [steady, halting], ell)


# ---- 8 ---------------------------------------------------------------------------------------------------------------------
LAYOUTS = {"aligned": dict(stride=2048), "odd stride": dict(stride=2049, out_stride=2051), "in off by 1": dict(stride=2048, in_offset=1),
           "out off by 3": dict(stride=2048, out_offset=3), "out wider": dict(stride=2048, out_stride=2112)}


@pytest.mark.parametrize("n_rows", [1, 63, 65])
def test_layout_and_neighbours(gpu_ctx, dev, n_rows):
    """every layout gives the same bits (16-byte and 4-byte loads and stores), with neighbours either side that are fed other
    samples; calls of 4 k and of 4 k + 1 samples, so the seam between ring and input falls on and off a group of four"""
    ell = 3
    rng = np.random.default_rng(770 + n_rows)
    N = 2000
    rows = [[rng.uniform(-0.6, 0.6, N).astype(np.float32)] for _ in range(n_rows)]
    split = [400, 401, 403, N - 1204]
    want = None
    for name, layout in LAYOUTS.items():
        joined = stream_groups(gpu_ctx, dev, rows, [split] * n_rows, ell, **layout)
        mid = joined[n_rows // 2][0]
        want = mid if want is None else want
        assert same_bits(mid, want), name


# ---- 9 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ell", [0, 8])
def test_under_the_ceiling_the_input_comes_back_delayed(gpu_ctx, dev, ell):
    lam = delay(ell)
    rng = np.random.default_rng(780 + ell)
    x = rng.uniform(-0.2, 0.2, 3000).astype(np.float32)
    x[[3, 77]] = [-0.0, 1e-45]
    ls = gpu_ctx.limit_stream_open(1, CEILING, ell)
    try:
        out, res = feed(gpu_ctx, dev, ls, [x[:1500]])
        assert res[0][0] == 1500 - lam and same_bits(out[0, :1500 - lam], x[:1500 - lam]) and res[1][0] == 1 and res[2][0] == 0
        out, res = feed(gpu_ctx, dev, ls, [x[1500:]])
        assert res[0][0] == 1500 and same_bits(out[0, :1500], x[1500 - lam:3000 - lam])
        out, res = flush(gpu_ctx, dev, ls)
        assert res[0][0] == lam and same_bits(out[0, :lam], x[3000 - lam:]) and res[1][0] == 1
    finally:
        ls.close()


# ---- 10 --------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_leave_outputs_and_state_untouched(gpu_ctx, dev):
    ell = 4
    rng = np.random.default_rng(790)
    x = rng.uniform(-0.6, 0.6, 1000).astype(np.float32)
    calls, tail = check_against_one_shot([x], CEILING, ell, [500, 500])
    lib = G.load()
    ls = gpu_ctx.limit_stream_open(1, CEILING, ell)
    other = gpu_ctx.limit_stream_open(1, CEILING, ell)
    try:
        out, res = feed(gpu_ctx, dev, ls, [x[:500]])
        same(out, res, [calls[0]], 1, "first call")
        d_in, d_len = dev.up(x[500:]), dev.up(np.array([500], np.uint32))
        d_out = dev.up(np.full(1024, CANARY, np.float32))
        h, s = gpu_ctx.handle, ls.handle
        bad = [lib.grail_limit_stream_next_async(h, None, d_in, 500, d_len, d_out, 512, None, None, None, None),
               lib.grail_limit_stream_next_async(h, C.c_void_p(0x1234), d_in, 500, d_len, d_out, 512, None, None, None, None),
               lib.grail_limit_stream_next_async(h, s, None, 500, d_len, d_out, 512, None, None, None, None),
               lib.grail_limit_stream_next_async(h, s, d_in, 500, None, d_out, 512, None, None, None, None),
               lib.grail_limit_stream_next_async(h, s, d_in, 500, d_len, None, 512, None, None, None, None),
               lib.grail_limit_stream_next_async(h, s, d_in, 500, d_len, d_out, 499, None, None, None, None),
               lib.grail_limit_stream_next_async(h, s, d_in, 500, d_len, d_in, 500, None, None, None, None),
               lib.grail_limit_stream_finish_async(h, s, None, d_out, delay(ell) - 1, None, None, None),
               lib.grail_limit_stream_finish_async(h, s, None, None, 64, None, None, None),
               lib.grail_limit_stream_finish_async(h, C.c_void_p(0x1234), None, d_out, 64, None, None, None),
               lib.grail_limit_stream_close(h, C.c_void_p(0x1234))]
        assert all(rc == G.ERR_INVALID_ARG for rc in bad), bad
        gpu_ctx.sync()
        assert np.all(dev.down(d_out, 1024, np.float32) == CANARY)
        for args in ((0, 1, 0.5, 4), (3, 2, 0.5, 4), (2, 0, 0.5, 4), (1, 1, 0.0, 4), (1, 1, float("nan"), 4), (1, 1, 0.5, 11)):
            handle = C.c_void_p(0x77)
            assert lib.grail_limit_stream_open(h, args[0], args[1], args[2], args[3], C.addressof(handle)) == G.ERR_INVALID_ARG
            assert handle.value == 0x77
        out, res = feed(gpu_ctx, dev, ls, [x[500:]])
        same(out, res, [calls[1]], 1, "the call after the refusals")
        out, res = flush(gpu_ctx, dev, ls)
        same(out, res, [tail], 1, "tail")
    finally:
        ls.close()
        other.close()


def test_two_finishing_calls_with_marks_queued_back_to_back(gpu_ctx, dev):
    """two `finish` calls with marks, their results left on the device, and no wait between them: the second writes the
    stream's host copy of the marks anew, which the first's upload may not have read yet, so it waits for the event behind that
    upload.  The first unit's tail comes from the first call alone and the others' from the second; behind what the feeding
    call wrote they are the one-shot rows"""
    ell, n, n_rows, group = 2, 40, 4, 2
    rng = np.random.default_rng(795)
    rows = [rng.uniform(-0.6, 0.6, n).astype(np.float32) for _ in range(n_rows)]
    stride, guard, marks = (delay(ell) + 3) // 4 * 4, 64, ([1, 0], [0, 1])
    ls = gpu_ctx.limit_stream_open(n_rows, CEILING, ell, group)
    try:
        out, res = feed(gpu_ctx, dev, ls, rows)
        joined = [[out[i, :res[0][i // group]]] for i in range(n_rows)]
        d_outs = [dev.up(np.full(guard + n_rows * stride + guard, CANARY, np.float32)) for _ in range(2)]
        d_lens = [dev.up(np.full(n_rows // group, 77, np.uint32)) for _ in range(2)]
        for d_out, d_len, which in zip(d_outs, d_lens, marks):
            ls.finish_async(at(d_out, guard), stride, which, d_len)
        gpu_ctx.sync()
        lens = [dev.down(p, n_rows // group, np.uint32) for p in d_lens]
        assert lens[0][0] > 0 and not lens[0][1:].any() and lens[1][0] == 0 and lens[1][1:].all(), lens
        for d_out, out_len in zip(d_outs, lens):
            flat = dev.down(d_out, guard + n_rows * stride + guard, np.float32)
            out = flat[guard:guard + n_rows * stride].reshape(n_rows, stride)
            assert np.all(flat[:guard] == CANARY) and np.all(flat[guard + n_rows * stride:] == CANARY), "written outside out"
            for i in range(n_rows):
                assert np.all(out[i, out_len[i // group]:] == CANARY), (i, "written past the row's tail")
                joined[i].append(out[i, :out_len[i // group]])
    finally:
        ls.close()
    for g in range(n_rows // group):
        device, _ = one_shot_on_device(gpu_ctx, dev, rows[g * group:(g + 1) * group], CEILING, ell, group)
        for j in range(group):
            assert same_bits(np.concatenate(joined[g * group + j]), device[j]), (g, j)


# ---- 11 --------------------------------------------------------------------------------------------------------------------
def test_interactive_example_limits_what_it_renders(gpu_ctx, dev):
    """grail_interactive --ceiling -6 --lookahead 8 on a short script writes what the same run without the option writes,
    limited afterwards by grail_limit_async in one piece; and again at -30 dBTP and the default look-ahead, a ceiling the
    voice is certain to be above"""
    exe = os.path.join(ROOT, "grail-rs_amd", "lib", "grail_interactive")
    script = b"a e\n@0.3 o i\n"

    def run(extra):
        r = subprocess.run([exe] + extra + ["441", "0.2"], input=script, capture_output=True, timeout=120)
        assert r.returncode == 0, r.stderr
        return np.frombuffer(r.stdout, np.float32), r.stderr

    x, _ = run([])
    assert len(x) > 4000
    for extra, ceiling_db, ell in ((["--ceiling", "-6", "--lookahead", "8"], -6.0, 8), (["--ceiling", "-30"], -30.0, 8)):
        z, err = run(extra)
        c = G.limit_ceiling(ceiling_db)
        device, (min_gain, n_limited, _) = one_shot_on_device(gpu_ctx, dev, [x], c, ell)
        assert len(z) == len(x) and same_bits(z, device[0]) and np.abs(z).max() <= c, extra
        assert b"%d samples late" % delay(ell) in err
        print(f"\n{extra}: the session peaks at {np.abs(x).max():.4f}, ceiling {c:.4f}, {n_limited[0]} samples limited, min gain {min_gain[0]:.4f}")
    assert n_limited[0] > 0 and np.abs(x).max() > c
