"""The look-ahead limiter on the device (grail_limit_async) against the numpy model of tests/test_limiter_host.py, bit for
bit in the limited samples, the smallest gain and both counts: hot samples at the seams of the kernel's chunks and at the
edges of the look-ahead window and of the halo, short rows, divisions that land next to an integer, linked pairs, rows
under the ceiling, whatever lies around or behind a row; a mix of overlapping speech; the example; one full-size batch."""
import ctypes as C
import os
import re
import subprocess
import wave

import numpy as np
import pytest

import grail_hip as G
from grail_hip import workload as W
from test_levels_gpu import CANARY, Dev, _place, dev, same_bits  # noqa: F401  (dev is a fixture)
from test_limiter_host import Q, REFUSED, bound_of, limiter_model
from test_true_peak_host import db, true_peak_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = G.LIMIT_CHUNK
ELLS = list(range(11))
SUM_LOG2 = 7                # limiter_kernels.hip's LIMIT_SUM_LOG2 (test_kernel_paths_host.py): the deficits of 2^7 minima are summed in
#                             32 bits, the L >> 7 pieces of a longer window in 64 bits at the apply


def _quiet(rng, n, scale=0.02):
    return (rng.standard_normal(n) * scale).astype(np.float32)


def _run(ctx, dev, rows, c, ell, group=1, stride=None, out_stride=None, in_offset=0, out_offset=0, fill=np.nan, lens=None):
    """rows[i] as row i of a buffer that holds `fill` everywhere else, limited into a buffer that holds CANARY
    -> (out [n_rows, out_stride] as it lies on the device afterwards, min_gain, n_limited, nonfinite)"""
    longest = max([len(x) for x in rows] + [1])
    stride = stride or (longest + 63) // 64 * 64
    out_stride = out_stride or stride
    host = np.full(len(rows) * stride + in_offset, fill, np.float32)
    for i, x in enumerate(rows):
        host[in_offset + i * stride:in_offset + i * stride + len(x)] = x
    d_in = dev.up(host)
    d_out = dev.up(np.full(len(rows) * out_stride + out_offset, CANARY, np.float32))
    d_len = dev.up(np.array([len(x) for x in rows] if lens is None else lens, np.uint32))
    stats = ctx.limit(C.c_void_p(d_in.value + in_offset * 4), stride, d_len, len(rows), c, ell,
                      C.c_void_p(d_out.value + out_offset * 4), out_stride, group)
    out = dev.down(d_out, len(rows) * out_stride + out_offset, np.float32)
    assert np.all(out[:out_offset] == CANARY)
    return (out[out_offset:].reshape(len(rows), out_stride),) + stats


def _same(rows, got, want, what):
    """the device's (out, min_gain, n_limited, nonfinite) against the model's; out rows hold the canary past their samples
    and throughout where the model gives None (a refused group)"""
    out, min_gain, n_limited, bad = got
    w_out, w_gain, w_limited, w_bad = want[:4]
    assert same_bits(min_gain, w_gain), (what, min_gain, w_gain)
    assert np.array_equal(n_limited, w_limited), (what, n_limited, w_limited)
    assert np.array_equal(bad, w_bad), (what, bad, w_bad)
    for i, z in enumerate(w_out):
        n = 0 if z is None else len(z)
        assert np.all(out[i, n:] == CANARY), (what, i, "written past the row's samples")
        if n:
            differ = np.flatnonzero(out[i, :n].view(np.uint32) != z.view(np.uint32))
            assert len(differ) == 0, (what, i, n, differ[:8], out[i, differ[:4]], z[differ[:4]])


def _seam_row(rng, n, L, hot=0.9):
    """quiet noise with hot samples at 0, n - 1, every chunk seam and the samples either side of it, L + 11 and L + 12 before
    and after each seam (the halo's edge), and pairs L - 1, L and L + 1 apart (the window's edges)"""
    x = _quiet(rng, n)
    at = {0, n - 1}
    for seam in range(T, n + 1, T):
        at |= {seam - 1, seam, seam + 1, seam - L - 11, seam - L - 12, seam + L + 10, seam + L + 11, seam - 2 * L - 10, seam - L}
    base = T // 3
    for k, gap in enumerate((L - 1, L, L + 1)):
        at |= {base + k * (3 * L + 40), base + k * (3 * L + 40) + gap}
    for p in sorted(p for p in at if 0 <= p < n):
        x[p] = np.float32(hot * (1.0 + 0.37 * rng.random()) * (-1.0) ** p)
    return x


# ---- seams and the look-ahead's reach -------------------------------------------------------------------------------------
@pytest.mark.parametrize("ell", ELLS)
def test_hot_samples_at_the_seams_and_at_the_windows_edges(gpu_ctx, dev, ell):
    """rows of T - 1, T, T + 1 and 2 T + L + 3 samples, NaN between a row's samples and the stride, a NaN and an infinite
    sample in the longest"""
    L = 1 << ell
    rng = np.random.default_rng(100 + ell)
    rows = [_seam_row(rng, n, L) for n in (T - 1, T, T + 1, 2 * T + L + 3)]
    rows[3][[T - 2, 2 * T + 2]] = [np.nan, -np.inf]
    c = np.float32(0.25)
    want = limiter_model(rows, c, ell)
    assert np.all(want[2] > 20) and want[3][3] == 2 and np.all(want[1] < 0.5)
    _same(rows, _run(gpu_ctx, dev, rows, c, ell), want, f"L = {L}")


@pytest.mark.parametrize("ell", ELLS)
def test_short_rows(gpu_ctx, dev, ell):
    """n = 0, 1, 11, 12, L - 1, L, L + 1: rows shorter than the filter, than the window, and just as long"""
    L = 1 << ell
    rng = np.random.default_rng(200 + ell)
    rows = []
    for n in sorted({0, 1, 11, 12, max(L - 1, 0), L, L + 1}):
        for hot_at in ((), (0,), (n - 1,), (n // 2, n - 1)):
            x = _quiet(rng, n)
            for p in hot_at:
                if 0 <= p < n:
                    x[p] = np.float32(0.7 + rng.random())
            rows.append(x)
    c = np.float32(0.3)
    want = limiter_model(rows, c, ell)
    assert np.count_nonzero(want[2]) > len(rows) // 2
    _same(rows, _run(gpu_ctx, dev, rows, c, ell), want, f"L = {L}")
    # rows of no samples at all: 1.0f, 0, 0, and a NULL input is fine
    d_len = dev.up(np.zeros(3, np.uint32))
    min_gain, n_limited, bad = gpu_ctx.limit(None, 0, d_len, 3, c, ell, None, 0)
    assert np.all(min_gain == 1) and not n_limited.any() and not bad.any()


# ---- the sum of the deficits at its bound ----------------------------------------------------------------------------------
_held = {}


def _held_at_zero(ell):
    """(row, c, what the model says of it), once per ell: quiet noise of T + 2 L + 40 samples with a run of 2 L + 30 samples
    of +-3e38 (finite, alternating in sign) from T - L - 5 on, across the chunk seam: q = 0 for longer than two windows, so
    every minimum of a whole window is 0, its deficits sum to L Q, and the gain is 0 for more than a window"""
    if ell not in _held:
        L = 1 << ell
        rng = np.random.default_rng(800 + ell)
        x = _quiet(rng, T + 2 * L + 40)
        run = np.full(2 * L + 30, 3e38, np.float32)
        run[1::2] = -run[1::2]
        x[T - L - 5:T - L - 5 + len(run)] = run
        assert np.all(np.isfinite(x)) and T - L - 5 + len(run) > T + L
        x.setflags(write=False)
        c = np.float32(0.25)
        _held[ell] = (x, c, limiter_model([x], c, ell, curves=True))
    return _held[ell]


@pytest.mark.parametrize("ell", [7, 8, 9, 10])
def test_a_window_held_at_gain_zero(gpu_ctx, dev, ell):
    """the deficits of a whole window at their largest, L Q: at ell = 7 the 32-bit sum holds 2^7 deficits of 2^24 (2^31, what
    LIMIT_SUM_LOG2 is sized for), at ell = 8, 9 and 10 the apply adds 2, 4 and 8 such pieces in 64 bits"""
    L = 1 << ell
    x, c, want = _held_at_zero(ell)
    out, min_gain, n_limited, bad, ((q, S, g),) = want
    assert ell >= SUM_LOG2 and L >> SUM_LOG2 == (1, 2, 4, 8)[ell - 7]
    assert min_gain[0] == 0.0 and bad[0] == 0 and np.count_nonzero(out[0] == 0) > 2 * L
    assert S.min() == 0 and np.count_nonzero(S == 0) > L                   # the sum of the deficits reached L Q, its bound
    assert n_limited[0] > 4 * L and np.all(np.abs(out[0]) <= c)
    _same([x], _run(gpu_ctx, dev, [x], c, ell), want, f"L = {L}")


@pytest.mark.parametrize("layout", ["aligned", "offset1"])
def test_a_window_held_at_gain_zero_by_the_third_member_of_a_group(gpu_ctx, dev, layout):
    """group = 3 at ell = 7: the members' q's are folded by minimum twice; the run is in the last member, the others are
    quiet and come out at gain zero where it is"""
    ell = SUM_LOG2
    x, c, alone = _held_at_zero(ell)
    rng = np.random.default_rng(807)
    rows = [_quiet(rng, len(x)), _quiet(rng, len(x)), x, _quiet(rng, 900), _seam_row(rng, 900, 1 << ell), _quiet(rng, 900)]
    want = limiter_model(rows, c, ell, group=3)
    assert want[1][0] == 0.0 and want[3][0] == 0 and all(np.count_nonzero(want[0][j] == 0) > 2 << ell for j in range(3))
    assert want[2][0] >= alone[2][0] and 0 < want[1][1] < 1
    _same(rows, _run(gpu_ctx, dev, rows, c, ell, group=3, **({} if layout == "aligned" else dict(in_offset=1))), want, layout)


# ---- the division ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ell", [0, 3])
def test_divisions_that_land_next_to_an_integer(gpu_ctx, dev, ell):
    """lone samples d = c Q / k for integers k, rounded to the float below and the float above (and the exact one where there
    is one), 64 samples apart: c Q / d lies within one of k, on either side, and the floor decides.  A lone sample's d is
    its own magnitude (the centre tap is 7964 / 8192), and at L <= 8 each dip stands alone, so out shows every q."""
    rng = np.random.default_rng(300 + ell)
    c = np.float32(0.3)
    ks = np.concatenate([rng.integers(Q // 16, Q, 700), [Q - 1, Q - 2, Q // 2, Q // 4, Q // 2 + 1, 3 * (Q // 4), Q // 16]])
    exact = float(c) * Q / ks
    below = exact.astype(np.float32)
    below = np.where(below.astype(np.float64) > exact, np.nextafter(below, np.float32(0.0)), below)
    above = np.nextafter(below, np.float32(np.inf))
    hot = np.concatenate([below, above]).astype(np.float32)
    hot[::2] = -hot[::2]
    x = np.zeros(64 * len(hot) + 40, np.float32)
    x[32:32 + 64 * len(hot):64] = hot
    want = limiter_model([x], c, ell, curves=True)
    q = want[4][0][0][32:32 + 64 * len(hot):64]
    near = np.abs(np.concatenate([ks, ks]) - q)
    assert near.max() <= 2 and len(np.unique(near)) >= 2 and np.count_nonzero(q == Q) < len(q) // 20
    _same([x], _run(gpu_ctx, dev, [x], c, ell), want, f"L = {1 << ell}")


# ---- groups ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ell", [0, 6])
def test_linked_pairs_and_a_refused_pair(gpu_ctx, dev, ell):
    """group = 2: a hot sample in one channel only dips both channels by the same curve; a pair of unequal lengths is flagged
    (NaN, GRAIL_LIMIT_REFUSED, 0) and its out rows keep the canary; the pairs around it are served"""
    rng = np.random.default_rng(400 + ell)
    n = T + 300
    left, right = _quiet(rng, n), _quiet(rng, n)
    left[[T - 3, T + 200]] = [0.95, -0.8]
    rows = [left, right, _seam_row(rng, 900, 1 << ell), _quiet(rng, 899), right, left, _quiet(rng, 0), _quiet(rng, 0)]
    c = np.float32(0.25)
    want = limiter_model(rows, c, ell, group=2, curves=True)
    assert want[0][2] is None and want[0][3] is None and want[2][1] == REFUSED and want[2][0] > 0
    got = _run(gpu_ctx, dev, rows, c, ell, group=2)
    _same(rows, got, want, f"L = {1 << ell}")
    assert np.isnan(got[1][1]) and got[2][1] == G.LIMIT_REFUSED and got[3][1] == 0
    g = want[4][0][2]
    assert same_bits(got[0][1, :n], g * right) and np.count_nonzero(got[0][1, :n] != right) >= 2 * (1 << ell)
    assert same_bits(got[0][4, :n], got[0][1, :n]) and same_bits(got[0][5, :n], got[0][0, :n])      # the order of the members
    # group = 4 over the same rows: the first four differ in length
    got4 = _run(gpu_ctx, dev, rows, c, ell, group=4)
    _same(rows, got4, limiter_model(rows, c, ell, group=4), "group = 4")
    assert got4[2][0] == G.LIMIT_REFUSED and np.isnan(got4[1][0]) and np.all(got4[0][:4] == CANARY)


# ---- layout and launch independence -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def awkward():
    """one row of 2 T + 67 samples with hot samples at its seams, NaN and +-Inf, -0.0 and denormals, and what the model says
    of it at L = 64"""
    rng = np.random.default_rng(500)
    x = _seam_row(rng, 2 * T + 67, 64)
    x[[5, T + 1, 2 * T + 60]] = [np.nan, np.inf, -np.inf]
    x[[9, 10, 11]] = [-0.0, 1e-45, -3e-39]
    c = np.float32(0.25)
    return dict(row=x, c=c, ell=6, model=limiter_model([x], c, 6))


@pytest.mark.parametrize("layout", ["stride4", "odd", "offset1", "offset3", "out_wider"])
def test_a_rows_result_does_not_depend_on_its_layout(gpu_ctx, dev, awkward, layout):
    """row_stride a multiple of 4 and odd; rows_dev 1 float and out_dev 3 floats past an aligned address (4-byte loads and
    stores instead of 16-byte ones); out_stride above row_stride; two short rows beside the row"""
    x, c, ell = awkward["row"], awkward["c"], awkward["ell"]
    rng = np.random.default_rng(501)
    rows = [_seam_row(rng, 700, 64), x, _quiet(rng, 13)]
    want = limiter_model(rows, c, ell)
    assert same_bits(want[0][1], awkward["model"][0][0])
    n = len(x)
    kw = {"stride4": dict(stride=(n + 3) // 4 * 4), "odd": dict(stride=(n + 3) // 4 * 4 + 1), "offset1": dict(in_offset=1),
          "offset3": dict(out_offset=3), "out_wider": dict(stride=(n + 3) // 4 * 4, out_stride=(n + 3) // 4 * 4 + 8)}[layout]
    _same(rows, _run(gpu_ctx, dev, rows, c, ell, **kw), want, layout)


@pytest.mark.parametrize("n_total", [1, 63, 65])
def test_a_rows_result_does_not_depend_on_the_rows_around_it(gpu_ctx, dev, awkward, n_total):
    x, c, ell = awkward["row"], awkward["c"], awkward["ell"]
    rng = np.random.default_rng(n_total)
    pos = int(rng.integers(0, n_total))
    stride = (len(x) + 63) // 64 * 64
    rows_dev, d_len, lens = _place(gpu_ctx, dev, [x], [pos], n_total, stride, 0, rng)
    d_out = dev.up(np.full(n_total * stride, CANARY, np.float32))
    min_gain, n_limited, bad = gpu_ctx.limit(rows_dev, stride, d_len, n_total, c, ell, d_out, stride)
    out = dev.down(d_out, (n_total, stride), np.float32)
    (z,), w_gain, w_limited, w_bad = awkward["model"]
    assert same_bits(out[pos, :len(x)], z) and np.all(out[pos, len(x):] == CANARY)
    assert same_bits(min_gain[pos:pos + 1], w_gain) and n_limited[pos] == w_limited[0] and bad[pos] == w_bad[0]
    # the other rows hold 0x3c3c3c3c samples (0.0115, under the ceiling) over a random length: they come back as they are
    const = np.frombuffer(b"\x3c" * 4, np.float32)[0]
    for k in np.setdiff1d(np.arange(n_total), [pos]):
        assert np.all(out[k, :lens[k]] == const) and np.all(out[k, lens[k]:] == CANARY), k
        assert min_gain[k] == 1 and n_limited[k] == 0 and bad[k] == 0


@pytest.mark.parametrize("stride", [T + 8, T + 5])
def test_a_len_above_row_stride_reads_as_row_stride(gpu_ctx, dev, stride):
    rng = np.random.default_rng(stride)
    rows = [_seam_row(rng, stride, 16) for _ in range(3)]
    c = np.float32(0.25)
    got = _run(gpu_ctx, dev, rows, c, 4, stride=stride, lens=[stride + 1, 0xFFFFFFFF, stride])
    _same(rows, got, limiter_model(rows, c, 4), stride)


# ---- nothing to do -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ell", [0, 8])
def test_rows_under_the_ceiling_come_back_bit_for_bit(gpu_ctx, dev, ell):
    """the chunk's fast path: no number above the ceiling in reach, so the rows are copied (a non-finite sample as +0.0)"""
    rng = np.random.default_rng(600 + ell)
    rows = [_quiet(rng, n, 0.05) for n in (0, 1, T, 2 * T + 5, 10001)]
    rows[3][[0, 7, T, 2 * T + 4]] = [-0.0, 1e-45, -3e-39, np.nan]
    c = np.float32(0.6)                                                     # 12 sigma: above what the taps can make of the noise
    got = _run(gpu_ctx, dev, rows, c, ell)
    _same(rows, got, limiter_model(rows, c, ell), f"L = {1 << ell}")
    assert not got[2].any() and np.all(got[1] == 1) and got[3][3] == 1
    for i, x in enumerate(rows):
        keep = np.isfinite(x)
        assert same_bits(got[0][i, :len(x)][keep], x[keep])
    # one chunk of a row hot, its neighbours not: both paths in one row
    x = _quiet(rng, 3 * T, 0.05)
    x[T + T // 2] = 0.9
    _same([x], _run(gpu_ctx, dev, [x], c, ell), limiter_model([x], c, ell), "one hot chunk")


def test_invalid_arguments_leave_the_output_untouched(gpu_ctx, dev):
    rng = np.random.default_rng(700)
    x = _seam_row(rng, 1000, 16)
    d_in, d_len = dev.up(x), dev.up(np.array([1000], np.uint32))
    d_out = dev.up(np.full(1000, CANARY, np.float32))
    for kw in (dict(ell=11), dict(group=0), dict(group=2), dict(c=0.0), dict(c=float("nan")), dict(c=float("inf")),
               dict(out=d_in), dict(out=C.c_void_p(d_in.value + 999 * 4)), dict(out_stride=999)):
        a = dict(c=0.25, ell=4, group=1, out=d_out, out_stride=1000)
        a.update(kw)
        with pytest.raises(G.GrailError) as ei:
            gpu_ctx.limit_async(d_in, 1000, d_len, 1, a["c"], a["ell"], a["out"], a["out_stride"], a["group"])
        assert ei.value.status == G.ERR_INVALID_ARG, kw
    gpu_ctx.sync()
    assert np.all(dev.down(d_out, 1000, np.float32) == CANARY) and same_bits(dev.down(d_in, 1000, np.float32), x)
    gpu_ctx.limit_async(d_in, 1000, d_len, 1, 0.25, 4, d_out)             # no result asked for: the rows alone
    gpu_ctx.sync()
    assert same_bits(dev.down(d_out, 1000, np.float32), limiter_model([x], 0.25, 4)[0][0])


# ---- real output -----------------------------------------------------------------------------------------------------------
def test_overlapping_speech_is_held_under_the_ceiling(gpu_ctx, dev):
    """eight speech-like rows at 8 kHz, mixed by grail_batch_mix_leveled_limited to a ceiling that binds every item, with
    items overlapping on both tracks (one of each twice at the same place): the per-item ceiling cannot hold the sum, the
    tracks' true peaks are above c.  The tracks limited as one linked pair at L = 256: the model's bits, |z| <= c exactly,
    and the true peak within the header's bound; the overshoot is printed for DESIGN.md."""
    rate = 8000
    n = 8
    gpu_ctx.set_voices(W.preset_voices(2, sample_rate=rate))
    segs, offs, vids, seeds, stride = W.speech_like_batch(n, np.random.default_rng(71), n_voices=2, sample_rate=rate)
    b = gpu_ctx.upload(segs, offs, vids, seeds)
    try:
        lens = b.lengths()
        item_rows = np.array([0, 0, 1, 2, 3, 4, 4, 5, 6, 7], np.uint32)
        item_tracks = np.array([0, 0, 0, 0, 0, 1, 1, 1, 1, 1], np.uint32)
        item_offs = np.array([0, 0, 700, 1500, 4000, 0, 0, 300, 900, 5000], np.uint64)
        track_len = int((item_offs + lens[item_rows]).max())
        track_stride = (track_len + 63) // 64 * 64
        ceiling_db = -12.0
        c = G.limit_ceiling(ceiling_db)
        d_t = dev.alloc(2 * track_stride * 4)
        _, gains, unleveled, limited = b.mix_leveled_limited(item_rows, item_offs, np.full(len(item_rows), -14.0, np.float32), d_t,
                                                             track_stride, 2, track_len, item_tracks=item_tracks, mode=G.LEVEL_RMS,
                                                             ceiling_db=ceiling_db)
        assert unleveled == 0 and limited >= 2
        d_len = dev.up(np.array([track_len, track_len], np.uint32))
        before, _ = gpu_ctx.true_peak(d_t, track_stride, d_len, 2)
        assert np.all(before > float(c)), before                           # the case the per-item ceiling cannot hold
        d_z = dev.up(np.full(2 * track_stride, CANARY, np.float32))
        min_gain, n_limited, bad = gpu_ctx.limit(d_t, track_stride, d_len, 2, c, 8, d_z, track_stride, group=2)
        after, _ = gpu_ctx.true_peak(d_z, track_stride, d_len, 2)
    finally:
        b.free()
    tracks = dev.down(d_t, (2, track_stride), np.float32)[:, :track_len]
    z = dev.down(d_z, (2, track_stride), np.float32)
    want = limiter_model([tracks[0], tracks[1]], c, 8, group=2)
    _same(None, (z, min_gain, n_limited, bad), want, "tracks")
    z = z[:, :track_len]
    assert np.all(np.abs(z) <= c) and bad[0] == 0 and n_limited[0] > 0 and min_gain[0] < 1
    for t in range(2):
        assert after[t] == true_peak_model(z[t])[0]
        assert after[t] <= bound_of(c, 8, tracks[t]), (t, after[t])
    over = db(after.max() / float(c))
    print(f"\ntracks of {track_len} samples at {db(before[0]):+.3f} and {db(before[1]):+.3f} dBTP, ceiling {ceiling_db} dBTP, L = 256: "
          f"{n_limited[0]} samples limited, smallest gain {min_gain[0]:.4f}; after: {db(after[0]):+.5f} and {db(after[1]):+.5f} dBTP, "
          f"overshoot {over:+.5f} dB against c (bound {db(bound_of(c, 8, tracks[0]) / float(c)):+.3f} dB)")
    kept = np.count_nonzero(z.view(np.uint32) == tracks.view(np.uint32)) / z.size
    print(f"{100 * kept:.1f} % of the samples pass unchanged")


# ---- the example ---------------------------------------------------------------------------------------------------------
def _wav(path):
    with wave.open(str(path), "rb") as w:
        assert w.getsampwidth() == 2
        return np.frombuffer(w.readframes(w.getnframes()), np.int16).reshape(-1, w.getnchannels())


def test_grail_dialogue_limit_option(gpu_ctx, tmp_path):
    """--lufs -16 --ceiling -9 --limit: exit status 0, the line it prints, every sample of the WAV within c; without --limit
    the program prints no such line and writes the file it writes on a second run without it"""
    exe = os.path.join(ROOT, "grail-rs_amd", "lib", "grail_dialogue")
    lines = ["hello there", "a fine day to you"]
    common = ["--lufs", "-16", "--ceiling", "-9"]
    r = subprocess.run([exe, "-o", str(tmp_path / "held.wav")] + common + ["--limit"] + lines, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"Limiter, (\d+) samples of look-ahead: (\d+) samples limited, smallest gain (\S+); track true peaks (\S+) and "
                  r"(\S+) dBTP before, (\S+) and (\S+) dBTP after", r.stdout)
    assert m, r.stdout
    print("\n" + m.group(0))
    assert int(m.group(1)) == 128                                           # the largest power of two within 44 100 / 200
    c = G.limit_ceiling(-9.0)
    held = _wav(tmp_path / "held.wav")
    assert held.shape[1] == 2 and np.abs(held.astype(np.int64)).max() <= int(np.ceil(float(c) * 32768.0))
    assert max(float(m.group(6)), float(m.group(7))) <= -9.0 + 0.01         # (measured overshoots are thousandths of a dB)
    plain = [subprocess.run([exe, "-o", str(tmp_path / f"plain{i}.wav")] + common + lines, capture_output=True, text=True, timeout=300)
             for i in range(2)]
    assert all(p.returncode == 0 and "Limiter" not in p.stdout for p in plain)
    assert plain[0].stdout.replace("plain0", "plain1") == plain[1].stdout
    assert (tmp_path / "plain0.wav").read_bytes() == (tmp_path / "plain1.wav").read_bytes()
    # what --limit prints before its own line, and everything but the samples, is what the plain run gives
    assert r.stdout.replace(m.group(0) + "\n", "").replace("held", "plain0") == plain[0].stdout
    assert _wav(tmp_path / "plain0.wav").shape == held.shape
    assert float(m.group(4)) == pytest.approx(float(re.search(r"track true peaks (\S+) and", plain[0].stdout).group(1)))


# ---- full size: config 3 -------------------------------------------------------------------------------------------------
def test_full_size(gpu_ctx, dev):
    """65 536 x 96 006 rendered rows as 32 768 linked pairs, the ceiling at half the median sample peak of the sounding
    rows, so that most sounding pairs are limited: per pair the numbers and 4 000 sampled
    positions of 24 pairs spread over the batch (first, last, workgroup boundaries, random) equal the model over the
    downloaded rows; every pair's smallest gain is consistent with its count"""
    n = 65536
    gpu_ctx.set_voices(W.single_voice())
    segs, offs, vids, seeds = W.make_batch(n)
    stride = W.max_samples()
    b = gpu_ctx.upload(segs, offs, vids, seeds)
    try:
        d_rows, d_len, d_out = dev.alloc(n * stride * 4), dev.alloc(n * 4), dev.alloc(n * stride * 4)
        d_gain, d_lim, d_bad, d_peak = (dev.alloc(n * 4) for _ in range(4))
        gpu_ctx.memset(d_rows, 0xFF, n * stride * 4)                       # NaNs until the rendering has run
        b.synthesize_async(d_rows, stride, d_len)
        gpu_ctx.levels_async(d_rows, stride, d_len, n, peak_dev=d_peak)
        gpu_ctx.sync()
        peak = dev.down(d_peak, n, np.float32)
        c = np.float32(np.median(peak[peak > 0]) / 2.0)
        gpu_ctx.limit_async(d_rows, stride, d_len, n, c, 8, d_out, stride, 2, d_gain, d_lim, d_bad)
        gpu_ctx.sync()
    finally:
        b.free()
    groups = n // 2
    min_gain, n_limited = dev.down(d_gain, groups, np.float32), dev.down(d_lim, groups, np.uint32)
    bad, lens = dev.down(d_bad, groups, np.uint32), dev.down(d_len, n, np.uint32)
    assert np.all(lens == 96006) and not bad.any()
    # (a deficit too small for binary32 still counts as limited: a gain of 1.0f does not say that nothing was)
    assert np.all(n_limited[min_gain < 1] > 0) and np.all(min_gain[n_limited == 0] == 1)
    assert np.all(min_gain > 0) and np.all(min_gain <= 1) and np.all(n_limited <= 96006)
    assert np.count_nonzero(n_limited) > groups // 8
    pair_peak = np.maximum(peak[0::2], peak[1::2])
    assert np.all(n_limited[pair_peak > c] > 0)
    print(f"\n{np.count_nonzero(n_limited)} of {groups} pairs limited at c = {float(c):.4f}: smallest gain {min_gain.min():.4f}, "
          f"{int(n_limited.astype(np.int64).sum())} samples limited")
    rng = np.random.default_rng(4)
    fixed = [0, groups - 1, 1, 127, 128, 4095, 4096, 16383]
    sample = fixed + [int(u) for u in rng.permutation(groups) if u not in fixed][:16]
    for u in sample:
        pair = [dev.down(d_rows, 96006, np.float32, offset=(2 * u + j) * stride * 4) for j in range(2)]
        out, w_gain, w_limited, w_bad = limiter_model(pair, c, 8, group=2)
        assert same_bits(min_gain[u:u + 1], w_gain) and n_limited[u] == w_limited[0] and w_bad[0] == 0, u
        at = np.unique(np.concatenate([rng.integers(0, 96006, 3900), np.arange(0, 96006, T)[1:], np.arange(0, 96006, T)[1:] - 1,
                                       [0, 96005]]))
        for j in range(2):
            z = dev.down(d_out, 96006, np.float32, offset=(2 * u + j) * stride * 4)
            assert same_bits(z[at], out[j][at]), (u, j)
