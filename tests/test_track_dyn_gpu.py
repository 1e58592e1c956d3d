"""Dynamics with a workgroup a row (grail_track_dyn_async) against the numpy model of tests/dyn_model.py, bit for bit in the
samples, the lengths, the non-finite counts and min_gain, as tests/test_dyn_gpu.py holds grail_dyn_async: the call is no
contract of its own.  The shapes are the new kernel's: with T = TRACK_TILE read from dyn_plan.h, rows of every length either
side of one, two, three and five tiles (the three-stage pipeline fills, runs full and drains) in calls of 1, 2, 13 and 70 rows;
non-finite samples at a tile's first sample, its last, in between and in the last, partial tile; outputs cut inside a tile and
exactly on a tile's edge with the row's smallest gain behind the cut; the 4-byte path against the 16-byte one; keys that end
inside a tile and keys longer than their rows; keys of no samples; refused rows; gains that compare equal with different sign bits in different
lanes and tiles; a row of 300 001 samples against grail_dyn_async on the same buffers; the calls that queue nothing; and the
dialogue example with --compress-tracks.  Every output buffer holds a canary wherever nothing may be written."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dyn_model as M
import grail_hip as G
from test_dyn_gpu import audio, edge_samples, same, same_bits, sets, staircase, three_curves  # noqa: F401  (sets is a fixture)
from test_dyn_gpu import variant as dyn_variant
from test_levels_gpu import CANARY, Dev, dev  # noqa: F401  (dev is a fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = int(re.search(r"constexpr uint32_t TRACK_TILE = (\d+);", open(os.path.join(ROOT, "grail-rs_amd", "csrc", "dyn_plan.h")).read()).group(1))
LENGTHS = [0, 1, 63, 64, 65, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 3 * T + 5, 5 * T + 1]
# track_env_kernel<VEC, KEYED>: the four that tests/test_track_dyn_code_objects.py finds in the library
VARIANTS = [(vec, keyed) for vec in (True, False) for keyed in (False, True)]


def variant(in_offset=0, stride=0, out_offset=0, out_stride=0, keyed=False, key_offset=0, key_stride=0):
    """the track_env_kernel<VEC, KEYED> that launch_track_dyn starts: test_dyn_gpu.variant's rule without the streams"""
    return dyn_variant(in_offset, stride, out_offset, out_stride, keyed, key_offset, key_stride)[:2]


def pad64(n):
    return (max(n, 1) + 63) // 64 * 64


def run(ctx, dev, dyn_set, rows, which=None, keys=None, key_row=None, key_lens=None, stride=None, out_stride=None, in_offset=0,
        out_offset=0, key_stride=None, key_offset=0, guard=64, lens=None, call="track_dyn", self_key=False):
    """test_dyn_gpu.run through Context.track_dyn (call="dyn": through Context.dyn): rows[i] as row i of a buffer that holds NaN
    everywhere else (keys[j] likewise), into a buffer that holds CANARY with `guard` floats of it before and after -> (out
    [n_rows, out_stride] as it lies on the device afterwards, out_len, nonfinite, min_gain).  self_key: key_dev = rows_dev."""
    longest = max([len(x) for x in rows] + [1])
    stride = stride or pad64(longest)
    out_stride = pad64(longest) if out_stride is None else out_stride
    host = np.full(len(rows) * stride + in_offset, np.nan, np.float32)
    for i, x in enumerate(rows):
        host[in_offset + i * stride:in_offset + i * stride + len(x)] = x
    d_in = C.c_void_p(dev.up(host).value + in_offset * 4)
    before = guard + out_offset
    d_out = dev.up(np.full(before + len(rows) * out_stride + guard, CANARY, np.float32))
    d_len = dev.up(np.array([len(x) for x in rows] if lens is None else lens, np.uint32))
    d_which = None if which is None else dev.up(np.array(which, np.uint32))
    kw = {}
    if self_key:
        kw = dict(key_dev=d_in, key_stride=stride, n_keys=len(rows), key_len_dev=d_len, key_row_dev=None)
    elif keys is not None:
        key_stride = pad64(max([len(k) for k in keys] + [1])) if key_stride is None else key_stride
        khost = np.full(max(len(keys) * key_stride + key_offset, 4), np.nan, np.float32)          # (key_stride 0: keys of no samples)
        for j, k in enumerate(keys):
            khost[key_offset + j * key_stride:key_offset + j * key_stride + len(k)] = k
        kw = dict(key_dev=C.c_void_p(dev.up(khost).value + key_offset * 4), key_stride=key_stride, n_keys=len(keys),
                  key_len_dev=None if key_lens is None else dev.up(np.array(key_lens, np.uint32)),
                  key_row_dev=None if key_row is None else dev.up(np.array(key_row, np.uint32)))
    out_len, bad, mg = getattr(ctx, call)(dyn_set, d_in, stride, d_len, len(rows), d_which, C.c_void_p(d_out.value + before * 4), out_stride, **kw)
    out = dev.down(d_out, before + len(rows) * out_stride + guard, np.float32)
    assert np.all(out[:before] == CANARY) and np.all(out[before + len(rows) * out_stride:] == CANARY), "written outside out"
    return out[before:before + len(rows) * out_stride].reshape(len(rows), out_stride), out_len, bad, mg


def gain_bits(x):
    return int(np.float64(x).view(np.uint64))


# ---- rows and lengths: the pipeline fills, runs full and drains ---------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed():
    """70 rows of the lengths above on the three curves, two of them refused, with the model's answer: computed once, read by
    every row count below (a row's numbers do not depend on the rows around it)"""
    rng = np.random.default_rng(70)
    rows = [audio(LENGTHS[(i * 5 + 12) % len(LENGTHS)], rng) for i in range(70)]
    which = [int(v) for v in rng.integers(0, 3, 70)]
    which[4], which[40] = 3, 0xFFFFFFFF
    assert sorted({len(x) for x in rows[:13]}) == sorted(LENGTHS) and len(rows[0]) == 5 * T + 1
    return rows, which, M.dyn_model(rows, three_curves(), which)


@pytest.mark.parametrize("n_rows", [1, 2, 13, 70])
def test_row_counts_and_lengths_either_side_of_the_tiles(gpu_ctx, dev, sets, mixed, n_rows):
    rows, which, want = mixed
    assert n_rows < 13 or [w[1] == M.REFUSED for w in want[:13]].count(True) == 1
    same(want[:n_rows], run(gpu_ctx, dev, sets(three_curves()), rows[:n_rows], which[:n_rows]), n_rows)


def test_curve_dev_null_is_curve_0_and_a_len_beyond_the_stride_is_the_stride(gpu_ctx, dev, sets):
    rng = np.random.default_rng(3)
    curves = three_curves()
    rows = [audio(n, rng) for n in (2 * T, T + 100, 2 * T, 0)]
    dyn_set = sets(curves)
    same(M.dyn_model(rows, curves), run(gpu_ctx, dev, dyn_set, rows), "curve_dev NULL")
    lens = [5 * T, T + 100, 0xFFFFFFFF, 0]
    want = M.dyn_model(rows, curves, [2, 1, 0, 2], lens=lens)
    same(want, run(gpu_ctx, dev, dyn_set, rows, [2, 1, 0, 2], stride=2 * T, out_stride=2 * T + 64, lens=lens), "len > row_stride")
    assert [w[1] for w in want] == [2 * T, T + 100, 2 * T, 0] and want[3][3] == 1.0


def test_the_scalar_path_gives_the_aligned_paths_bits(gpu_ctx, dev, sets):
    """a stride that is no multiple of 4 with a base 4 bytes off 16-byte alignment takes the 4-byte loads and stores; each side
    misaligned alone too"""
    rng = np.random.default_rng(6)
    curves = three_curves()
    rows = [audio(n, rng) for n in (2 * T + 1, T - 1, 0, 17, T, 2 * T + 9, T + 1)]
    rows[1][[0, 500]] = (np.inf, np.nan)
    which = [0, 1, 1, 2, 1, 2, 0]
    dyn_set = sets(curves)
    want = M.dyn_model(rows, curves, which)
    wide, odd = 2 * T + 64, 2 * T + 9
    aligned = run(gpu_ctx, dev, dyn_set, rows, which, stride=wide, out_stride=wide)
    same(want, aligned, "aligned")
    for kw in (dict(in_offset=1, stride=odd, out_offset=1, out_stride=odd), dict(in_offset=1, stride=wide, out_stride=wide),
               dict(stride=odd, out_stride=wide), dict(stride=wide, out_offset=3, out_stride=wide), dict(stride=wide, out_stride=odd + 1)):
        got = run(gpu_ctx, dev, dyn_set, rows, which, **kw)
        same(want, got, kw)
        for i, (y, n_out, _, _) in enumerate(want):
            same_bits(got[0][i, :n_out], aligned[0][i, :n_out], (kw, i))


# ---- non-finite samples and cut outputs ------------------------------------------------------------------------------------------
def test_nonfinite_samples_at_a_tiles_ends_and_in_the_last_partial_tile(gpu_ctx, dev, sets):
    rng = np.random.default_rng(7)
    curves = three_curves()
    n = 2 * T + 100
    rows = [audio(n, rng) for _ in range(3)] + [audio(T, rng)]
    at = [0, 5, T - 1, T, T + 500, 2 * T - 1, 2 * T, 2 * T + 50, n - 1]       # a tile's first, its last, in between, the last tile
    rows[0][at] = np.nan
    rows[1][at[::2]], rows[1][at[1::2]] = np.inf, -np.inf
    rows[3][[0, T - 1]] = np.nan
    want = M.dyn_model(rows, curves, [0, 1, 2, 2])
    assert [w[2] for w in want] == [len(at), len(at), 0, 2]
    got = run(gpu_ctx, dev, sets(curves), rows, [0, 1, 2, 2])
    same(want, got, "non-finite")
    assert np.all(got[0][0, at].view(np.uint32) == 0)          # (their outputs are +0.0)


@pytest.fixture(scope="module")
def cut_rows():
    rng = np.random.default_rng(8)
    n = 2 * T + 200
    rows = [audio(n, rng), audio(T, rng), audio(3, rng), audio(0, rng), audio(n, rng)]
    rows[0][2 * T + 150], rows[4][n - 1] = np.nan, -np.inf       # (past the cut of every stride below n)
    rows[4][2 * T + 100:] *= np.float32(64.0)                    # ... and the row's smallest gain with them
    which = [0, 1, 2, 0, 0]
    return rows, which, M.dyn_model(rows, three_curves(), which)


@pytest.mark.parametrize("out_stride", [0, 100, T, T + 100, 2 * T, 2 * T + 256])
def test_out_stride_cuts_the_outputs_and_nothing_else(gpu_ctx, dev, sets, cut_rows, out_stride):
    """out_stride 0 (the results only, out_dev NULL), below n inside a tile and exactly on a tile's edge, and above n: min_gain
    and nonfinite are over all n samples, and the smallest gain of row 4 lies behind every cut"""
    rows, which, whole = cut_rows
    want = [(w[0][:min(w[1], out_stride)], min(w[1], out_stride), w[2], w[3]) for w in whole]
    assert whole[0][2] == 1 and whole[4][2] == 1
    at_cut = M.dyn_model([rows[4][:2 * T + 100]], three_curves(), [0])[0][3]
    assert whole[4][3] < at_cut                                  # (the model's smallest gain lies behind the cuts)
    dyn_set = sets(three_curves())
    stride = 2 * T + 256
    if out_stride == 0:
        d_in = dev.up(np.concatenate([np.concatenate([x, np.full(stride - len(x), np.nan, np.float32)]) for x in rows]))
        d_len = dev.up(np.array([len(x) for x in rows], np.uint32))
        out_len, bad, mg = gpu_ctx.track_dyn(dyn_set, d_in, stride, d_len, 5, dev.up(np.array(which, np.uint32)), None, 0)
        for i, w in enumerate(want):
            assert (out_len[i], bad[i]) == (0, w[2]) and gain_bits(mg[i]) == gain_bits(w[3]), i
        return
    same(want, run(gpu_ctx, dev, dyn_set, rows, which, stride=stride, out_stride=out_stride), out_stride)


# ---- alphas and the lookup's edges --------------------------------------------------------------------------------------------
def test_alphas_of_zero_and_an_attack_far_below_the_release(gpu_ctx, dev, sets):
    rng = np.random.default_rng(10)
    comp = G.dyn_design(G.DYN_COMPRESS, G.DYN_PEAK, -30.0, 8.0, 0.0, 0.0, 0.0)
    curves = [(comp, (0.0, 0.0), G.DYN_PEAK), (staircase(), (0.0, 0.0), G.DYN_SQUARE),
              (comp, G.dyn_ballistics(48000, 0.05, 400.0), G.DYN_PEAK), (staircase(), (0.0, 0.999), G.DYN_PEAK)]
    n = 2 * T + 77
    rows = [audio(n, rng), audio(n, rng), audio(n, rng), audio(n, rng), np.full(T + 200, 0.3, np.float32), np.full(T + 200, -0.3, np.float32)]
    which = [0, 1, 2, 3, 0, 1]
    want = M.dyn_model(rows, curves, which)
    same(want, run(gpu_ctx, dev, sets(curves), rows, which), "alphas")
    assert len(set(want[5][0].view(np.uint32).tolist())) == 1     # the staircase at alpha = 0 on a constant: one gain


def test_samples_on_the_lookups_edges(gpu_ctx, dev, sets):
    """test_dyn_gpu's edge samples (every lev[k] and its neighbours, below 2^-32 and at it, 2^8 and above, +-0.0, denormals, NaN,
    +-Inf: over two tiles of them) on the caller's staircase G[k] = k with alpha = 0, and riding a release across the table's
    lower end"""
    x = edge_samples()
    assert len(x) > 2 * T
    rng = np.random.default_rng(12)
    gate = G.dyn_design(G.DYN_EXPAND, G.DYN_PEAK, -150.0, 2.0, 10.0, 60.0, 0.0)
    curves = [(staircase(), (0.0, 0.0), G.DYN_PEAK), (staircase(), (0.0, 0.0), G.DYN_SQUARE), (gate, (0.0, 0.5), G.DYN_PEAK),
              (staircase(), (0.5, 0.96875), G.DYN_SQUARE)]
    rows = [x, x, x, x, rng.permutation(x), rng.permutation(x)]
    which = [0, 1, 2, 3, 0, 1]
    want = M.dyn_model(rows, curves, which)
    same(want, run(gpu_ctx, dev, sets(curves), rows, which), "edges")
    k = 37
    at = int(np.flatnonzero(np.abs(x) == np.float32(M.LEVELS[k]))[0])
    assert want[0][2] == 3 and want[0][0][at] == np.float32(k * float(x[at]))


# ---- keys ---------------------------------------------------------------------------------------------------------------------
def test_keys_that_end_inside_a_tile_and_keys_longer_than_their_rows(gpu_ctx, dev, sets):
    rng = np.random.default_rng(13)
    curves = three_curves()
    rows = [audio(n, rng) for n in (2 * T + 200, T + 129, 64, 2 * T + 300, 1, 0, 200)]
    keys = [audio(n, rng) for n in (T + 100, 2 * T + 300, 64, 0)]
    keys[0][[2, T - 1, T]], keys[1][7] = (np.nan, -np.inf, np.nan), np.inf
    which = [0, 1, 2, 0, 1, 2, 0]
    key_row = [0, 1, 2, 1, 3, 0, 4]                              # rows 1 and 3 on key 1; row 6 on a key that is not there
    dyn_set = sets(curves)
    want = M.dyn_model(rows, curves, which, keys=keys, key_row=key_row)
    assert want[6][1] == M.REFUSED and want[0][2] == 0          # (a key's non-finite samples are not counted)
    same(want, run(gpu_ctx, dev, dyn_set, rows, which, keys=keys, key_row=key_row, key_lens=[len(k) for k in keys]), "keyed")
    # key_len_dev holds more than the stride, and less than the key: the key is min(key_len, key_stride) long
    ks = 2 * T + 320
    padded = [np.concatenate([k, np.zeros(ks - len(k), np.float32)]) for k in keys]
    want = M.dyn_model(rows, curves, which, keys=padded, key_row=key_row, key_lens=[ks, T + 10, ks, 0])
    same(want, run(gpu_ctx, dev, dyn_set, rows, which, keys=padded, key_row=key_row, key_lens=[5 * T, T + 10, 0xFFFFFFFF, 0], key_stride=ks),
         "key_len")
    # key_len_dev NULL, key_row_dev NULL: row u listens to the whole of key u
    seven = [audio(ks, rng) for _ in range(7)]
    want = M.dyn_model(rows, curves, which, keys=seven)
    same(want, run(gpu_ctx, dev, dyn_set, rows, which, keys=seven), "key NULLs")
    # the scalar path: an odd key stride with a base 4 bytes off, rows and out aligned
    odd = [np.concatenate([k, np.zeros(1, np.float32)]) for k in seven]
    same(M.dyn_model(rows, curves, which, keys=odd), run(gpu_ctx, dev, dyn_set, rows, which, keys=odd, key_stride=ks + 1, key_offset=1),
         "key scalar")


def test_a_row_may_be_its_own_key(gpu_ctx, dev, sets):
    """key_dev = rows_dev itself, key u for row u, is the self-keyed call, bit for bit"""
    rng = np.random.default_rng(14)
    curves = three_curves()
    rows = [audio(n, rng) for n in (2 * T + 200, 65, T)]
    rows[0][T] = np.nan
    dyn_set = sets(curves)
    want = M.dyn_model(rows, curves, [0, 1, 2])
    same(want, run(gpu_ctx, dev, dyn_set, rows, [0, 1, 2]), "self-keyed")
    same(want, run(gpu_ctx, dev, dyn_set, rows, [0, 1, 2], self_key=True), "keyed by rows_dev")


def test_keys_of_no_samples(gpu_ctx, dev, sets):
    """key_stride 0 (keys of no samples): `key_loads` is false, no worker loads a key sample, every one reads +0.0 and the gain
    is the curve's at e = +0.0 over one tile, two and a partial third, on either path.  No other case runs the keyed kernel
    without a key load."""
    rng = np.random.default_rng(16)
    curves = three_curves()
    rows = [audio(n, rng) for n in (2 * T + 77, T, 0, 65)]
    rows[0][T] = np.nan
    which = [0, 1, 2, 2]
    nothing = [np.zeros(0, np.float32)]
    want = M.dyn_model(rows, curves, which, keys=nothing, key_row=[0] * 4)
    at_rest = [float(np.asarray(curves[c][0], np.float64)[0]) for c in which]          # (e = +0.0 lies below the table: G[0] itself)
    assert [w[3] for w in want] == [g if len(x) else 1.0 for g, x in zip(at_rest, rows)]
    dyn_set = sets(curves)
    wide = 2 * T + 128
    for kw, vec in ((dict(stride=wide, out_stride=wide), True), (dict(stride=wide, out_stride=wide, out_offset=1), False)):
        assert variant(0, wide, kw.get("out_offset", 0), wide, True, 0, 0) == (vec, True)
        same(want, run(gpu_ctx, dev, dyn_set, rows, which, keys=nothing, key_row=[0] * 4, key_stride=0, **kw), ("no key samples", kw))


# ---- gains that compare equal ------------------------------------------------------------------------------------------------
def test_the_first_of_equal_gains_is_returned_with_its_sign(gpu_ctx, dev, sets):
    """Alphas 0 on the peak detector, so e[t] = |x[t]| and each sample picks its own gain.  The curve is -0.0 on its lowest
    points, +0.0 on its highest and 1.0 between; below 2^-32 the gain is G[0] itself and from 2^8 on G[640] itself.  Row 0 meets
    its first zero gain as -0.0 late in tile 0, in the last worker's samples, and a +0.0 at the first sample of tile 2, which is
    the first worker's; row 1 is the mirror image.  -0.0 == +0.0, so only the time says which is the row's min_gain."""
    gain = np.ones(M.POINTS)
    gain[:8], gain[-8:] = -0.0, 0.0
    curves = [(gain, (0.0, 0.0), G.DYN_PEAK)]
    n = 2 * T + 300
    late, early = T - 3, 2 * T
    rows = [np.full(n, 0.5, np.float32), np.full(n, 0.5, np.float32)]
    rows[0][late], rows[0][early] = 0.0, 300.0
    rows[1][late], rows[1][early] = 300.0, 0.0
    want = M.dyn_model(rows, curves)
    # the model tells them apart: a test that it could not would show nothing
    assert gain_bits(want[0][3]) == 1 << 63 and gain_bits(want[1][3]) == 0
    got = run(gpu_ctx, dev, sets(curves), rows)
    same(want, got, "equal gains")
    assert [gain_bits(g) for g in got[3]] == [1 << 63, 0]


# ---- a long row against the one-lane call ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("keyed", [False, True])
def test_a_long_row_is_grail_dyn_asyncs_on_the_same_buffers(gpu_ctx, dev, sets, keyed):
    """300 001 samples (293 tiles): the host model is too slow for it, the one-lane kernel is not, and it is held to the model
    by tests/test_dyn_gpu.py"""
    rng = np.random.default_rng(15 + keyed)
    n = 300_001
    stride = pad64(n)
    x = audio(n, rng)
    x[[0, 100_000, n - 1]] = (np.nan, np.inf, -np.inf)
    host = np.full(2 * stride, np.nan, np.float32)
    host[:n], host[stride:stride + n - 5000] = x, audio(n - 5000, rng)      # (row 1, the key, ends inside the row's last tiles)
    d_in = dev.up(host)
    d_len = dev.up(np.array([n, n - 5000], np.uint32))
    kw = dict(key_dev=C.c_void_p(d_in.value + 4 * stride), key_stride=stride, key_len_dev=C.c_void_p(d_len.value + 4), n_keys=1) if keyed else {}
    dyn_set = sets(three_curves())
    results = []
    for call in (gpu_ctx.dyn, gpu_ctx.track_dyn):
        d_out = dev.up(np.full(stride + 128, CANARY, np.float32))
        res = call(dyn_set, d_in, stride, d_len, 1, None, C.c_void_p(d_out.value + 4 * 64), stride, **kw)
        results.append((dev.down(d_out, stride + 128, np.float32), res))
    (lane_out, lane_res), (group_out, group_res) = results
    assert np.array_equal(lane_out.view(np.uint32), group_out.view(np.uint32))
    assert np.all(group_out[:64] == CANARY) and np.all(group_out[64 + n:] == CANARY) and not np.any(group_out[64:64 + n] == CANARY)
    assert (lane_res[0][0], lane_res[1][0]) == (group_res[0][0], group_res[1][0]) == (n, 3)
    assert gain_bits(lane_res[2][0]) == gain_bits(group_res[2][0]) and 0.0 < group_res[2][0] < 1.0


# ---- the calls that have nothing to do -------------------------------------------------------------------------------------------
def test_trivial_calls(gpu_ctx, dev, sets):
    dyn_set = sets(three_curves())
    d_any = dev.up(np.zeros(64, np.float32))
    out_len, bad, mg = gpu_ctx.track_dyn(dyn_set, d_any, 64, d_any, 0, None, d_any, 64)
    assert len(out_len) == len(bad) == len(mg) == 0
    d_len = dev.up(np.array([5, 0, 7], np.uint32))
    gpu_ctx.track_dyn_async(dyn_set, None, 0, d_len, 3, None, None, 0)         # rows of no samples, and nobody asks
    out_len, bad, mg = gpu_ctx.track_dyn(dyn_set, None, 0, d_len, 3, dev.up(np.array([0, 9, 2], np.uint32)), None, 0)
    assert out_len.tolist() == [0, M.REFUSED, 0] and bad.tolist() == [0, 0, 0]
    assert mg[0] == mg[2] == 1.0 and gain_bits(mg[1]) == 0x7FF8000000000000


def test_a_set_of_another_context_is_refused(gpu_ctx, dev, sets):
    other = G.Context(0)
    try:
        theirs = other.dyn_create(three_curves())
        d_any = dev.up(np.zeros(128, np.float32))
        with pytest.raises(G.GrailError, match="grail_track_dyn_async: not a curve set of this context"):
            gpu_ctx.track_dyn_async(theirs, d_any, 64, d_any, 1, None, C.c_void_p(d_any.value + 256), 64)
        other.dyn_free(theirs)
    finally:
        other.close()


# ---- the example ----------------------------------------------------------------------------------------------------------------
def test_dialogue_example_compresses_tracks_to_the_same_wav(gpu_ctx, tmp_path):
    exe = os.path.join(ROOT, "grail-rs_amd", "lib", "grail_dialogue")
    wavs = []
    for flag in ([], ["--compress-tracks"]):
        wav = tmp_path / ("tracks.wav" if flag else "lanes.wav")
        r = subprocess.run([exe, "-o", str(wav), "--lufs", "-23", "--compress", "-24:3:6:5:120"] + flag +
                           ["a e i o u a e i o u", "o u a e i o u a e i"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        name = "grail_track_dyn_async" if flag else "grail_dyn_async"
        assert re.search(r"Compressed \(%s\) above -24 dB at 3:1, knee 6 dB, attack 5 ms, release 120 ms" % name, r.stdout), r.stdout
        wavs.append(wav.read_bytes())
    assert len(wavs[0]) > 44 and wavs[0] == wavs[1]
