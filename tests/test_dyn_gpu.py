"""Dynamics on the device (grail_dyn_async) against the numpy model of tests/dyn_model.py, bit for bit in the samples, the
lengths, the non-finite counts and min_gain (a refused row's NaN compared as NaN), nothing excluded: partial last waves, rows
of every length either side of a tile mixed in one wave, the scalar path against the aligned one, out_stride 0, below and
above a row, three curves with both detectors in one wave (a compressor, an expander with a range, and the caller's own
staircase G[k] = k, on which a wrong k or f shows in every bit), refused rows, alphas of 0 and an attack far below the release,
samples aimed at every edge of the lookup, and keyed calls: keys shorter and longer than their rows, key_len_dev NULL, two rows
on one key, a key index outside, non-finite key samples, keys of no samples, and a bed ducked under voices.  Every output buffer holds a canary
wherever nothing may be written, and is checked there."""
import ctypes as C

import numpy as np
import pytest

import dyn_model as M
import grail_hip as G
from test_levels_gpu import CANARY, Dev, dev  # noqa: F401  (dev is a fixture)

pytestmark = pytest.mark.gpu
LENGTHS = [0, 1, 3, 63, 64, 65, 127, 128, 129, 200, 1000]
# dyn_kernel<VEC, KEYED, STREAM>: the eight that tests/test_dyn_code_objects.py finds in the library
VARIANTS = [(vec, keyed, stream) for vec in (True, False) for keyed in (False, True) for stream in (False, True)]


def variant(in_offset=0, stride=0, out_offset=0, out_stride=0, keyed=False, key_offset=0, key_stride=0, stream=False):
    """the dyn_kernel<VEC, KEYED, STREAM> that launch_dyn starts: VEC by aligned16 over rows and out and, keyed, over the key
    (the offsets are floats from a 16-byte aligned base).  keyed: the call brings a key_dev: a keyed stream's call of no
    samples (in_stride 0) does not, and runs the unkeyed kernel."""
    vec = in_offset % 4 == 0 and stride % 4 == 0 and out_offset % 4 == 0 and out_stride % 4 == 0
    if keyed:
        vec = vec and key_offset % 4 == 0 and key_stride % 4 == 0
    return (vec, keyed, stream)


def staircase():
    return np.arange(M.POINTS, dtype=np.float64)


def three_curves():
    """a compressor on the peak, an expander with a range on the square, the caller's staircase"""
    comp = G.dyn_design(G.DYN_COMPRESS, G.DYN_PEAK, -24.0, 4.0, 6.0, 0.0, 3.0)
    gate = G.dyn_design(G.DYN_EXPAND, G.DYN_SQUARE, -40.0, 3.0, 4.0, 30.0, 0.0)
    return [(comp, G.dyn_ballistics(48000, 1.0, 50.0), G.DYN_PEAK), (gate, G.dyn_ballistics(48000, 0.2, 5.0), G.DYN_SQUARE),
            (staircase(), (0.25, 0.875), G.DYN_PEAK)]


def audio(n, rng):
    """samples whose levels wander over ten octaves, so that the envelope crosses many points of a curve"""
    return (rng.uniform(-1.0, 1.0, n) * 2.0 ** rng.uniform(-9.0, 1.0, n)).astype(np.float32)


def run(ctx, dev, dyn_set, rows, which=None, keys=None, key_row=None, key_lens=None, stride=None, out_stride=None, in_offset=0,
        out_offset=0, key_stride=None, key_offset=0, guard=64, lens=None):
    """rows[i] as row i of a buffer that holds NaN everywhere else (keys[j] likewise), through curve which[i] of the set (None:
    curve_dev NULL), keyed by key key_row[i] (None: key_row_dev NULL; key_lens None: key_len_dev NULL), into a buffer that
    holds CANARY with `guard` floats of it before and after -> (out [n_rows, out_stride] as it lies on the device afterwards,
    out_len, nonfinite, min_gain)."""
    longest = max([len(x) for x in rows] + [1])
    stride = stride or (longest + 63) // 64 * 64
    out_stride = (longest + 63) // 64 * 64 if out_stride is None else out_stride
    host = np.full(len(rows) * stride + in_offset, np.nan, np.float32)
    for i, x in enumerate(rows):
        host[in_offset + i * stride:in_offset + i * stride + len(x)] = x
    d_in = dev.up(host)
    before = guard + out_offset
    d_out = dev.up(np.full(before + len(rows) * out_stride + guard, CANARY, np.float32))
    d_len = dev.up(np.array([len(x) for x in rows] if lens is None else lens, np.uint32))
    d_which = None if which is None else dev.up(np.array(which, np.uint32))
    kw = {}
    if keys is not None:
        key_stride = (max([len(k) for k in keys] + [1]) + 63) // 64 * 64 if key_stride is None else key_stride
        khost = np.full(max(len(keys) * key_stride + key_offset, 4), np.nan, np.float32)          # (key_stride 0: keys of no samples)
        for j, k in enumerate(keys):
            khost[key_offset + j * key_stride:key_offset + j * key_stride + len(k)] = k
        kw = dict(key_dev=C.c_void_p(dev.up(khost).value + key_offset * 4), key_stride=key_stride, n_keys=len(keys),
                  key_len_dev=None if key_lens is None else dev.up(np.array(key_lens, np.uint32)),
                  key_row_dev=None if key_row is None else dev.up(np.array(key_row, np.uint32)))
    out_len, bad, mg = ctx.dyn(dyn_set, C.c_void_p(d_in.value + in_offset * 4), stride, d_len, len(rows), d_which,
                               C.c_void_p(d_out.value + before * 4), out_stride, **kw)
    out = dev.down(d_out, before + len(rows) * out_stride + guard, np.float32)
    assert np.all(out[:before] == CANARY) and np.all(out[before + len(rows) * out_stride:] == CANARY), "written outside out"
    return out[before:before + len(rows) * out_stride].reshape(len(rows), out_stride), out_len, bad, mg


def same_bits(got, want, what):
    differ = np.flatnonzero(np.asarray(got, np.float32).view(np.uint32) != np.asarray(want, np.float32).view(np.uint32))
    assert len(differ) == 0, (what, differ[:8], got[differ[:4]], want[differ[:4]])


def same(want, got, what):
    """the device's (out, out_len, nonfinite, min_gain) against the model's rows; out rows hold the canary past their outputs;
    a refused row holds nothing else and reads (REFUSED, 0, NaN)"""
    out, out_len, bad, mg = got
    for i, (y, n_out, w_bad, w_mg) in enumerate(want):
        assert (out_len[i], bad[i]) == (n_out, w_bad), (what, i, out_len[i], n_out, bad[i], w_bad)
        if n_out == M.REFUSED:
            assert np.all(out[i] == CANARY) and np.isnan(mg[i]), (what, i, "a refused row")
            continue
        assert np.float64(mg[i]).view(np.uint64) == np.float64(w_mg).view(np.uint64), (what, i, mg[i], w_mg)
        assert np.all(out[i, n_out:] == CANARY), (what, i, "written past the row's outputs")
        same_bits(out[i, :n_out], y, (what, i))
    return want


@pytest.fixture
def sets(gpu_ctx):
    made = []

    def create(curves):
        made.append(gpu_ctx.dyn_create(curves))
        return made[-1]
    yield create
    for s in made:
        gpu_ctx.dyn_free(s)


# ---- rows and lengths ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 130])
def test_row_counts_and_lengths_mixed_within_a_wave(gpu_ctx, dev, sets, n_rows):
    """whole and partial last waves, every length of LENGTHS among a wave's rows, the three curves dealt over them"""
    rng = np.random.default_rng(n_rows)
    curves = three_curves()
    rows = [audio(LENGTHS[(i * 7 + n_rows) % len(LENGTHS)], rng) for i in range(n_rows)]
    rows[-1] = audio(1000, rng)
    which = rng.integers(0, 3, n_rows).tolist()
    same(M.dyn_model(rows, curves, which), run(gpu_ctx, dev, sets(curves), rows, which), n_rows)


def test_curve_dev_null_is_curve_0_and_a_len_beyond_the_stride_is_the_stride(gpu_ctx, dev, sets):
    rng = np.random.default_rng(3)
    curves = three_curves()
    rows = [audio(n, rng) for n in (128, 100, 128, 0)]
    dyn_set = sets(curves)
    same(M.dyn_model(rows, curves), run(gpu_ctx, dev, dyn_set, rows), "curve_dev NULL")
    lens = [5000, 100, 0xFFFFFFFF, 0]
    want = M.dyn_model(rows, curves, [2, 1, 0, 2], lens=lens)
    same(want, run(gpu_ctx, dev, dyn_set, rows, [2, 1, 0, 2], stride=128, out_stride=192, lens=lens), "len > row_stride")
    assert [w[1] for w in want] == [128, 100, 128, 0] and want[3][3] == 1.0


def test_the_scalar_path_gives_the_aligned_paths_bits(gpu_ctx, dev, sets):
    """a stride of 1001 with a base 4 bytes off 16-byte alignment takes the 4-byte loads and stores; each side alone too"""
    rng = np.random.default_rng(6)
    curves = three_curves()
    rows = [audio(n, rng) for n in (1000, 999, 0, 17, 64, 1001, 129)]
    rows[1][[0, 500]] = (np.inf, np.nan)
    which = [0, 1, 1, 2, 1, 2, 0]
    dyn_set = sets(curves)
    want = M.dyn_model(rows, curves, which)
    aligned = run(gpu_ctx, dev, dyn_set, rows, which, stride=1024, out_stride=1024)
    same(want, aligned, "aligned")
    for kw in (dict(in_offset=1, stride=1001, out_offset=1, out_stride=1001), dict(in_offset=1, stride=1024, out_stride=1024),
               dict(stride=1001, out_stride=1024), dict(stride=1024, out_offset=3, out_stride=1024), dict(stride=1024, out_stride=1002)):
        got = run(gpu_ctx, dev, dyn_set, rows, which, **kw)
        same(want, got, kw)
        for i, (y, n_out, _, _) in enumerate(want):
            same_bits(got[0][i, :n_out], aligned[0][i, :n_out], (kw, i))


@pytest.mark.parametrize("out_stride", [0, 4, 100, 130, 256])
def test_out_stride_cuts_the_outputs_and_nothing_else(gpu_ctx, dev, sets, out_stride):
    """out_stride 0 (the results only, out_dev NULL), below n and above it: min_gain and nonfinite are over all n samples"""
    rng = np.random.default_rng(8)
    curves = three_curves()
    rows = [audio(n, rng) for n in (129, 64, 3, 0, 200)]
    rows[0][120], rows[4][199] = np.nan, -np.inf                  # (past the cut of the smaller strides)
    rows[4][150:] *= np.float32(64.0)                            # ... and the row's smallest gain with them
    which = [0, 1, 2, 0, 0]
    whole = M.dyn_model(rows, curves, which)
    want = M.dyn_model(rows, curves, which, out_stride=out_stride)
    assert [w[2:] for w in want] == [w[2:] for w in whole] and want[0][2] == 1 and want[4][2] == 1
    dyn_set = sets(curves)
    if out_stride == 0:
        d_in = dev.up(np.concatenate([np.concatenate([x, np.full(256 - len(x), np.nan, np.float32)]) for x in rows]))
        d_len = dev.up(np.array([len(x) for x in rows], np.uint32))
        out_len, bad, mg = gpu_ctx.dyn(dyn_set, d_in, 256, d_len, 5, dev.up(np.array(which, np.uint32)), None, 0)
        for i, w in enumerate(want):
            assert (out_len[i], bad[i]) == (0, w[2]) and np.float64(mg[i]).view(np.uint64) == np.float64(w[3]).view(np.uint64)
        return
    same(want, run(gpu_ctx, dev, dyn_set, rows, which, stride=256, out_stride=out_stride), out_stride)


def test_a_curve_index_outside_the_set_is_refused(gpu_ctx, dev, sets):
    rng = np.random.default_rng(9)
    curves = three_curves()
    rows = [audio(100, rng) for _ in range(5)]
    which = [0, 3, 2, 0xFFFFFFFF, 1]
    want = M.dyn_model(rows, curves, which)
    assert [w[1] == M.REFUSED for w in want] == [False, True, False, True, False]
    same(want, run(gpu_ctx, dev, sets(curves), rows, which), "refused")


def test_alphas_of_zero_and_an_attack_far_below_the_release(gpu_ctx, dev, sets):
    """alpha = 0 both ways: the envelope is the detector's value at once, and a constant input makes a == e at every step
    after the first (the compare a > e is false, the release's alpha taken).  Then a fast attack with a slow release."""
    rng = np.random.default_rng(10)
    comp = G.dyn_design(G.DYN_COMPRESS, G.DYN_PEAK, -30.0, 8.0, 0.0, 0.0, 0.0)
    curves = [(comp, (0.0, 0.0), G.DYN_PEAK), (staircase(), (0.0, 0.0), G.DYN_SQUARE),
              (comp, G.dyn_ballistics(48000, 0.05, 400.0), G.DYN_PEAK), (staircase(), (0.0, 0.999), G.DYN_PEAK)]
    rows = [audio(300, rng), audio(300, rng), audio(300, rng), audio(300, rng), np.full(200, 0.3, np.float32),
            np.full(200, -0.3, np.float32)]
    which = [0, 1, 2, 3, 0, 1]
    want = M.dyn_model(rows, curves, which)
    same(want, run(gpu_ctx, dev, sets(curves), rows, which), "alphas")
    # the staircase at alpha = 0 on a constant: every output is the one gain times the sample
    assert len(set(want[5][0].view(np.uint32).tolist())) == 1


# ---- the lookup's edges ------------------------------------------------------------------------------------------------------
def edge_samples():
    """float32 samples whose |x| (PEAK) or x * x (SQUARE) lands on the lookup's edges when alpha = 0"""
    lev = M.LEVELS.astype(np.float32)                            # (every lev[k] is a float32)
    assert np.array_equal(lev.astype(np.float64), M.LEVELS)
    peak = np.concatenate([lev, np.nextafter(lev, np.float32(0.0)), np.nextafter(lev, np.float32(np.inf))])
    roots = np.array([m * 2.0 ** a for a in range(-17, 5) for m in (1.0, 1.25, 1.5)], np.float32)       # squares that are levels
    square = np.concatenate([roots, np.nextafter(roots, np.float32(0.0)), np.nextafter(roots, np.float32(np.inf))])
    odd = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, 1.1754944e-38, 2.0 ** -33, 2.0 ** -32, 1.5 * 2.0 ** -33, 2.0 ** -40, 2.0 ** -16,
                    2.0 ** -17, 0.9 * 2.0 ** -16, 16.0, 16.5, 17.0, 255.9, 256.0, 257.0, 1e4, 3e38, -3e38, np.nan, np.inf, -np.inf,
                    1e-30, 2.0 ** -64, 2.0 ** -75], np.float32)
    x = np.concatenate([peak, square, odd])
    x[1::2] = -x[1::2]
    return x


def edge_curves():
    """the four settings the edge samples go through: the staircase at alpha = 0 on either detector, an expander whose release
    rides below 2^-32, and the staircase on the square with alphas that are not 0"""
    gate = G.dyn_design(G.DYN_EXPAND, G.DYN_PEAK, -150.0, 2.0, 10.0, 60.0, 0.0)       # its knee lies on the table's lower end
    return [(staircase(), (0.0, 0.0), G.DYN_PEAK), (staircase(), (0.0, 0.0), G.DYN_SQUARE), (gate, (0.0, 0.5), G.DYN_PEAK),
            (staircase(), (0.5, 0.96875), G.DYN_SQUARE)]


def test_samples_on_the_lookups_edges(gpu_ctx, dev, sets):
    """every lev[k], the float32 below and above it, the squares' roots and their neighbours, magnitudes below 2^-32 and above
    2^8 (for the square: below 2^-16 and above 16), +-0.0, denormals, NaN and +-Inf: with alpha = 0 the staircase answers k + f
    for each, so a k off by one or an f off by a bit is in the output's bits; with the expander's curve and a slow release the
    same samples cross the table's lower end on the way down"""
    x = edge_samples()
    rng = np.random.default_rng(12)
    curves = edge_curves()
    rows = [x, x, x, x, rng.permutation(x), rng.permutation(x)]
    which = [0, 1, 2, 3, 0, 1]
    want = M.dyn_model(rows, curves, which)
    same(want, run(gpu_ctx, dev, sets(curves), rows, which), "edges")
    finite = np.abs(x) <= M.FLT_MAX
    assert want[0][2] == 3 and np.all(want[0][0][~finite].view(np.uint32) == 0)     # NaN, Inf -> +0.0, counted
    # the staircase's own answers, where the model is not needed: |x| = lev[k] -> k * x
    k = 37
    at = int(np.flatnonzero(np.abs(x) == np.float32(M.LEVELS[k]))[0])
    assert want[0][0][at] == np.float32(k * float(x[at]))


# ---- keys ---------------------------------------------------------------------------------------------------------------------
def test_keys_shorter_and_longer_than_their_rows(gpu_ctx, dev, sets):
    """a key that ends before its row (the row's end rides the release on +0.0), one that outlasts it, key_len_dev NULL (every
    key is key_stride long: what lies past a key's own samples is read, so the buffer holds zeros there), two rows on one key,
    a row that is its neighbour's key's listener through key_row_dev, a key index outside (refused), non-finite key samples"""
    rng = np.random.default_rng(13)
    curves = three_curves()
    rows = [audio(n, rng) for n in (200, 129, 64, 300, 1, 0, 200)]
    keys = [audio(n, rng) for n in (100, 300, 64, 0)]
    keys[0][[2, 50]], keys[1][7] = (np.nan, -np.inf), np.inf
    which = [0, 1, 2, 0, 1, 2, 0]
    key_row = [0, 1, 2, 1, 3, 0, 4]                              # rows 1 and 3 on key 1; row 6 on a key that is not there
    dyn_set = sets(curves)
    want = M.dyn_model(rows, curves, which, keys=keys, key_row=key_row)
    assert want[6][1] == M.REFUSED and want[0][2] == 0          # (a key's non-finite samples are not counted)
    same(want, run(gpu_ctx, dev, dyn_set, rows, which, keys=keys, key_row=key_row, key_lens=[len(k) for k in keys]), "keyed")
    # key_len_dev holds more than the stride, and less than the key: the key is min(key_len, key_stride) long
    lens = [5000, 10, 0xFFFFFFFF, 0]
    padded = [np.concatenate([k, np.zeros(320 - len(k), np.float32)]) for k in keys]
    want = M.dyn_model(rows, curves, which, keys=padded, key_row=key_row, key_lens=[320, 10, 320, 0])
    same(want, run(gpu_ctx, dev, dyn_set, rows, which, keys=padded, key_row=key_row, key_lens=lens, key_stride=320), "key_len")
    # key_len_dev NULL, key_row_dev NULL: row u listens to the whole of key u
    seven = [audio(320, rng) for _ in range(7)]
    want = M.dyn_model(rows, curves, which, keys=seven)
    same(want, run(gpu_ctx, dev, dyn_set, rows, which, keys=seven), "key NULLs")
    # the scalar path: a key stride of 321 with a base 4 bytes off, rows and out aligned
    odd = [np.concatenate([k, np.zeros(1, np.float32)]) for k in seven]
    same(M.dyn_model(rows, curves, which, keys=odd), run(gpu_ctx, dev, dyn_set, rows, which, keys=odd, key_stride=321, key_offset=1),
         "key scalar")


def test_a_row_may_be_its_own_key(gpu_ctx, dev, sets):
    """key_dev = rows_dev with key u for row u is the self-keyed call, bit for bit"""
    rng = np.random.default_rng(14)
    curves = three_curves()
    rows = [audio(n, rng) for n in (200, 65, 128)]
    rows[0][5] = np.nan
    dyn_set = sets(curves)
    alone = run(gpu_ctx, dev, dyn_set, rows, [0, 1, 2])
    keyed = run(gpu_ctx, dev, dyn_set, rows, [0, 1, 2], keys=rows, key_lens=[len(x) for x in rows])
    want = M.dyn_model(rows, curves, [0, 1, 2])
    same(want, alone, "self-keyed")
    same(want, keyed, "keyed by itself")


def test_keys_of_no_samples(gpu_ctx, dev, sets):
    """key_stride 0 (the header allows it: keys of no samples): no key load is issued (`key_loads` false in the keyed kernel,
    the key's tile never written), every key sample reads +0.0 and the gain is the curve's at e = +0.0 throughout, on either
    path.  No other case runs a keyed call without a key load."""
    rng = np.random.default_rng(16)
    curves = three_curves()
    rows = [audio(n, rng) for n in (200, 65, 0, 64, 129)]
    rows[0][3] = np.nan
    which = [0, 1, 2, 2, 1]
    nothing = [np.zeros(0, np.float32)]
    want = M.dyn_model(rows, curves, which, keys=nothing, key_row=[0] * 5)
    at_rest = [float(np.asarray(curves[c][0], np.float64)[0]) for c in which]          # (e = +0.0 lies below the table: G[0] itself)
    assert [w[3] for w in want] == [g if len(x) else 1.0 for g, x in zip(at_rest, rows)]
    dyn_set = sets(curves)
    for kw, vec in ((dict(stride=256, out_stride=256), True), (dict(stride=256, out_stride=256, in_offset=1), False),
                    (dict(stride=256, out_stride=256, key_offset=1), False)):
        assert variant(kw.get("in_offset", 0), 256, 0, 256, True, kw.get("key_offset", 0), 0) == (vec, True, False)
        same(want, run(gpu_ctx, dev, dyn_set, rows, which, keys=nothing, key_row=[0] * 5, key_stride=0, **kw), ("no key samples", kw))


def test_a_bed_ducks_under_the_voices_that_speak(gpu_ctx, dev, sets):
    """70 bed rows, each keyed by one of 5 voice tracks, of which two are silent and one speaks only below the threshold: a
    bed's min_gain is below 1 exactly where the model's is, which is exactly under the two voices that are loud"""
    rng = np.random.default_rng(15)
    duck = G.dyn_design(G.DYN_COMPRESS, G.DYN_SQUARE, -30.0, 6.0, 6.0, 0.0, 0.0)
    curves = [(duck, G.dyn_ballistics(48000, 2.0, 80.0), G.DYN_SQUARE)]
    n = 400
    beds = [audio(n, rng) for _ in range(70)]
    voices = [np.zeros(n, np.float32), (0.5 * rng.uniform(-1, 1, n)).astype(np.float32), np.zeros(n, np.float32),
              (1e-3 * rng.uniform(-1, 1, n)).astype(np.float32), (0.8 * rng.uniform(-1, 1, n)).astype(np.float32)]
    key_row = [int(v) for v in rng.integers(0, 5, 70)]
    want = M.dyn_model(beds, curves, keys=voices, key_row=key_row)
    got = run(gpu_ctx, dev, sets(curves), beds, None, keys=voices, key_row=key_row, key_lens=[n] * 5)
    same(want, got, "ducking")
    ducked = [w[3] < 1.0 for w in want]
    assert ducked == [bool(m < 1.0) for m in got[3]] == [k in (1, 4) for k in key_row] and any(ducked) and not all(ducked)
    # an unducked bed is its own samples times 1.0
    quiet = key_row.index(0)
    same_bits(got[0][quiet, :n], beds[quiet], "an unducked bed")


def test_dialogue_example_compresses_before_the_limiter(gpu_ctx, tmp_path):
    """grail_dialogue --compress through the C ABI: the WAV is written, both tracks' largest gain reduction is printed (a
    threshold this low reduces every line), and the limiter's line comes after the compressor's"""
    import os
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    wav = tmp_path / "dialogue.wav"
    r = subprocess.run([os.path.join(root, "grail-rs_amd", "lib", "grail_dialogue"), "-o", str(wav), "--lufs", "-23", "--compress", "-40:3:6:5:120",
                        "--makeup", "2", "--ceiling", "-1", "--limit", "a e i o u a e i o u", "o u a e i o u a e i"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"Compressed \(grail_dyn_async\) above -40 dB at 3:1, knee 6 dB, attack 5 ms, release 120 ms, make-up 2 dB: "
                  r"largest gain reduction ([0-9.]+) dB and ([0-9.]+) dB", r.stdout)
    assert m and float(m.group(1)) > 0.5 and float(m.group(2)) > 0.5, r.stdout
    assert r.stdout.index("Compressed") < r.stdout.index("Limiter,") and wav.stat().st_size > 44
