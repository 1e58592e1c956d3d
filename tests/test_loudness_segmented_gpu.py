"""The segmented K-weighting on the device (include/grail_hip.h, "levels, continued": THE SEGMENTED FORM):
grail_loudness_segmented_async compared BIT FOR BIT with the numpy model of its contract
(tests/test_loudness_segmented_host.py: segmented_hops_model) and, where the header says the two are one, with
grail_loudness_async on the same buffer.

Everything bit-exact runs at 2 560, 2 570, 2 580 and 2 590 Hz — hops of 256 .. 259 samples, every H mod 4 — with the
K-weighting of 48 kHz as the caller's own ten coefficients: at such hops the slow pole pair decays only to 0.28 per hop, so
a warm-up that starts one sample or one hop off changes the bits instead of hiding below them.  At 8 kHz with the rate's
own K-weighting the device's two calls are held to the bound the host test asserts of the two models."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import grail_hip as G
from test_levels_gpu import CANARY, Dev, _place, dev  # noqa: F401  (dev is a fixture)
from test_loudness_host import gate_model, kweighting_model, lufs_model, same_bits
from test_loudness_segmented_host import HOP_BOUND, LU_BOUND, P, closeness_signals, segmented_hops_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = [2560, 2570, 2580, 2590]
HOPS = [0, 1, 3, 4, 5, 63, 64, 65, 67, 130]          # P + 1 and P + 2, a wave's edge, a second and a third wave of one row
COEF = kweighting_model(48000)
BAD = 0xABCD1234


def tails(H):
    return [0, 1, H - 1]


def _awkward(rng, n):
    """audio-sized samples with -0.0, denormals, +-1.0, NaN and +-Inf sprinkled in (about one sample in sixty).  Nothing
    huge: a sample of 3e38 would own its hops' sums and hide a warm-up that starts one sample off below their last bit."""
    x = (rng.standard_normal(n) * 0.2).astype(np.float32)
    specials = np.array([-0.0, 0.0, 1e-45, -1e-45, 1e-39, -3e-39, -1.0, np.nan, np.inf, -np.inf, 1.0], np.float32)
    mask = rng.random(n) < 1.0 / 60.0
    x[mask] = specials[rng.integers(0, len(specials), int(mask.sum()))]
    return x


def model_of(rows, rate):
    """[(hops, gated mean square, nonfinite)] per row"""
    H = rate // 10
    return [(h, gate_model(h, H), b) for h, b in segmented_hops_model(rows, rate, COEF)]


_cache = {}


def rows_at(rate):
    """the rows of HOPS whole hops with tails of 0, 1 and H - 1 samples (awkward values: -0.0, denormals, +-1.0, NaN, +-Inf
    about one sample in sixty) and what the model says of them — computed once per rate and never changed"""
    if rate not in _cache:
        H = rate // 10
        rng = np.random.default_rng(rate)
        rows = [_awkward(rng, k * H + tails(H)[i % 3]) for i, k in enumerate(HOPS)]
        rows[1][0] = np.float32(np.nan)
        for x in rows:
            x.setflags(write=False)
        _cache[rate] = dict(rate=rate, H=H, rows=rows, model=model_of(rows, rate))
    return _cache[rate]


def measure(ctx, dev, rows_dev, stride, d_len, n, rate, coef=COEF, hs=None, call=None):
    """grail_loudness_segmented_async into arrays with a canary before and after each -> (gated [n], hops [n, hs],
    nonfinite [n]); hops past a row's last hold CANARY"""
    hs = stride // (rate // 10) + 2 if hs is None else hs
    g0, h0, b0 = np.full(n + 2, CANARY), np.full(n * hs + 2, CANARY), np.full(n + 2, BAD, np.uint32)
    d_g, d_h, d_b = dev.up(g0), dev.up(h0), dev.up(b0)
    (call or ctx.loudness_segmented_async)(rows_dev, stride, d_len, n, rate, coef, C.c_void_p(d_g.value + 8),
                                           C.c_void_p(d_h.value + 8), hs, C.c_void_p(d_b.value + 4))
    ctx.sync()
    g, h, b = dev.down(d_g, n + 2, np.float64), dev.down(d_h, n * hs + 2, np.float64), dev.down(d_b, n + 2, np.uint32)
    assert g[0] == CANARY and g[-1] == CANARY and h[0] == CANARY and h[-1] == CANARY, "a canary around an output was written"
    assert b[0] == BAD and b[-1] == BAD
    return g[1:-1], h[1:-1].reshape(n, hs), b[1:-1]


def check_rows(got, model, positions, what):
    g, h, b = got
    for i, pos in enumerate(positions):
        wh, wg, wb = model[i]
        k = len(wh)
        assert same_bits(h[pos, :k], wh), (what, i, "hops", int(np.argmax(h[pos, :k].view(np.uint64) != wh.view(np.uint64))))
        assert np.all(h[pos, k:] == CANARY), (what, i, "a hop past the row's last was written")
        assert same_bits(g[pos], wg), (what, i, g[pos], wg)
        assert b[pos] == wb, (what, i, b[pos], wb)


# ---- the rows against the model, every output alone, and against the serial call --------------------------------------------
@pytest.mark.parametrize("rate", RATES)
def test_rows_equal_the_segmented_model(gpu_ctx, dev, rate):
    """0, 1, 3, 4, 5, 63, 64, 65, 67 and 130 whole hops with tails of 0, 1 and H - 1 samples in one call: hop sums, gated
    mean squares and non-finite counts bit for bit; no hop past a row's last written up to hops_stride, no canary
    touched; then the hops through the context's scratch, and each output alone"""
    S = rows_at(rate)
    rows, model, H = S["rows"], S["model"], S["H"]
    n = len(rows)
    stride = (max(len(x) for x in rows) + 63) // 64 * 64
    rows_dev, d_len, _ = _place(gpu_ctx, dev, rows, list(range(n)), n, stride)
    got = measure(gpu_ctx, dev, rows_dev, stride, d_len, n, rate)
    check_rows(got, model, list(range(n)), f"rate {rate}")
    assert [len(m[0]) for m in model] == HOPS and sum(m[2] for m in model) > 100 and model[3][1] > 0
    want_g, want_b = np.array([m[1] for m in model]), np.array([m[2] for m in model], np.uint32)
    # hop_sumsq_dev NULL: the hops go through scratch
    g, _, b = gpu_ctx.loudness_segmented(rows_dev, stride, d_len, n, rate, COEF, hops=False)
    assert same_bits(g, want_g) and np.array_equal(b, want_b)
    # each output alone
    d_g, d_b = dev.up(np.full(n, CANARY)), dev.up(np.full(n, 7, np.uint32))
    hs = stride // H
    d_h = dev.up(np.full(n * hs, CANARY))
    gpu_ctx.loudness_segmented_async(rows_dev, stride, d_len, n, rate, COEF, gated_ms_dev=d_g)
    gpu_ctx.loudness_segmented_async(rows_dev, stride, d_len, n, rate, COEF, nonfinite_dev=d_b)
    gpu_ctx.loudness_segmented_async(rows_dev, stride, d_len, n, rate, COEF, hop_sumsq_dev=d_h, hops_stride=hs)
    gpu_ctx.sync()
    assert same_bits(dev.down(d_g, n, np.float64), want_g) and np.array_equal(dev.down(d_b, n, np.uint32), want_b)
    h = dev.down(d_h, (n, hs), np.float64)
    for i, m in enumerate(model):
        assert same_bits(h[i, :len(m[0])], m[0]) and np.all(h[i, len(m[0]):] == CANARY)
    # none at all: nothing to do, nothing written
    gpu_ctx.loudness_segmented_async(rows_dev, stride, d_len, n, rate, COEF)
    gpu_ctx.sync()


def test_a_hop_of_a_multiple_of_four_but_not_of_eight_samples(gpu_ctx, dev):
    """2 600 Hz: H = 260 keeps the 16-byte loads (H % 4 == 0) and puts the end of the warm-up, 3 H = 780 samples on, 12 into a
    tile: a run of 12 is one unrolled eight and four samples one by one.  Of RATES only 2 560 has 16-byte loads, and its
    warm-up and hop end with a tile"""
    rate = 2600
    H = rate // 10
    assert H % 4 == 0 and (3 * H) % 64 % 8 != 0 and [r // 10 % 4 for r in RATES] == [0, 1, 2, 3] and (3 * 256) % 64 == 0
    S = rows_at(rate)
    rows, model = S["rows"], S["model"]
    n = len(rows)
    stride = (max(len(x) for x in rows) + 63) // 64 * 64
    rows_dev, d_len, _ = _place(gpu_ctx, dev, rows, list(range(n)), n, stride)
    check_rows(measure(gpu_ctx, dev, rows_dev, stride, d_len, n, rate), model, list(range(n)), f"rate {rate}")
    assert [len(m[0]) for m in model] == HOPS and sum(m[2] for m in model) > 100 and model[3][1] > 0


@pytest.mark.parametrize("rate", RATES)
def test_the_first_hops_and_short_rows_are_the_serial_calls(gpu_ctx, dev, rate):
    """hops 0 .. P of every row, and every number of the rows of at most P + 1 hops, equal grail_loudness_async on the
    same buffer bit for bit; the counts are the serial call's for every row; a later hop is not the serial call's"""
    S = rows_at(rate)
    rows = S["rows"]
    n = len(rows)
    stride = (max(len(x) for x in rows) + 63) // 64 * 64
    rows_dev, d_len, _ = _place(gpu_ctx, dev, rows, list(range(n)), n, stride)
    g1, h1, b1 = measure(gpu_ctx, dev, rows_dev, stride, d_len, n, rate)
    g0, h0, b0 = measure(gpu_ctx, dev, rows_dev, stride, d_len, n, rate, call=gpu_ctx.loudness_async)
    assert np.array_equal(b0, b1)
    for i, k in enumerate(HOPS):
        first = min(k, P + 1)
        assert same_bits(h1[i, :first], h0[i, :first]), i
        if k <= P + 1:
            assert same_bits(h1[i], h0[i]) and same_bits(g1[i], g0[i]), i
    assert not same_bits(h1[9, :130], h0[9, :130])


@pytest.mark.parametrize("rate", RATES)
def test_a_non_finite_sample_is_counted_once(gpu_ctx, dev, rate):
    """NaN and +-Inf at sample 0, inside a hop, in a hop that three later hops warm up over (and a fourth does not), and in
    the tail after the last whole hop: four in the row's count, and the hops are the model's.  The same row without its
    tail, and one that is a tail only."""
    H = rate // 10
    rng = np.random.default_rng(rate + 1)
    x = (rng.standard_normal(10 * H + 40) * 0.2).astype(np.float32)
    x[0], x[2 * H + 17], x[5 * H + H // 2], x[10 * H + 39] = np.nan, np.inf, -np.inf, np.nan
    rows = [x, x[:10 * H], x[10 * H:], x[:5 * H + H // 2 + 1]]
    stride = (len(x) + 3) // 4 * 4
    rows_dev, d_len, _ = _place(gpu_ctx, dev, rows, [0, 1, 2, 3], 4, stride)
    model = model_of(rows, rate)
    assert [m[2] for m in model] == [4, 3, 1, 3]
    check_rows(measure(gpu_ctx, dev, rows_dev, stride, d_len, 4, rate), model, [0, 1, 2, 3], "non-finite")


# ---- neighbours and layout -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", RATES)
def test_a_rows_numbers_do_not_depend_on_the_rows_around_it(gpu_ctx, dev, rate):
    """a row measured alone, and the rows at other indices among 63, 64, 65 and 300 rows (the others hold 0x3c3c3c3c over
    random lengths): the same bits"""
    S = rows_at(rate)
    rows, model = S["rows"], S["model"]
    for i in (9, 8, 4, 1):
        stride = (len(rows[i]) + 63) // 64 * 64
        rows_dev, d_len, _ = _place(gpu_ctx, dev, [rows[i]], [0], 1, stride)
        check_rows(measure(gpu_ctx, dev, rows_dev, stride, d_len, 1, rate), [model[i]], [0], f"alone {i}")
    stride = (max(len(x) for x in rows) + 63) // 64 * 64
    for n_total in (11, 63, 64, 65, 300):
        rng = np.random.default_rng(n_total)
        pos = sorted(rng.choice(n_total, len(rows), replace=False).tolist())
        pos = [pos[i] for i in rng.permutation(len(rows))]
        rows_dev, d_len, lens = _place(gpu_ctx, dev, rows, pos, n_total, stride, 0, rng)
        g, h, b = got = measure(gpu_ctx, dev, rows_dev, stride, d_len, n_total, rate)
        check_rows(got, model, pos, f"among {n_total}")
        rest = np.setdiff1d(np.arange(n_total), pos)
        assert not b[rest].any() and np.all(np.isfinite(g[rest]))
        dev.free()


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("layout", ["stride4", "odd", "stride2", "offset1", "offset3", "reversed"])
def test_a_rows_numbers_do_not_depend_on_its_layout(gpu_ctx, dev, rate, layout):
    """row_stride a multiple of 4 but not of 64, odd, even but no multiple of 4; rows_dev 4 and 12 bytes past an
    allocation's alignment; the rows in another order"""
    S = rows_at(rate)
    rows, model = S["rows"], S["model"]
    longest = max(len(x) for x in rows)
    stride = {"stride4": (longest + 3) // 4 * 4, "odd": (longest + 3) // 4 * 4 + 1, "stride2": (longest + 3) // 4 * 4 + 2}.get(
        layout, (longest + 63) // 64 * 64)
    offset = int(layout[-1]) if layout.startswith("offset") else 0
    pos = list(range(len(rows)))[::-1] if layout == "reversed" else list(range(len(rows)))
    rows_dev, d_len, _ = _place(gpu_ctx, dev, rows, pos, len(rows), stride, offset)
    check_rows(measure(gpu_ctx, dev, rows_dev, stride, d_len, len(rows), rate), model, pos, layout)


@pytest.mark.parametrize("rate", RATES)
def test_a_len_above_row_stride_reads_as_row_stride(gpu_ctx, dev, rate):
    H = rate // 10
    base = (6 * H + 40) // 4 * 4
    for stride in (base, base - 1):
        rng = np.random.default_rng(stride)
        rows = [_awkward(rng, stride) for _ in range(3)]
        rows_dev, _, _ = _place(gpu_ctx, dev, rows, [0, 1, 2], 3, stride)
        d_len = dev.up(np.array([stride + 1, 0xFFFFFFFF, stride], np.uint32))
        check_rows(measure(gpu_ctx, dev, rows_dev, stride, d_len, 3, rate), model_of(rows, rate), [0, 1, 2], f"stride {stride}")


def test_more_rows_than_a_grids_second_dimension_holds(gpu_ctx, dev):
    """70 000 rows of one hop and a tail (the hardware ends grid.y at 65 535): sampled rows, the last among them, equal
    the model; every row's count is its NaNs"""
    rate, H, n = 2570, 257, 70000
    stride = 300
    rng = np.random.default_rng(7)
    x = (rng.standard_normal((n, stride)) * 0.2).astype(np.float32)
    lens = rng.integers(0, stride + 1, n).astype(np.uint32)
    lens[-1], lens[65535], lens[65536] = stride, 299, 257
    x[np.arange(n) % 7 == 0, 5] = np.nan
    rows_dev, d_len = dev.up(x), dev.up(lens)
    g, h, b = gpu_ctx.loudness_segmented(rows_dev, stride, d_len, n, rate, COEF, fill=CANARY)
    assert np.array_equal(b, ((np.arange(n) % 7 == 0) & (lens > 5)).astype(np.uint32)) and np.all(g == 0.0)
    assert np.all(h[lens < H, 0] == CANARY) and np.all(h[lens >= H, 0] != CANARY)
    sample = [0, 1, 255, 65534, 65535, 65536, 65537, n - 2, n - 1]
    for u, (wh, _, _) in zip(sample, model_of([x[u, :lens[u]] for u in sample], rate)):
        assert same_bits(h[u, :len(wh)], wh), u


# ---- invalid arguments -----------------------------------------------------------------------------------------------------
def test_invalid_arguments(gpu_ctx, dev):
    d_rows, d_len = dev.up(np.zeros(48000, np.float32)), dev.up(np.array([48000], np.uint32))
    d_h = dev.up(np.full(16, CANARY))
    for rate, hs in ((48000, 9), (48000, 0), (2559, 16), (1048577, 16), (0, 16)):
        with pytest.raises(G.GrailError) as ei:
            gpu_ctx.loudness_segmented_async(d_rows, 48000, d_len, 1, rate, None, None, d_h, hs, None)
        assert ei.value.status == G.ERR_INVALID_ARG and "grail_loudness_segmented_async" in str(ei.value), (rate, hs)
    for rows_dev, len_dev in ((None, d_len), (d_rows, None)):
        with pytest.raises(G.GrailError) as ei:
            gpu_ctx.loudness_segmented_async(rows_dev, 48000, len_dev, 1, 48000, None, None, d_h, 16, None)
        assert ei.value.status == G.ERR_INVALID_ARG and "NULL buffer" in str(ei.value)
    # the one refusal of its own: more than 2^26 - 1 waves of 64 hops in all (refused before anything is read or launched)
    for n_rows, stride in ((1 << 26, 4800), (1 << 20, 64 * 64 * 4800)):
        with pytest.raises(G.GrailError) as ei:
            gpu_ctx.loudness_segmented_async(d_rows, stride, d_len, n_rows, 48000, None, None, None, 0, d_h)
        assert ei.value.status == G.ERR_INVALID_ARG and "waves" in str(ei.value)
    gpu_ctx.sync()
    assert np.all(dev.down(d_h, 16, np.float64) == CANARY)
    gpu_ctx.loudness_segmented_async(d_rows, 48000, d_len, 1, 48000, None, None, d_h, 10, None)      # exactly row_stride / H
    gpu_ctx.loudness_segmented_async(None, 0, None, 0, 48000, None, None, d_h, 0, None)                # no rows: nothing to do
    gpu_ctx.sync()
    h = dev.down(d_h, 16, np.float64)
    assert np.all(h[:10] == 0.0) and np.all(h[10:] == CANARY)


# ---- the K-weighting of the rate itself: close to the serial call -------------------------------------------------------------
def test_at_8_khz_the_two_calls_agree_to_the_asserted_bound(gpu_ctx, dev):
    """rows of 30 hops and a tail at 8 000 Hz, coef NULL: the device's segmented hops and LUFS within the bounds the host
    test asserts of the two models (100 times what it measured), and bit-equal to the model over grail_kweighting's ten"""
    rate, H = 8000, 800
    rows = list(closeness_signals(rate).values())
    n = len(rows)
    stride = (max(len(x) for x in rows) + 63) // 64 * 64
    rows_dev, d_len, _ = _place(gpu_ctx, dev, rows, list(range(n)), n, stride)
    g1, h1, b1 = measure(gpu_ctx, dev, rows_dev, stride, d_len, n, rate, coef=None)
    g0, h0, b0 = measure(gpu_ctx, dev, rows_dev, stride, d_len, n, rate, coef=None, call=gpu_ctx.loudness_async)
    coef = G.kweighting(rate)
    for i, (wh, _) in enumerate(segmented_hops_model(rows, rate, coef)):
        assert same_bits(h1[i, :30], wh) and same_bits(g1[i], gate_model(wh, H)), i
    d_hop = float(np.max(np.abs(h1[:, :30] - h0[:, :30])) / H)
    d_lu = max(abs(lufs_model(a) - lufs_model(b)) for a, b in zip(g1, g0))
    print(f"\nsegmented against serial on the device: |d hop| / H {d_hop:.2e}, |d LUFS| {d_lu:.2e}")
    assert not b1.any() and not b0.any() and np.all(g0 > 0)
    assert d_hop <= HOP_BOUND and d_lu <= LU_BOUND


# ---- the example ---------------------------------------------------------------------------------------------------------
def test_grail_dialogue_report_option(gpu_ctx, tmp_path):
    """--report: exit status 0 and one line of five fields per track, numbers where the track is long enough"""
    exe = os.path.join(ROOT, "grail-rs_amd", "lib", "grail_dialogue")
    path = str(tmp_path / "report.wav")
    r = subprocess.run([exe, "-o", path, "--lufs", "-23", "--report", "hello there, how are you on this fine day",
                        "a fine day to you, and to all of yours, wherever they may be"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = re.findall(r"^Track (\d): integrated (\S+)(?: LUFS)?, range (\S+)(?: LU)?, max momentary (\S+)(?: LUFS)?, "
                       r"max short-term (\S+)(?: LUFS)?, true peak (\S+)(?: dBTP)?$", r.stdout, flags=re.M)
    assert [m[0] for m in lines] == ["1", "2"], r.stdout
    for m in lines:
        integrated, momentary, peak = float(m[1]), float(m[3]), float(m[5])
        assert -40.0 < integrated < -15.0 and momentary >= integrated - 1.0 and -40.0 < peak < 6.0, r.stdout
        for field in (m[2], m[4]):                      # a track shorter than 3 s has no short-term loudness and no range
            assert field == "-" or np.isfinite(float(field))
