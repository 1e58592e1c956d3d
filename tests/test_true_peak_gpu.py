"""True peak on the device (grail_true_peak_async, grail_batch_mix_leveled_limited) against the numpy model of
tests/test_true_peak_host.py: bit for bit over awkward rows, at the seams of the kernel's steps and chunks and in the
tail after a row's last sample, whatever lies around or behind a row; rendered rows; the limited mix against the host
model of its gains and against grail_batch_mix; the full-size batch; the example."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import grail_hip as G
from grail_hip import workload as W
from test_levels_gpu import CANARY, Dev, _place, dev, same_bits  # noqa: F401  (dev is a fixture)
from test_true_peak_host import FLT_MAX, ROUNDING, TAP_SUM, ceiling_of, limit_model, true_peak_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = [0, 1, 2, 11, 12, 13, 255, 256, 257, 4095, 4096, 4097, 4107, 96006, 100003]
UNIT = 7964.0 / 8192.0                  # what a lone 1.0 reads: the centre tap of phases 0 and 3


def _awkward(rng, n):
    """noise over sixty decades of scale with -0.0, denormals, +-FLT_MAX, NaN and +-Inf sprinkled in (about one sample in
    forty); stretches of the row are scaled apart so that small and large samples meet inside one filter window"""
    x = rng.standard_normal(n) * 10.0 ** rng.uniform(-30.0, 30.0, n // 500 + 1).repeat(500)[:n]
    with np.errstate(over="ignore"):
        x = np.clip(x, -float(FLT_MAX), float(FLT_MAX)).astype(np.float32)
    specials = np.array([-0.0, 0.0, 1e-45, -1e-45, 1e-39, -3e-39, FLT_MAX, -FLT_MAX, np.nan, np.inf, -np.inf, 1.0], np.float32)
    mask = rng.random(n) < 1.0 / 40.0
    x[mask] = specials[rng.integers(0, len(specials), int(mask.sum()))]
    return x


@pytest.fixture(scope="module")
def synthetic():
    rng = np.random.default_rng(91)
    rows = [_awkward(rng, n) for n in LENGTHS]
    rows[1][0] = np.float32(-0.5)                       # the one-sample row holds a sample that counts
    rows[2][:] = [FLT_MAX, FLT_MAX]
    rows[13][-1] = np.float32(np.nan)
    rows[14][-1] = np.float32(-3.0)
    model = [true_peak_model(x) for x in rows]
    assert sum(m[1] for m in model) > 100 and model[0] == (0.0, 0) and model[1] == (0.5 * UNIT, 0)
    return dict(rows=rows, model=model)


def _check(ctx, synthetic, rows_dev, stride, d_len, n_total, positions, what, which=None):
    tp, bad = ctx.true_peak(rows_dev, stride, d_len, n_total)
    for i, pos in enumerate(positions):
        k = i if which is None else which[i]
        want_tp, want_bad = synthetic["model"][k]
        assert same_bits(tp[pos:pos + 1], np.array([want_tp])), (what, LENGTHS[k], tp[pos], want_tp)
        assert bad[pos] == want_bad, (what, LENGTHS[k], bad[pos], want_bad)
    return tp, bad


def _upload_filled(ctx, dev, rows, stride, fill, offset=0):
    """rows[i] as row i of a buffer whose every other float, the memory past each row's len included, holds `fill`"""
    host = np.full(len(rows) * stride + offset, fill, np.float32)
    for i, x in enumerate(rows):
        host[offset + i * stride:offset + i * stride + len(x)] = x
    base = dev.up(host)
    return C.c_void_p(base.value + offset * 4), dev.up(np.array([len(x) for x in rows], np.uint32))


# ---- synthetic rows ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", ["canary", "nan"])
def test_synthetic_rows_equal_the_model(gpu_ctx, dev, synthetic, fill):
    """lengths 0 ... 100 003 of noise over many scales, -0.0, denormals, +-FLT_MAX, NaN and +-Inf (counted), the memory
    between len and row_stride holding the canary or NaN: true peak and count bit for bit; either output may be NULL"""
    rows = synthetic["rows"]
    stride = (max(LENGTHS) + 63) // 64 * 64
    rows_dev, d_len = _upload_filled(gpu_ctx, dev, rows, stride, CANARY if fill == "canary" else np.nan)
    pos = list(range(len(rows)))
    tp, bad = _check(gpu_ctx, synthetic, rows_dev, stride, d_len, len(rows), pos, fill)
    assert tp[0] == 0 and not np.signbit(tp[0]) and bad[0] == 0
    d_t = dev.up(np.full(len(rows), CANARY))
    gpu_ctx.true_peak_async(rows_dev, stride, d_len, len(rows), true_peak_dev=d_t)
    gpu_ctx.sync()
    assert same_bits(dev.down(d_t, len(rows), np.float64), np.array([m[0] for m in synthetic["model"]]))
    d_b = dev.up(np.full(len(rows), 0xEEEEEEEE, np.uint32))
    gpu_ctx.true_peak_async(rows_dev, stride, d_len, len(rows), nonfinite_dev=d_b)
    gpu_ctx.sync()
    assert np.array_equal(dev.down(d_b, len(rows), np.uint32), np.array([m[1] for m in synthetic["model"]], np.uint32))
    gpu_ctx.true_peak_async(rows_dev, stride, d_len, len(rows))          # nothing asked for: nothing done
    gpu_ctx.true_peak_async(None, 0, d_len, len(rows), true_peak_dev=d_t)  # rows of no samples
    gpu_ctx.sync()
    assert same_bits(dev.down(d_t, len(rows), np.float64), np.zeros(len(rows)))
    with pytest.raises(G.GrailError) as ei:
        gpu_ctx.true_peak_async(None, stride, d_len, len(rows), true_peak_dev=d_t)
    assert ei.value.status == G.ERR_INVALID_ARG


def test_a_lone_one_reads_the_centre_tap_at_every_seam_and_in_the_tail(gpu_ctx, dev):
    """a single 1.0 at every position within +-12 of EVERY multiple of 256 in a row of 12 388 samples (49 of them, the
    multiples of 4 096 among them: the kernel's steps and chunks, whatever their unroll) and at the row's last samples,
    where only the eleven outputs after the row hold the centre tap: 7964 / 8192 exactly, as the model says"""
    n = 3 * 4096 + 100
    at = sorted({p for m in range(0, n + 1, 256) for p in range(m - 12, m + 13) if 0 <= p < n} |
                {n - 1, n - 2, n - 11, n - 12, n - 13})
    assert len(at) > 1200
    rows = []
    for p in at:
        x = np.zeros(n, np.float32)
        x[p] = 1.0
        rows.append(x)
    assert true_peak_model(rows[0]) == (UNIT, 0) and true_peak_model(rows[-1]) == (UNIT, 0)
    for stride, offset in ((n + 3) // 4 * 4, 0), (n + 1, 1):              # 16-byte loads, 4-byte loads
        rows_dev, d_len = _upload_filled(gpu_ctx, dev, rows, stride, np.nan, offset)
        tp, bad = gpu_ctx.true_peak(rows_dev, stride, d_len, len(rows))
        assert not bad.any()
        assert np.all(tp == UNIT), [(at[i], tp[i]) for i in np.flatnonzero(tp != UNIT)]
    # the last sample of rows of every awkward length
    tails = []
    for k in LENGTHS[1:]:
        x = np.zeros(k, np.float32)
        x[-1] = 1.0
        tails.append(x)
    stride = (max(LENGTHS) + 63) // 64 * 64
    rows_dev, d_len = _upload_filled(gpu_ctx, dev, tails, stride, CANARY)
    tp, bad = gpu_ctx.true_peak(rows_dev, stride, d_len, len(tails))
    assert np.all(tp == UNIT) and not bad.any(), tp


@pytest.mark.parametrize("n_total", [1, 63, 64, 65, 300])
def test_a_rows_number_does_not_depend_on_the_rows_around_it(gpu_ctx, dev, synthetic, n_total):
    rng = np.random.default_rng(n_total)
    which = [14] if n_total == 1 else list(range(len(LENGTHS)))
    rows = [synthetic["rows"][k] for k in which]
    pos = sorted(rng.choice(n_total, len(rows), replace=False).tolist())
    pos = [pos[i] for i in rng.permutation(len(rows))]
    stride = (max(LENGTHS) + 63) // 64 * 64
    rows_dev, d_len, lens = _place(gpu_ctx, dev, rows, pos, n_total, stride, 0, rng)
    tp, bad = _check(gpu_ctx, synthetic, rows_dev, stride, d_len, n_total, pos, f"among {n_total}", which)
    # the other rows: constant 0x3c3c3c3c samples
    c = np.frombuffer(b"\x3c" * 4, np.float32)[0]
    rest = np.setdiff1d(np.arange(n_total), pos)
    assert not bad[rest].any()
    for k in rest[:8]:
        assert same_bits(tp[k:k + 1], np.array([true_peak_model(np.full(lens[k], c, np.float32))[0]])), (k, lens[k])


@pytest.mark.parametrize("layout", ["stride4", "odd", "offset1", "offset3", "reversed"])
def test_a_rows_number_does_not_depend_on_its_layout(gpu_ctx, dev, synthetic, layout):
    """row_stride a multiple of 4 and odd; rows_dev 1 and 3 floats past an aligned address (4-byte loads instead of 16-byte
    ones); the rows in another order"""
    rows = synthetic["rows"]
    longest = max(LENGTHS)
    stride = {"stride4": (longest + 3) // 4 * 4, "odd": (longest + 3) // 4 * 4 + 1}.get(layout, (longest + 63) // 64 * 64)
    offset = int(layout[-1]) if layout.startswith("offset") else 0
    pos = list(range(len(rows)))[::-1] if layout == "reversed" else list(range(len(rows)))
    rows_dev, d_len, _ = _place(gpu_ctx, dev, rows, pos, len(rows), stride, offset)
    _check(gpu_ctx, synthetic, rows_dev, stride, d_len, len(rows), pos, layout)


@pytest.mark.parametrize("stride", [96008, 96007, 4096, 4085])
def test_a_len_above_row_stride_reads_as_row_stride(gpu_ctx, dev, stride):
    rng = np.random.default_rng(stride)
    rows = [_awkward(rng, stride) for _ in range(3)]
    rows_dev, _, _ = _place(gpu_ctx, dev, rows, [0, 1, 2], 3, stride)
    d_len = dev.up(np.array([stride + 1, 0xFFFFFFFF, stride], np.uint32))
    tp, bad = gpu_ctx.true_peak(rows_dev, stride, d_len, 3)
    for i, x in enumerate(rows):
        want = true_peak_model(x)
        assert same_bits(tp[i:i + 1], np.array([want[0]])) and bad[i] == want[1], (stride, i)


# ---- rendered rows ---------------------------------------------------------------------------------------------------------
def test_rendered_rows_equal_the_model_over_their_downloaded_samples(gpu_ctx, dev):
    """64 rows of the eight preset voices, measured right behind their rendering (no sync in between)"""
    n = 64
    voices = W.preset_voices(8)
    segs, offs, vids, seeds = W.make_batch(n, n_voices=8)
    stride = W.max_samples()
    gpu_ctx.set_voices(voices)
    b = gpu_ctx.upload(segs, offs, vids, seeds)
    try:
        d_rows, d_len = dev.alloc(n * stride * 4), dev.alloc(n * 4)
        gpu_ctx.memset(d_rows, 0xFF, n * stride * 4)                      # NaNs until the rendering has run
        b.synthesize_async(d_rows, stride, d_len)
        tp, bad = gpu_ctx.true_peak(d_rows, stride, d_len, n)
        _, peak, _ = gpu_ctx.levels(d_rows, stride, d_len, n)
    finally:
        b.free()
    lens = dev.down(d_len, n, np.uint32)
    rows = dev.down(d_rows, (n, stride), np.float32)
    assert not bad.any() and np.count_nonzero(tp) > n // 2
    for u in range(n):
        assert same_bits(tp[u:u + 1], np.array([true_peak_model(rows[u, :lens[u]])[0]])), u
    on = tp > 0
    over = 20.0 * np.log10(tp[on] / peak[on].astype(np.float64))
    print(f"\nrendered rows: true peak {over.min():+.3f} .. {over.max():+.3f} dB against their sample peak")
    assert over.min() >= -0.26 and np.all(tp <= TAP_SUM * peak.astype(np.float64) * ROUNDING)


# ---- the limited mix -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def speech8k_batch():
    """1 100 speech-like rows of two voices at 8 kHz (0.5 - 3.8 s), one of them emptied"""
    rate = 8000
    voices = W.preset_voices(2, sample_rate=rate)
    n = 1100
    segs, offs, vids, seeds, stride = W.speech_like_batch(n, np.random.default_rng(61), n_voices=2, sample_rate=rate)
    cut = int(offs[7])
    segs = np.concatenate([segs[:cut], segs[int(offs[8]):]])             # utterance 7 loses its segments
    offs = offs.copy()
    offs[8:] -= offs[8] - cut
    return dict(rate=rate, voices=voices, n=n, batch=(segs, offs, vids, seeds), stride=stride)


def _level_gains_of(ctx, mode, rate, d_rows, stride, d_len, lens, item_rows, level_db):
    """the leveled mix's gains from the device's own measurements of the rows (entry points that tests/test_levels_gpu.py
    and tests/test_loudness_gpu.py hold to their models), by the library's host function"""
    n = len(lens)
    if mode == G.LEVEL_LOUDNESS:
        gated, _, bad = ctx.loudness(d_rows, stride, d_len, n, rate, hops=False)
        return G.level_gains(mode, item_rows, level_db, nonfinite=bad, row_len=lens,
                             active_level=np.array([G.loudness_level(g) for g in gated]))
    sumsq, peak, bad = ctx.levels(d_rows, stride, d_len, n)
    return G.level_gains(mode, item_rows, level_db, sumsq=sumsq, peak=peak, nonfinite=bad, row_len=lens)


@pytest.mark.parametrize("mode", ["rms", "lufs"])
def test_limited_mix(gpu_ctx, dev, speech8k_batch, mode):
    """grail_batch_mix_leveled_limited on 1 100 rendered rows, babble-like items, the ceiling at the median of what the
    leveled items would reach (so about half of them are limited):
    - the gains equal the host model: grail_level_gains over the rows' measured levels, then the numpy model of
      grail_true_peak_limit_gains over the rows' measured true peaks (which equal the model over the downloaded rows);
    - |gain| x true peak <= c for every item, exactly;
    - the tracks are the bits of grail_batch_mix with those gains; planned as ONE compute unit (blocks of 512 rows: three
      of them) the same tracks, gains and counts;
    - with a ceiling of +200 dB nothing is limited and the tracks are the bits of grail_batch_mix_leveled"""
    S = speech8k_batch
    gmode = {"rms": G.LEVEL_RMS, "lufs": G.LEVEL_LOUDNESS}[mode]
    n, stride, rate = S["n"], S["stride"], S["rate"]
    gpu_ctx.set_voices(S["voices"])
    b = gpu_ctx.upload(*S["batch"])
    try:
        lens = b.lengths()
        assert lens[7] == 0 and lens.max() <= stride
        d_rows, d_len = dev.alloc(n * stride * 4), dev.alloc(n * 4)
        b.synthesize_async(d_rows, stride, d_len)
        tp, tp_bad = gpu_ctx.true_peak(d_rows, stride, d_len, n)
        host_rows = dev.down(d_rows, (n, stride), np.float32)
        for u in list(range(0, n, 37)) + [7]:
            assert same_bits(tp[u:u + 1], np.array([true_peak_model(host_rows[u, :lens[u]])[0]])), u
        assert not tp_bad.any() and tp[7] == 0
        rng = np.random.default_rng(62)
        item_rows = np.concatenate([np.arange(n), rng.integers(0, n, 300), [7]]).astype(np.uint32)
        item_rows = item_rows[rng.permutation(len(item_rows))]
        n_tracks = n // 16
        item_tracks = (item_rows // 16 % n_tracks).astype(np.uint32)
        item_offs = rng.integers(0, 4000, len(item_rows)).astype(np.uint64)
        level_db = rng.uniform(-36.0, -14.0, len(item_rows)).astype(np.float32)
        track_len = 4000 + int(lens.max())
        track_stride = (track_len + 63) // 64 * 64
        leveled, want_unleveled = _level_gains_of(gpu_ctx, gmode, rate, d_rows, stride, d_len, lens, item_rows, level_db)
        reach = leveled.astype(np.float64) * tp[item_rows]
        ceiling_db = float(np.float32(20.0 * np.log10(np.median(reach[reach > 0]))))
        c = ceiling_of(ceiling_db)
        want, want_limited = limit_model(tp, item_rows, leveled, ceiling_db)
        assert len(item_rows) // 3 < want_limited < 2 * len(item_rows) // 3 and want_unleveled >= 2
        d_a, d_b, d_c, d_d = (dev.alloc(n_tracks * track_stride * 4) for _ in range(4))
        out_len, gains, unleveled, limited = b.mix_leveled_limited(item_rows, item_offs, level_db, d_a, track_stride, n_tracks,
                                                           track_len, item_tracks=item_tracks, mode=gmode,
                                                           ceiling_db=ceiling_db)
        assert np.array_equal(out_len, lens) and unleveled == want_unleveled and limited == want_limited
        assert same_bits(gains, want), np.flatnonzero(gains.view(np.uint32) != want.view(np.uint32))[:10]
        assert np.all(np.abs(gains).astype(np.float64) * tp[item_rows] <= c)
        A = dev.down(d_a, (n_tracks, track_stride), np.float32)[:, :track_len]
        b.mix(item_rows, item_offs, d_b, track_stride, n_tracks, track_len, item_tracks=item_tracks, item_gains=gains)
        assert same_bits(A, dev.down(d_b, (n_tracks, track_stride), np.float32)[:, :track_len])
        assert np.isfinite(A).all() and np.abs(A).max() > 0
        saved = gpu_ctx.get_option("assume_compute_units")
        try:
            gpu_ctx.set_option("assume_compute_units", 1)
            assert n > 2 * 2 * 256
            out_len2, gains2, unleveled2, limited2 = b.mix_leveled_limited(item_rows, item_offs, level_db, d_c, track_stride,
                                                                   n_tracks, track_len, item_tracks=item_tracks, mode=gmode,
                                                                   ceiling_db=ceiling_db)
        finally:
            gpu_ctx.set_option("assume_compute_units", saved)
        assert np.array_equal(out_len2, lens) and (unleveled2, limited2) == (unleveled, limited) and same_bits(gains2, gains)
        assert same_bits(A, dev.down(d_c, (n_tracks, track_stride), np.float32)[:, :track_len])
        # a ceiling nothing reaches
        _, gains3, unleveled3, limited3 = b.mix_leveled_limited(item_rows, item_offs, level_db, d_c, track_stride, n_tracks, track_len,
                                                        item_tracks=item_tracks, mode=gmode, ceiling_db=200.0)
        _, gains4, unleveled4 = b.mix_leveled(item_rows, item_offs, level_db, d_d, track_stride, n_tracks, track_len,
                                              item_tracks=item_tracks, mode=gmode)
        assert limited3 == 0 and unleveled3 == unleveled4 == unleveled and same_bits(gains3, gains4) and same_bits(gains3, leveled)
        assert same_bits(dev.down(d_c, (n_tracks, track_stride), np.float32), dev.down(d_d, (n_tracks, track_stride), np.float32))
        # invalid: a ceiling that is no number; outputs stay as they were
        lib = G.load()
        g = np.full(len(item_rows), CANARY, np.float32)
        out, lim = C.c_uint32(99), C.c_uint32(98)
        for ceiling in (float("nan"), float("inf")):
            rc = lib.grail_batch_mix_leveled_limited(gpu_ctx.handle, b.handle, item_rows.ctypes.data, item_tracks.ctypes.data,
                                                     item_offs.ctypes.data, level_db.ctypes.data, gmode, len(item_rows), d_c,
                                                     track_stride, n_tracks, track_len, None, g.ctypes.data, C.addressof(out),
                                                     ceiling, C.addressof(lim), 0)
            assert rc == G.ERR_INVALID_ARG and np.all(g == CANARY) and (out.value, lim.value) == (99, 98)
    finally:
        b.free()


def test_limited_tracks_stay_under_the_ceiling_when_items_do_not_overlap(gpu_ctx, dev, speech8k_batch):
    """every row once, 16 to a track, eleven samples of silence between neighbours (no filter window spans two items): each
    finished track's measured true peak is at most c + (16571 / 8192) x 2^-24 x max_i(|g_i| x sample_peak_i), the second
    term being the mix's one rounding per product pushed through the taps"""
    S = speech8k_batch
    n, stride = S["n"], S["stride"]
    gpu_ctx.set_voices(S["voices"])
    b = gpu_ctx.upload(*S["batch"])
    try:
        lens = b.lengths()
        item_rows = np.arange(n, dtype=np.uint32)
        n_tracks = -(-n // 16)
        item_tracks = (item_rows // 16).astype(np.uint32)
        item_offs, track_lens = G.mix_place_sequential(lens, item_rows, item_tracks, np.full(n, 11, np.int64), n_tracks)
        track_len = int(track_lens.max())
        track_stride = (track_len + 63) // 64 * 64
        d_t = dev.alloc(n_tracks * track_stride * 4)
        ceiling_db = -9.0
        c = ceiling_of(ceiling_db)
        _, gains, unleveled, limited = b.mix_leveled_limited(item_rows, item_offs, np.full(n, -20.0, np.float32), d_t, track_stride,
                                                     n_tracks, track_len, item_tracks=item_tracks, mode=G.LEVEL_RMS,
                                                     ceiling_db=ceiling_db)
        assert unleveled == 1 and limited > n // 20, (unleveled, limited)
        d_rows, d_len = dev.alloc(n * stride * 4), dev.alloc(n * 4)
        b.synthesize_async(d_rows, stride, d_len)
        _, peak, _ = gpu_ctx.levels(d_rows, stride, d_len, n)
        track_tp, track_bad = gpu_ctx.true_peak(d_t, track_stride, dev.up(track_lens.astype(np.uint32)), n_tracks)
        assert not track_bad.any()
        reach = np.abs(gains).astype(np.float64) * peak.astype(np.float64)
        worst = -np.inf
        for t in range(n_tracks):
            bound = c + TAP_SUM * 2.0 ** -24 * reach[item_tracks == t].max()
            worst = max(worst, track_tp[t] - c)
            assert track_tp[t] <= bound, (t, track_tp[t], bound)
        print(f"\n{limited} of {n} items limited to {ceiling_db} dBTP; the loudest track reads {20 * np.log10(track_tp.max()):.6f} dBTP "
              f"({worst:+.3e} against c)")
        assert track_tp.max() > 0.9 * c                                     # the ceiling was reached, not missed by far
    finally:
        b.free()


def test_limited_mix_refuses_a_voice_table_of_two_rates_in_lufs_mode(gpu_ctx, dev):
    v = W.preset_voices(2)
    other = W.preset_voices(2, sample_rate=44100)
    segs, offs, vids, seeds, stride = W.speech_like_batch(8, np.random.default_rng(63), n_voices=2)
    item_rows = np.arange(8, dtype=np.uint32)
    item_offs = np.zeros(8, np.uint64)
    lufs = np.full(8, -23.0, np.float32)
    d_t = dev.up(np.full(stride, CANARY, np.float32))
    lib = G.load()
    gpu_ctx.set_voices([v[0], other[1]])
    b = gpu_ctx.upload(segs, offs, vids, seeds)
    try:
        g = np.full(8, CANARY, np.float32)
        out, lim, lens = C.c_uint32(99), C.c_uint32(98), np.full(8, 0xEEEEEEEE, np.uint32)
        rc = lib.grail_batch_mix_leveled_limited(gpu_ctx.handle, b.handle, item_rows.ctypes.data, None, item_offs.ctypes.data,
                                                 lufs.ctypes.data, G.LEVEL_LOUDNESS, 8, d_t, stride, 1, stride,
                                                 lens.ctypes.data, g.ctypes.data, C.addressof(out), -1.0, C.addressof(lim), 0)
        assert rc == G.ERR_INVALID_ARG and b"sample rate" in lib.grail_last_error()
        assert np.all(g == CANARY) and (out.value, lim.value) == (99, 98) and np.all(lens == 0xEEEEEEEE)
        gpu_ctx.sync()
        assert np.all(dev.down(d_t, stride, np.float32) == CANARY)
        # the other modes do not ask for a rate
        b.mix_leveled_limited(item_rows, item_offs, lufs, d_t, stride, 1, stride, mode=G.LEVEL_RMS, ceiling_db=-1.0)
    finally:
        b.free()
        gpu_ctx.set_voices(v)


# ---- full size: config 3 -------------------------------------------------------------------------------------------------
def test_full_size(gpu_ctx, dev):
    """65 536 x 96 006, true_peak_async queued right behind synthesize_async: every row's true peak is at most
    (16571 / 8192) x its sample peak from grail_levels_async (times ROUNDING of tests/test_true_peak_host.py for the binary64 adds) and no row holds a
    non-finite sample; 64 rows spread over the batch (first, last, wave and workgroup boundaries, random) equal the model
    over their downloaded samples"""
    n = 65536
    gpu_ctx.set_voices(W.single_voice())
    segs, offs, vids, seeds = W.make_batch(n)
    stride = W.max_samples()
    b = gpu_ctx.upload(segs, offs, vids, seeds)
    try:
        d_rows, d_len = dev.alloc(n * stride * 4), dev.alloc(n * 4)
        d_tp, d_bad, d_peak = dev.alloc(n * 8), dev.alloc(n * 4), dev.alloc(n * 4)
        gpu_ctx.memset(d_rows, 0xFF, n * stride * 4)                       # NaNs until the rendering has run
        b.synthesize_async(d_rows, stride, d_len)
        gpu_ctx.true_peak_async(d_rows, stride, d_len, n, d_tp, d_bad)
        gpu_ctx.levels_async(d_rows, stride, d_len, n, peak_dev=d_peak)
        gpu_ctx.sync()
    finally:
        b.free()
    tp, bad = dev.down(d_tp, n, np.float64), dev.down(d_bad, n, np.uint32)
    peak = dev.down(d_peak, n, np.float32).astype(np.float64)
    lens = dev.down(d_len, n, np.uint32)
    assert np.all(lens == 96006) and not bad.any()
    assert np.all(np.isfinite(tp)) and np.all(tp >= 0) and np.all((tp == 0) == (peak == 0))
    assert np.all(tp <= TAP_SUM * peak * ROUNDING) and np.count_nonzero(tp) > n // 2
    on = tp > 0
    over = 20.0 * np.log10(tp[on] / peak[on])
    print(f"\n{np.count_nonzero(on)} of {n} rows sound: true peak {over.min():+.3f} .. {over.max():+.3f} dB against the sample "
          f"peak, {20 * np.log10(tp.max()):+.3f} dBTP at most")
    rng = np.random.default_rng(3)
    fixed = [0, n - 1, 63, 64, 65, 127, 128, 255, 256, 257, 4095, 4096]
    sample = fixed + [int(u) for u in rng.permutation(n) if u not in fixed][:52]
    assert len(set(sample)) == 64
    for u in sample:
        x = dev.down(d_rows, int(lens[u]), np.float32, offset=u * stride * 4)
        assert same_bits(tp[u:u + 1], np.array([true_peak_model(x)[0]])), u


# ---- the example ---------------------------------------------------------------------------------------------------------
def test_grail_dialogue_ceiling_option(gpu_ctx, dev, tmp_path):
    """--lufs -23 --ceiling -1: exit status 0, and the track true peaks and the count it prints are those of the binding's
    mix_leveled_limited(ceiling_db=-1) of the same placements, measured by true_peak, to the six decimals it prints.  Without
    --ceiling the program prints no such line."""
    exe = os.path.join(ROOT, "grail-rs_amd", "lib", "grail_dialogue")
    lines = ["hello there", "a fine day to you"]
    r = subprocess.run([exe, "-o", str(tmp_path / "capped.wav"), "--lufs", "-23", "--ceiling", "-1"] + lines,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"Ceiling -1\.0 dBTP: (\d+) of 4 placements limited; track true peaks (\S+) and (\S+) dBTP", r.stdout)
    assert m, r.stdout
    plain = subprocess.run([exe, "-o", str(tmp_path / "plain.wav"), "--lufs", "-23"] + lines, capture_output=True, text=True,
                           timeout=300)
    assert plain.returncode == 0 and "Ceiling" not in plain.stdout and "dBTP" not in plain.stdout
    v0 = G.voice_generic()
    v1 = v0.copy()
    v1.center_frequency = float(np.float32(v0.center_frequency) * np.float32(1.5))
    gpu_ctx.set_voices([v0, v1])
    s0, s1 = G.text_to_phoneme_elems(v0, lines[0]), G.text_to_phoneme_elems(v1, lines[1])
    b = gpu_ctx.upload(np.concatenate([s0, s1]), [0, len(s0), len(s0) + len(s1)], [0, 1], [0, 0])
    try:
        lens = b.lengths()
        at, end = G.mix_place_sequential(lens, [0, 1], None, [0, int(np.float32(44100.0) * np.float32(3.0) / np.float32(10.0))], 1)
        track_len = int(end[0])
        track_stride = (track_len + 63) // 64 * 64
        # the program's levels: level + 20 log10(pan) in binary32, by the C library's log10f as the program calls it
        log10f = C.CDLL("libm.so.6").log10f
        log10f.restype, log10f.argtypes = C.c_float, [C.c_float]
        pans = [0.8, 0.2, 0.2, 0.8]
        levels = np.array([np.float32(-23.0) + np.float32(20.0) * np.float32(log10f(p)) for p in pans], np.float32)
        d_t = dev.alloc(2 * track_stride * 4)
        _, gains, unleveled, limited = b.mix_leveled_limited([0, 0, 1, 1], [at[0], at[0], at[1], at[1]], levels, d_t, track_stride, 2,
                                                     track_len, item_tracks=[0, 1, 0, 1], mode=G.LEVEL_LOUDNESS, ceiling_db=-1.0)
        tp, bad = gpu_ctx.true_peak(d_t, track_stride, dev.up(np.array([track_len, track_len], np.uint32)), 2)
    finally:
        b.free()
    print(f"\nprinted {m.groups()}, the binding: {limited} limited, {[G.true_peak_db(t) for t in tp]} dBTP, gains {gains}")
    assert unleveled == 0 and not bad.any() and int(m.group(1)) == limited
    assert [m.group(2), m.group(3)] == ["%.6f" % G.true_peak_db(t) for t in tp]
    assert all(G.true_peak_db(t) <= -1.0 + 1e-5 for t in tp)               # (two placements per track, one line each: no overlap)
