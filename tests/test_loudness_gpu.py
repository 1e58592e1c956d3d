"""K-weighted gated loudness on the device (include/grail_hip.h, "levels, continued"): grail_loudness_async and
grail_batch_mix_leveled in GRAIL_LEVEL_LOUDNESS, compared BIT FOR BIT with the numpy model of the contract
(tests/test_loudness_host.py: kweight_hops_model, gate_model) — on synthetic rows with every awkward length and value at
four sample rates, under every layout of the same rows, on rows the library rendered (against the model over the ORACLE's
rendering), in the leveled mix, at full size, and through the dialogue example."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import grail_hip as G
from grail_hip import workload as W
from test_levels_gpu import CANARY, Dev, _awkward, _oracle, _place, dev, fold  # noqa: F401  (dev is a fixture)
from test_levels_host import gains_model, within_one_ulp
from test_loudness_host import gate_model, kweight_hops_model, kweighting_model, lufs_model, same_bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = [8000, 22050, 48000, 192000]


def lengths_for(rate):
    H = rate // 10
    return [0, 1, H - 1, H, 4 * H - 1, 4 * H, 4 * H + 1, 96006, 1000003, 61 * H + 17]


def own_coef(rate):
    """ten doubles of the test's own: the K-weighting of another rate, the numerators a little off"""
    c = kweighting_model(rate * 3 // 2 + 7)
    c[[0, 2, 5, 7]] *= [1.0625, 0.96875, 0.875, 1.03125]
    return c


def synthetic_rows(rate, seed):
    """rows of the awkward lengths: -0.0, denormals, 3e38, NaN and +-Inf sprinkled in; the last one is loud for one hop
    and then exactly zero for six seconds (the filter's state decays through the denormal range)"""
    rng = np.random.default_rng(seed)
    H = rate // 10
    rows = [_awkward(rng, n) for n in lengths_for(rate)]
    rows[1][0] = np.float32(-0.5)
    rows[7][-1] = np.float32(np.nan)
    rows[9][:] = 0.0
    rows[9][:H] = (rng.standard_normal(H) * 0.5).astype(np.float32)
    return rows


def model_of(rows, rate, coef):
    """[(hops, gated mean square, nonfinite)] per row"""
    H = rate // 10
    return [(h, gate_model(h, H), b) for h, b in kweight_hops_model(rows, rate, coef)]


def measure(ctx, dev, rows_dev, stride, d_len, n, rate, coef=None, hs=None):
    """grail_loudness_async into arrays with a canary before and after each -> (gated [n], hops [n, hs], nonfinite [n]);
    hops past a row's last hold CANARY"""
    hs = max(stride // (rate // 10), 1) if hs is None else hs
    g0, h0, b0 = np.full(n + 2, CANARY), np.full(n * hs + 2, CANARY), np.full(n + 2, 0xABCD1234, np.uint32)
    d_g, d_h, d_b = dev.up(g0), dev.up(h0), dev.up(b0)
    ctx.loudness_async(rows_dev, stride, d_len, n, rate, coef, C.c_void_p(d_g.value + 8), C.c_void_p(d_h.value + 8), hs,
                       C.c_void_p(d_b.value + 4))
    ctx.sync()
    g, h, b = dev.down(d_g, n + 2, np.float64), dev.down(d_h, n * hs + 2, np.float64), dev.down(d_b, n + 2, np.uint32)
    assert g[0] == CANARY and g[-1] == CANARY and h[0] == CANARY and h[-1] == CANARY, "a canary around an output was written"
    assert b[0] == 0xABCD1234 and b[-1] == 0xABCD1234
    return g[1:-1], h[1:-1].reshape(n, hs), b[1:-1]


def check_rows(got, model, positions, what):
    g, h, b = got
    for i, pos in enumerate(positions):
        wh, wg, wb = model[i]
        k = len(wh)
        assert same_bits(h[pos, :k], wh), (what, i, "hops")
        assert np.all(h[pos, k:] == CANARY), (what, i, "a hop past the row's last was written")
        assert same_bits(g[pos], wg), (what, i, g[pos], wg)
        assert b[pos] == wb, (what, i, b[pos], wb)


# ---- synthetic rows ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", RATES)
def test_synthetic_rows_equal_the_model(gpu_ctx, dev, rate):
    """lengths 0, 1, H - 1, H, 4H - 1, 4H, 4H + 1, 96 006, 1 000 003 and a row that falls silent for six seconds: hop sums,
    gated mean squares and non-finite counts bit for bit, with coef NULL (grail_kweighting of the rate) and with ten
    doubles of the test's own"""
    rows = synthetic_rows(rate, 100 + rate)
    n = len(rows)
    stride = (max(len(x) for x in rows) + 63) // 64 * 64
    rows_dev, d_len, _ = _place(gpu_ctx, dev, rows, list(range(n)), n, stride)
    for coef in (None, own_coef(rate)):
        model = model_of(rows, rate, G.kweighting(rate) if coef is None else coef)
        got = measure(gpu_ctx, dev, rows_dev, stride, d_len, n, rate, coef)
        check_rows(got, model, list(range(n)), f"rate {rate}")
        assert [len(m[0]) for m in model] == [len(x) // (rate // 10) for x in rows]
        assert sum(m[2] for m in model) > 100 and all(m[1] == 0 for m in model[:5]) and model[5][1] > 0
    # the silent tail: the state decays (21 decades of z*z per hop) through the denormals to exactly zero
    tail = model[9][0]
    assert tail[0] > 1.0 and tail[-1] == 0.0 and any(0.0 < x < 1e-200 for x in tail)
    # any output may be NULL: each one alone gives the same bits
    g_only, _, _ = gpu_ctx.loudness(rows_dev, stride, d_len, n, rate, coef, hops=False)
    assert same_bits(g_only, np.array([m[1] for m in model]))
    d_b = dev.up(np.full(n, 7, np.uint32))
    gpu_ctx.loudness_async(rows_dev, stride, d_len, n, rate, nonfinite_dev=d_b)
    gpu_ctx.sync()
    assert np.array_equal(dev.down(d_b, n, np.uint32), [m[2] for m in model])


def test_invalid_arguments(gpu_ctx, dev):
    d_rows, d_len = dev.up(np.zeros(48000, np.float32)), dev.up(np.array([48000], np.uint32))
    d_h = dev.up(np.full(16, CANARY))
    for rate, hs in ((48000, 9), (48000, 0), (2559, 16), (1048577, 16), (0, 16)):
        with pytest.raises(G.GrailError) as ei:
            gpu_ctx.loudness_async(d_rows, 48000, d_len, 1, rate, None, None, d_h, hs, None)
        assert ei.value.status == G.ERR_INVALID_ARG, (rate, hs)
    gpu_ctx.sync()
    assert np.all(dev.down(d_h, 16, np.float64) == CANARY)
    gpu_ctx.loudness_async(d_rows, 48000, d_len, 1, 48000, None, None, d_h, 10, None)        # exactly row_stride / H
    gpu_ctx.sync()
    h = dev.down(d_h, 16, np.float64)
    assert np.all(h[:10] == 0.0) and np.all(h[10:] == CANARY)


# ---- layouts -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rows48k():
    rate = 48000
    rows = synthetic_rows(rate, 9)
    return dict(rate=rate, rows=rows, model=model_of(rows, rate, G.kweighting(rate)))


@pytest.mark.parametrize("n_total", [1, 63, 64, 65, 300])
def test_a_rows_numbers_do_not_depend_on_the_rows_around_it(gpu_ctx, dev, rows48k, n_total):
    """the same rows at other row indices among 1, 63, 64, 65 and 300 rows (the others hold 0x3c3c3c3c over random lengths)"""
    rate, rows, model = rows48k["rate"], rows48k["rows"], rows48k["model"]
    rng = np.random.default_rng(n_total)
    if n_total == 1:
        for i in (8, 9, 5):
            stride = (len(rows[i]) + 63) // 64 * 64
            rows_dev, d_len, _ = _place(gpu_ctx, dev, [rows[i]], [0], 1, stride)
            check_rows(measure(gpu_ctx, dev, rows_dev, stride, d_len, 1, rate), [model[i]], [0], f"alone {i}")
        return
    pos = sorted(rng.choice(n_total, len(rows), replace=False).tolist())
    pos = [pos[i] for i in rng.permutation(len(rows))]
    stride = (max(len(x) for x in rows) + 63) // 64 * 64
    rows_dev, d_len, lens = _place(gpu_ctx, dev, rows, pos, n_total, stride, 0, rng)
    g, h, b = got = measure(gpu_ctx, dev, rows_dev, stride, d_len, n_total, rate)
    check_rows(got, model, pos, f"among {n_total}")
    rest = np.setdiff1d(np.arange(n_total), pos)
    assert not b[rest].any() and np.all(np.isfinite(g[rest]))
    k = int(rest[np.argmax(lens[rest])])
    c = np.frombuffer(b"\x3c" * 4, np.float32)[0]
    check_rows((g[k:k + 1], h[k:k + 1], b[k:k + 1]), model_of([np.full(lens[k], c, np.float32)], rate, G.kweighting(rate)), [0],
               "a constant row")


@pytest.mark.parametrize("layout", ["stride4", "odd", "stride2", "offset1", "offset3", "reversed"])
def test_a_rows_numbers_do_not_depend_on_its_layout(gpu_ctx, dev, rows48k, layout):
    """row_stride a multiple of 4 but not of 64, odd, even but no multiple of 4; rows_dev 4 and 12 bytes past an
    allocation's alignment (4-byte loads instead of 16-byte ones); the rows in another order"""
    rate, rows, model = rows48k["rate"], rows48k["rows"], rows48k["model"]
    longest = max(len(x) for x in rows)
    stride = {"stride4": (longest + 3) // 4 * 4, "odd": (longest + 3) // 4 * 4 + 1, "stride2": (longest + 3) // 4 * 4 + 2}.get(
        layout, (longest + 63) // 64 * 64)
    offset = int(layout[-1]) if layout.startswith("offset") else 0
    pos = list(range(len(rows)))[::-1] if layout == "reversed" else list(range(len(rows)))
    rows_dev, d_len, _ = _place(gpu_ctx, dev, rows, pos, len(rows), stride, offset)
    check_rows(measure(gpu_ctx, dev, rows_dev, stride, d_len, len(rows), rate), model, pos, layout)


@pytest.mark.parametrize("offset", [0, 1])
def test_hops_that_end_off_a_multiple_of_eight_under_either_kind_of_load(gpu_ctx, dev, offset):
    """22 050 Hz: H = 2 205, so a hop ends at every residue of 8 within a tile of 64 samples and the samples of a run past
    its last whole eight are filtered one by one; rows48k (H = 4 800 = 75 tiles) never leaves the unrolled loop, so the
    layouts with 4-byte loads above do not reach this"""
    rate = 22050
    H = rate // 10
    assert H % 8 != 0 and 4800 % 64 == 0
    rng = np.random.default_rng(2205 + offset)
    rows = [_awkward(rng, n) for n in (0, H - 1, 4 * H + 1, 9 * H + 5)]
    stride = (9 * H + 5 + 63) // 64 * 64
    rows_dev, d_len, _ = _place(gpu_ctx, dev, rows, [0, 1, 2, 3], 4, stride, offset)
    model = model_of(rows, rate, G.kweighting(rate))
    assert [len(m[0]) for m in model] == [0, 0, 4, 9] and sum(m[2] for m in model) > 20
    check_rows(measure(gpu_ctx, dev, rows_dev, stride, d_len, 4, rate), model, [0, 1, 2, 3], f"offset {offset}")


@pytest.mark.parametrize("stride", [96008, 96007])
def test_a_len_above_row_stride_reads_as_row_stride(gpu_ctx, dev, stride):
    rate = 48000
    rng = np.random.default_rng(stride)
    rows = [_awkward(rng, stride) for _ in range(3)]
    rows_dev, _, _ = _place(gpu_ctx, dev, rows, [0, 1, 2], 3, stride)
    d_len = dev.up(np.array([stride + 1, 0xFFFFFFFF, stride], np.uint32))
    check_rows(measure(gpu_ctx, dev, rows_dev, stride, d_len, 3, rate), model_of(rows, rate, G.kweighting(rate)), [0, 1, 2],
               f"stride {stride}")


# ---- rendered rows ---------------------------------------------------------------------------------------------------------
def test_rendered_rows_against_the_model_over_the_oracles_rendering(gpu_ctx, dev):
    """64 rows of the eight preset voices, rendered by the library and measured where they lie (no sync in between),
    against the model applied to the oracle's rendering of the same rows"""
    n = 64
    voices = W.preset_voices(8)
    segs, offs, vids, seeds = W.make_batch(n, n_voices=8)
    stride = W.max_samples()
    rate = int(voices[0].sample_rate)
    gpu_ctx.set_voices(voices)
    b = gpu_ctx.upload(segs, offs, vids, seeds)
    try:
        d_rows, d_len = dev.alloc(n * stride * 4), dev.alloc(n * 4)
        b.synthesize_async(d_rows, stride, d_len)
        got = measure(gpu_ctx, dev, d_rows, stride, d_len, n, rate)
    finally:
        b.free()
    ref, ref_len = _oracle(voices, segs, offs, vids, seeds, stride)
    assert np.array_equal(dev.down(d_len, n, np.uint32), ref_len)
    model = model_of([ref[u, :ref_len[u]] for u in range(n)], rate, G.kweighting(rate))
    check_rows(got, model, list(range(n)), "rendered")
    assert not got[2].any() and np.count_nonzero(got[0]) > n // 2
    print(f"\nrendered rows read {min(lufs_model(m[1]) for m in model if m[1] > 0):.2f} .. "
          f"{max(lufs_model(m[1]) for m in model):.2f} LUFS")


# ---- the leveled mix ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def speech8k():
    """1 100 speech-like rows of two voices at 8 kHz (0.5 - 3.8 s), one of them emptied and one cut to 300 ms, and the
    oracle's rendering of them with the model's levels"""
    rate = 8000
    voices = W.preset_voices(2, sample_rate=rate)
    n = 1100
    segs, offs, vids, seeds, stride = W.speech_like_batch(n, np.random.default_rng(61), n_voices=2, sample_rate=rate)
    cut = int(offs[7])
    segs = np.concatenate([segs[:cut], segs[int(offs[8]):]])             # utterance 7 loses its segments
    offs = offs.copy()
    offs[8:] -= offs[8] - cut
    s = slice(int(offs[9]), int(offs[10]))                                # utterance 9 lasts 300 ms
    segs["length"][s] = (segs["length"][s] * (0.3 / float(segs["length"][s].sum()))).astype(np.float32)
    ref, ref_len = _oracle(voices, segs, offs, vids, seeds, stride)
    assert ref_len[7] == 0 and 0.25 * rate < ref_len[9] < 0.4 * rate and ref_len.max() <= stride
    model = model_of([ref[u, :ref_len[u]] for u in range(n)], rate, G.kweighting(rate))
    level = np.array([np.sqrt(m[1] * G.LOUDNESS_LEVEL_SCALE) for m in model])
    return dict(rate=rate, voices=voices, n=n, batch=(segs, offs, vids, seeds), ref=ref, ref_len=ref_len, level=level)


def test_leveled_mix_in_lufs(gpu_ctx, dev, speech8k):
    """grail_batch_mix_leveled(GRAIL_LEVEL_LOUDNESS): the tracks equal the mixing contract's fold over the oracle's rows
    with the gains the call returned; those gains are within one binary32 unit in the last place of the gains numpy
    derives from the model's levels of the oracle's rows; the empty and the 300-ms utterance are unleveled and counted;
    planned as ONE compute unit (several blocks) the same tracks and gains"""
    S = speech8k
    n, ref, ref_len = S["n"], S["ref"], S["ref_len"]
    gpu_ctx.set_voices(S["voices"])
    b = gpu_ctx.upload(*S["batch"])
    try:
        assert np.array_equal(b.lengths(), ref_len)
        rng = np.random.default_rng(62)
        item_rows = np.concatenate([np.arange(n), rng.integers(0, n, 300), [7, 9]]).astype(np.uint32)
        item_rows = item_rows[rng.permutation(len(item_rows))]
        n_tracks = n // 16
        item_tracks = (item_rows // 16 % n_tracks).astype(np.uint32)
        item_offs = rng.integers(0, 4000, len(item_rows)).astype(np.uint64)
        lufs = rng.uniform(-36.0, -14.0, len(item_rows)).astype(np.float32)
        track_len = 4000 + int(ref_len.max())
        track_stride = (track_len + 63) // 64 * 64
        d_a, d_c = (dev.alloc(n_tracks * track_stride * 4) for _ in range(2))
        out_len, gains, unleveled = b.mix_leveled(item_rows, item_offs, lufs, d_a, track_stride, n_tracks, track_len,
                                                  item_tracks=item_tracks, mode=G.LEVEL_LOUDNESS)
        want, want_out = gains_model(G.LEVEL_LOUDNESS, lufs, item_rows, active=S["level"])
        left_out = np.isin(item_rows, np.flatnonzero(S["level"] == 0))
        assert np.array_equal(out_len, ref_len)
        assert unleveled == want_out == int(left_out.sum()) and np.all(gains[left_out] == 0) and np.all(gains[~left_out] > 0)
        assert left_out[item_rows == 7].all() and left_out[item_rows == 9].all() and 4 <= unleveled < 12
        assert within_one_ulp(gains, want), np.max(np.abs(gains[~left_out] / want[~left_out] - 1))
        A = dev.down(d_a, (n_tracks, track_stride), np.float32)[:, :track_len]
        assert same_bits(A, fold(ref, ref_len, item_rows, item_tracks, item_offs, gains, n_tracks, track_len))
        saved = gpu_ctx.get_option("assume_compute_units")
        try:
            gpu_ctx.set_option("assume_compute_units", 1)
            assert n > 2 * 2 * 256
            out_len2, gains2, unleveled2 = b.mix_leveled(item_rows, item_offs, lufs, d_c, track_stride, n_tracks, track_len,
                                                         item_tracks=item_tracks, mode=G.LEVEL_LOUDNESS)
        finally:
            gpu_ctx.set_option("assume_compute_units", saved)
        assert np.array_equal(out_len2, ref_len) and unleveled2 == unleveled and same_bits(gains2, gains)
        assert same_bits(A, dev.down(d_c, (n_tracks, track_stride), np.float32)[:, :track_len])
        # every leveled item's row then reads its target: the model over gain * row (the product rounded to binary32,
        # as the mix rounds it), for a sample of the items
        worst = 0.0
        for i in np.flatnonzero(~left_out)[:40]:
            r = item_rows[i]
            x = np.float32(gains[i]) * ref[r, :ref_len[r]]
            worst = max(worst, abs(lufs_model(model_of([x], S["rate"], G.kweighting(S["rate"]))[0][1]) - float(lufs[i])))
        print(f"\nworst miss of the target loudness over 40 items: {worst:.2e} LU")
        assert worst <= 1e-4
    finally:
        b.free()


def test_leveled_mix_refuses_a_voice_table_of_two_rates(gpu_ctx, dev):
    v = W.preset_voices(2)
    other = W.preset_voices(2, sample_rate=44100)
    segs, offs, vids, seeds, stride = W.speech_like_batch(8, np.random.default_rng(63), n_voices=2)
    item_rows = np.arange(8, dtype=np.uint32)
    item_offs = np.zeros(8, np.uint64)
    lufs = np.full(8, -23.0, np.float32)
    d_t = dev.up(np.full(stride, CANARY, np.float32))
    lib = G.load()
    for voices in ([v[0], other[1]],):
        gpu_ctx.set_voices(voices)
        b = gpu_ctx.upload(segs, offs, vids, seeds)
        try:
            g = np.full(8, CANARY, np.float32)
            out, lens = C.c_uint32(99), np.full(8, 0xEEEEEEEE, np.uint32)
            rc = lib.grail_batch_mix_leveled(gpu_ctx.handle, b.handle, item_rows.ctypes.data, None, item_offs.ctypes.data,
                                             lufs.ctypes.data, G.LEVEL_LOUDNESS, 8, d_t, stride, 1, stride, lens.ctypes.data,
                                             g.ctypes.data, C.addressof(out), 0)
            assert rc == G.ERR_INVALID_ARG and b"sample rate" in lib.grail_last_error()
            assert np.all(g == CANARY) and out.value == 99 and np.all(lens == 0xEEEEEEEE)
            gpu_ctx.sync()
            assert np.all(dev.down(d_t, stride, np.float32) == CANARY)
            # the other modes do not ask for a rate
            b.mix_leveled(item_rows, item_offs, lufs, d_t, stride, 1, stride, mode=G.LEVEL_RMS)
        finally:
            b.free()
    gpu_ctx.set_voices(v)


# ---- full size: config 3 -------------------------------------------------------------------------------------------------
def test_full_size(gpu_ctx, dev):
    """65 536 x 96 006 at 48 kHz, loudness_async queued right behind synthesize_async:
    - every row's gated mean square is finite, and positive wherever the row is not silent (its mean square, from
      grail_levels_async, above -50 dB); a row of four silences reads 0, like its sum of squares.  (The workload draws
      every phoneme at random, so a few rows in a hundred are four silences: "positive for every row" cannot hold.
      Measured: 63 107 of the 65 536 rows read a loudness and lie above -50 dB, the other 2 429 are exactly silent.)
    - 64 sampled rows (first, last, wave boundaries, random) equal the model over the ORACLE's rendering of those rows;
    - every row mixed alone onto a track of its own at -23 LUFS and measured again by the device reads -23 LUFS within
      1e-4 dB (one binary32 rounding of the gain moves the mean square by a relative 2^-23 at most, the rounded products
      by as much again: about 1e-6 dB).  Measured: worst miss 5.1e-7 dB."""
    n, rate = 65536, 48000
    voices = W.single_voice()
    gpu_ctx.set_voices(voices)
    segs, offs, vids, seeds = W.make_batch(n)
    stride = W.max_samples()
    b = gpu_ctx.upload(segs, offs, vids, seeds)
    try:
        d_rows, d_len = dev.alloc(n * stride * 4), dev.alloc(n * 4)
        d_g, d_b, d_s = dev.alloc(n * 8), dev.alloc(n * 4), dev.alloc(n * 8)
        gpu_ctx.memset(d_rows, 0xFF, n * stride * 4)                       # NaNs until the rendering has run
        b.synthesize_async(d_rows, stride, d_len)
        gpu_ctx.loudness_async(d_rows, stride, d_len, n, rate, None, d_g, None, 0, d_b)
        gpu_ctx.levels_async(d_rows, stride, d_len, n, sumsq_dev=d_s)
        gpu_ctx.sync()
        gated, bad, sumsq = dev.down(d_g, n, np.float64), dev.down(d_b, n, np.uint32), dev.down(d_s, n, np.float64)
        lens = dev.down(d_len, n, np.uint32)
        assert np.all(lens == 96006) and not bad.any()
        assert np.all(np.isfinite(gated)) and np.all(gated >= 0)
        audible = sumsq / 96006.0 > 1e-5
        print(f"\n{np.count_nonzero(gated)} of {n} rows read a loudness, {np.count_nonzero(sumsq == 0)} are silent, "
              f"{np.count_nonzero(audible)} lie above -50 dB")
        assert np.all(gated[audible] > 0) and np.all(gated[sumsq == 0] == 0) and np.count_nonzero(audible) > n // 2
        # the sampled rows against the model over the oracle
        rng = np.random.default_rng(3)
        fixed = [0, n - 1, 63, 64, 65, 127, 128, 255, 256, 257, 4095, 4096]
        sample = fixed + [int(u) for u in rng.permutation(n) if u not in fixed][:52]
        assert len(set(sample)) == 64
        parts = [W.make_batch(1, first_utt=u) for u in sample]
        s_segs = np.concatenate([p[0] for p in parts])
        s_offs = np.arange(len(sample) + 1, dtype=np.uint32) * np.uint32(len(parts[0][0]))
        s_seeds = np.concatenate([p[3] for p in parts])
        for u, p in zip(sample, parts):
            assert np.array_equal(p[0], segs[offs[u]:offs[u + 1]]) and p[3][0] == seeds[u]
        ref, ref_len = _oracle(voices, s_segs, s_offs, np.zeros(len(sample), np.uint32), s_seeds, stride)
        model = model_of([ref[k, :ref_len[k]] for k in range(len(sample))], rate, G.kweighting(rate))
        for k, u in enumerate(sample):
            assert ref_len[k] == 96006 and same_bits(gated[u], model[k][1]), (u, gated[u], model[k][1])
        # single-item tracks at -23 LUFS, measured again
        item_rows = np.arange(n, dtype=np.uint32)
        d_t = dev.alloc(n * stride * 4)
        _, gains, unleveled = b.mix_leveled(item_rows, np.zeros(n, np.uint64), np.full(n, -23.0, np.float32), d_t, stride, n,
                                            96006, item_tracks=item_rows, mode=G.LEVEL_LOUDNESS)
        assert unleveled == np.count_nonzero(gated == 0) and np.array_equal(gains == 0, gated == 0)
        gpu_ctx.loudness_async(d_t, stride, d_len, n, rate, None, d_g, None, 0, d_b)
        gpu_ctx.sync()
        again = dev.down(d_g, n, np.float64)
        on = gated > 0
        miss = np.abs(-0.691 + 10.0 * np.log10(again[on]) + 23.0)
        print(f"tracks at -23 LUFS: worst miss {miss.max():.2e} dB")
        assert miss.max() <= 1e-4 and np.all(again[~on] == 0)
    finally:
        b.free()


# ---- the example ---------------------------------------------------------------------------------------------------------
def test_grail_dialogue_lufs_option(gpu_ctx, dev, tmp_path):
    """--lufs -23: exit status 0, a WAV of two channels, and the gains it prints are those of
    mix_leveled(mode=LEVEL_LOUDNESS) for the same two lines (to the four digits it prints)"""
    exe = os.path.join(ROOT, "grail-rs_amd", "lib", "grail_dialogue")
    lines = ["hello there", "a fine day to you"]
    path = str(tmp_path / "lufs.wav")
    r = subprocess.run([exe, "-o", path, "--lufs", "-23"] + lines, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    data = open(path, "rb").read()
    _, _, ch, rate, _, align, bits = struct.unpack("<IHHIIHH", data[16:36])
    assert (ch, rate, align, bits) == (2, 44100, 4, 16)
    m = re.search(r"Lines brought to -23\.0 LUFS: gains (\S+) and (\S+)", r.stdout)
    assert m, r.stdout
    printed = [float(m.group(1)), float(m.group(2))]
    v0 = G.voice_generic()
    v1 = v0.copy()
    v1.center_frequency = float(np.float32(v0.center_frequency) * np.float32(1.5))
    gpu_ctx.set_voices([v0, v1])
    s0, s1 = G.text_to_phoneme_elems(v0, lines[0]), G.text_to_phoneme_elems(v1, lines[1])
    b = gpu_ctx.upload(np.concatenate([s0, s1]), [0, len(s0), len(s0) + len(s1)], [0, 1], [0, 0])
    try:
        lens = b.lengths()
        track_len = int(lens.sum())
        track_stride = (track_len + 63) // 64 * 64
        d_t = dev.alloc(2 * track_stride * 4)
        _, gains, unleveled = b.mix_leveled([0, 1], [0, int(lens[0])], [-23.0, -23.0], d_t, track_stride, 2, track_len,
                                            item_tracks=[0, 1], mode=G.LEVEL_LOUDNESS)
    finally:
        b.free()
    print(f"\nprinted {printed}, mix_leveled {gains}")
    assert unleveled == 0 and np.all(gains > 0)
    # the program prints the gain of the line's own side (its level lowered by the pan, 0.8) divided by 0.8: four digits
    for p, g in zip(printed, gains):
        assert abs(p / float(g) - 1.0) <= 6e-4
