"""Levels on the device (include/grail_hip.h, "levels"): grail_levels_async, grail_frame_levels_async and
grail_batch_mix_leveled, compared BIT FOR BIT with the numpy model of the contract (tests/test_levels_host.py: frame_model,
row_model) — on synthetic rows with every awkward length and value, under every layout of the same rows, on rows the
library rendered (against the model over the ORACLE's rendering), at full size, and through the dialogue example."""
import ctypes as C
import os
import struct
import subprocess
import time

import numpy as np
import pytest

import grail_hip as G
import oracle_lib as O
from grail_hip import workload as W
from test_levels_host import frame_model, gains_model, row_model, within_one_ulp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = [0, 1, 255, 256, 257, 4095, 4096, 4097, 96006, 1000003]
FRAMES = [256, 441, 480, 4096, 65536]
CANARY = -7.25


def fold(rows, row_len, item_rows, item_tracks, item_offsets, item_gains, n_tracks, track_len):
    """the mixing contract in numpy, as tests/test_mix_gpu.py states it"""
    acc = np.zeros((n_tracks, track_len), np.float32)
    for i in np.argsort(np.asarray(item_rows), kind="stable"):
        o, r, t = int(item_offsets[i]), int(item_rows[i]), int(item_tracks[i])
        if o >= track_len:
            continue
        k = min(int(row_len[r]), track_len - o)
        acc[t, o:o + k] = acc[t, o:o + k] + np.float32(item_gains[i]) * rows[r, :k]
    return acc


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.dtype.itemsize in (4, 8)
    u = np.uint32 if a.dtype.itemsize == 4 else np.uint64
    return a.shape == b.shape and np.array_equal(a.view(u), b.view(u))


def active_model(frame_sumsq, row_len, frame=4096, floor_db=40.0):
    """the header's words for grail_active_level in numpy's binary64"""
    frames = -(-int(row_len) // frame)
    if frames == 0:
        return 0.0
    counts = np.full(frames, float(frame))
    counts[-1] = row_len - (frames - 1) * frame
    ms = np.asarray(frame_sumsq[:frames], np.float64) / counts
    if not ms.max() > 0:
        return 0.0
    s = n = np.float64(0.0)
    for f in np.nonzero(ms >= ms.max() * 10.0 ** (-floor_db / 10.0))[0]:
        s, n = s + frame_sumsq[f], n + counts[f]
    return float(np.sqrt(s / n))


class Dev:
    """a test's device buffers, freed at its end"""

    def __init__(self, ctx):
        self.ctx, self.ptrs = ctx, []

    def alloc(self, nbytes):
        p = self.ctx.device_alloc(max(int(nbytes), 4))
        self.ptrs.append(p)
        return p

    def up(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.alloc(arr.nbytes)
        self.ctx.h2d(p, arr, arr.nbytes)
        return p

    def down(self, p, shape, dtype, offset=0):
        out = np.empty(shape, dtype)
        self.ctx.d2h(out, p, out.nbytes, offset)
        return out

    def free(self):
        for p in self.ptrs:
            self.ctx.device_free(p)
        self.ptrs = []


@pytest.fixture
def dev(gpu_ctx):
    d = Dev(gpu_ctx)
    yield d
    d.free()


def _awkward(rng, n):
    """audio-sized samples with -0.0, denormals, 3e38, NaN and +-Inf sprinkled in (about one sample in sixty)"""
    x = (rng.standard_normal(n) * 0.2).astype(np.float32)
    specials = np.array([-0.0, 0.0, 1e-45, -1e-45, 1e-39, -3e-39, 3e38, -3e38, np.nan, np.inf, -np.inf, 1.0], np.float32)
    mask = rng.random(n) < 1.0 / 60.0
    x[mask] = specials[rng.integers(0, len(specials), int(mask.sum()))]
    return x


@pytest.fixture(scope="module")
def synthetic():
    """rows of the awkward lengths and what the model says of them (totals, and frames for every F of FRAMES)"""
    rng = np.random.default_rng(77)
    rows = [_awkward(rng, n) for n in LENGTHS]
    rows[1][0] = np.float32(-0.5)                       # the one-sample row holds a sample that counts
    rows[4][256] = np.float32(3e38)                     # the 257th sample, alone in its chunk
    rows[8][-1] = np.float32(np.nan)
    totals = [row_model(x) for x in rows]
    frames = {F: [frame_model(x, F) for x in rows] for F in FRAMES}
    assert sum(t[2] for t in totals) > 100 and totals[9][1] == np.float32(3e38)
    return dict(rows=rows, totals=totals, frames=frames)


def _place(ctx, dev, rows, positions, n_total, stride, offset=0, rng=None):
    """rows[i] as row positions[i] of a device buffer of n_total rows at `stride`, `offset` floats past an allocation's
    (256-byte aligned) start; the other rows hold 0x3c3c3c3c (0.0115) over a random length.  -> (rows_dev, len_dev, lens)"""
    lens = np.zeros(n_total, np.uint32)
    if n_total > len(rows):
        lens[:] = (rng or np.random.default_rng(0)).integers(0, stride + 1, n_total)
    nbytes = (n_total * stride + offset) * 4
    base = dev.alloc(nbytes)
    ctx.memset(base, 0x3C, nbytes)
    for x, pos in zip(rows, positions):
        lens[pos] = len(x)
        if len(x):
            ctx.h2d(C.c_void_p(base.value + (pos * stride + offset) * 4), np.ascontiguousarray(x), len(x) * 4)
    return C.c_void_p(base.value + offset * 4), dev.up(lens), lens


def _check_totals(ctx, synthetic, rows_dev, stride, d_len, n_total, positions, what):
    sumsq, peak, bad = ctx.levels(rows_dev, stride, d_len, n_total)
    for i, pos in enumerate(positions):
        ws, wp, wb = synthetic["totals"][i]
        assert same_bits(sumsq[pos:pos + 1], np.array([ws], np.float64)), (what, LENGTHS[i], sumsq[pos], ws)
        assert same_bits(peak[pos:pos + 1], np.array([wp], np.float32)), (what, LENGTHS[i], peak[pos], wp)
        assert bad[pos] == wb, (what, LENGTHS[i], bad[pos], wb)
    return sumsq, peak, bad


def _check_frames(ctx, synthetic, rows_dev, stride, d_len, n_total, positions, F, what):
    fs, fp = ctx.frame_levels(rows_dev, stride, d_len, n_total, F, fill=CANARY)
    assert fs.shape == (n_total, max(-(-stride // F), 1))
    for i, pos in enumerate(positions):
        ws, wp, _ = synthetic["frames"][F][i]
        k = len(ws)
        assert k == -(-LENGTHS[i] // F)
        assert same_bits(fs[pos, :k], ws), (what, F, LENGTHS[i])
        assert same_bits(fp[pos, :k], wp), (what, F, LENGTHS[i])
        assert np.all(fs[pos, k:] == CANARY) and np.all(fp[pos, k:] == CANARY), (what, F, LENGTHS[i], "canary written")


def test_synthetic_rows_equal_the_model(gpu_ctx, dev, synthetic):
    """lengths 0 ... 1 000 003 with -0.0, denormals, 3e38, NaN and +-Inf: totals, and frames of 256, 441, 480, 4096 and
    65 536 samples, bit for bit; frames past a row's end keep the canary"""
    rows = synthetic["rows"]
    stride = (max(LENGTHS) + 63) // 64 * 64
    pos = list(range(len(rows)))
    rows_dev, d_len, _ = _place(gpu_ctx, dev, rows, pos, len(rows), stride)
    _, peak, bad = _check_totals(gpu_ctx, synthetic, rows_dev, stride, d_len, len(rows), pos, "plain")
    assert peak[0] == 0 and bad[0] == 0 and peak[1] == 0.5
    for F in FRAMES:
        _check_frames(gpu_ctx, synthetic, rows_dev, stride, d_len, len(rows), pos, F, "plain")
    # any output may be NULL
    d_s = dev.up(np.full(len(rows), CANARY))
    gpu_ctx.levels_async(rows_dev, stride, d_len, len(rows), sumsq_dev=d_s)
    gpu_ctx.sync()
    assert same_bits(dev.down(d_s, len(rows), np.float64), np.array([t[0] for t in synthetic["totals"]]))
    d_p = dev.up(np.full(len(rows), CANARY, np.float32))
    gpu_ctx.levels_async(rows_dev, stride, d_len, len(rows), peak_dev=d_p)
    gpu_ctx.sync()
    assert same_bits(dev.down(d_p, len(rows), np.float32), np.array([t[1] for t in synthetic["totals"]], np.float32))


def test_invalid_frame_arguments(gpu_ctx, dev):
    d_rows, d_len = dev.up(np.zeros(4096, np.float32)), dev.up(np.array([4096], np.uint32))
    d_s = dev.up(np.full(16, CANARY))
    for frame, frames_stride in ((255, 64), (1048577, 1), (0, 1), (256, 15), (1000, 4)):
        with pytest.raises(G.GrailError) as ei:
            gpu_ctx.frame_levels_async(d_rows, 4096, d_len, 1, frame, d_s, None, frames_stride)
        assert ei.value.status == G.ERR_INVALID_ARG, (frame, frames_stride)
    gpu_ctx.sync()
    assert np.all(dev.down(d_s, 16, np.float64) == CANARY)
    gpu_ctx.frame_levels_async(d_rows, 4096, d_len, 1, 256, d_s, None, 16)          # exactly ceil(row_stride / frame)
    gpu_ctx.sync()
    assert np.all(dev.down(d_s, 16, np.float64) == 0.0)


@pytest.mark.parametrize("layout", ["stride64", "stride4", "odd", "offset1", "offset2", "offset3", "reversed"])
def test_a_rows_numbers_do_not_depend_on_its_layout(gpu_ctx, dev, synthetic, layout):
    """row_stride = the longest length rounded to 64, to 4, and odd; rows_dev 1, 2 and 3 floats past an aligned address
    (4-byte loads instead of 16-byte ones); the rows in another order: every row's totals and frames as the model's"""
    rows = synthetic["rows"]
    longest = max(LENGTHS)
    stride = {"stride64": (longest + 63) // 64 * 64, "stride4": (longest + 3) // 4 * 4, "odd": (longest + 3) // 4 * 4 + 1}.get(
        layout, (longest + 63) // 64 * 64)
    if layout == "odd":
        assert stride % 2 == 1
    offset = int(layout[-1]) if layout.startswith("offset") else 0
    pos = list(range(len(rows)))[::-1] if layout == "reversed" else list(range(len(rows)))
    rows_dev, d_len, _ = _place(gpu_ctx, dev, rows, pos, len(rows), stride, offset)
    _check_totals(gpu_ctx, synthetic, rows_dev, stride, d_len, len(rows), pos, layout)
    for F in (441, 480, 4096):
        _check_frames(gpu_ctx, synthetic, rows_dev, stride, d_len, len(rows), pos, F, layout)


LEVEL_CHUNKS = 8            # level_kernels.hip: a frame is walked in steps of eight chunks of 256 samples, what is left in one
#                             step of 2, 4 or 8 slots


def level_steps(n, F):
    """the steps level_frames_kernel takes over a row of n samples in frames of F: {"full", "tail2", "tail4", "tail8"}"""
    taken = set()
    for start in range(0, n, F):
        end = min(start + F, n)
        chunks = (end + 255) // 256 - start // 256
        if chunks >= LEVEL_CHUNKS:
            taken.add("full")
        left = chunks % LEVEL_CHUNKS
        if left:
            taken.add("tail8" if left > 4 else "tail4" if left > 2 else "tail2")
    return taken


@pytest.mark.parametrize("offset", [0, 1])
def test_frames_whose_last_step_is_of_every_size(gpu_ctx, dev, offset):
    """rows of 1 to 17 chunks as one frame each, with 16-byte loads and (the base one float off) with 4-byte ones: every
    number of chunks left over after the steps of eight, 1 to 7, meets the step of its size; LENGTHS x FRAMES leave a frame
    of 5 to 7 chunks past a multiple of eight out"""
    F = 65536
    assert not any("tail8" in level_steps(n, f) for n in LENGTHS for f in FRAMES)
    lengths = [256 * k - 3 for k in range(1, 18)]
    assert [((n + 255) // 256) % LEVEL_CHUNKS for n in lengths] == [1, 2, 3, 4, 5, 6, 7, 0, 1, 2, 3, 4, 5, 6, 7, 0, 1]
    assert set().union(*(level_steps(n, F) for n in lengths)) == {"full", "tail2", "tail4", "tail8"}
    assert {"tail8", "full"} <= level_steps(lengths[12], F) and level_steps(lengths[4], F) == {"tail8"}
    rng = np.random.default_rng(88)
    rows = [_awkward(rng, n) for n in lengths]
    stride = (max(lengths) + 63) // 64 * 64
    pos = list(range(len(rows)))
    rows_dev, d_len, _ = _place(gpu_ctx, dev, rows, pos, len(rows), stride, offset)
    fs, fp = gpu_ctx.frame_levels(rows_dev, stride, d_len, len(rows), F, fill=CANARY)
    sumsq, peak, bad = gpu_ctx.levels(rows_dev, stride, d_len, len(rows))
    assert fs.shape == (len(rows), 1)
    for i, x in enumerate(rows):
        ws, wp, _ = frame_model(x, F)
        assert same_bits(fs[i], ws) and same_bits(fp[i], wp), (offset, i, len(x))
        w = row_model(x)
        assert same_bits(sumsq[i:i + 1], np.array([w[0]])) and peak[i] == w[1] and bad[i] == w[2], (offset, i, len(x))
    assert bad.sum() > 20


@pytest.mark.parametrize("others", [1, 7, 3000])
def test_a_rows_numbers_do_not_depend_on_the_rows_around_it(gpu_ctx, dev, synthetic, others):
    """the same rows scattered among 1, 7 and 3 000 other rows (12 GB of them in the last case: the million-sample row
    sets the stride)"""
    rows = synthetic["rows"]
    rng = np.random.default_rng(others)
    n_total = len(rows) + others
    pos = sorted(rng.choice(n_total, len(rows), replace=False).tolist())
    pos = [pos[i] for i in rng.permutation(len(rows))]
    stride = (max(LENGTHS) + 63) // 64 * 64
    rows_dev, d_len, lens = _place(gpu_ctx, dev, rows, pos, n_total, stride, 0, rng)
    sumsq, peak, bad = _check_totals(gpu_ctx, synthetic, rows_dev, stride, d_len, n_total, pos, f"among {others}")
    _check_frames(gpu_ctx, synthetic, rows_dev, stride, d_len, n_total, pos, 480 if others < 3000 else 65536, f"among {others}")
    # the other rows: constant 0x3c3c3c3c samples
    c = np.frombuffer(b"\x3c" * 4, np.float32)[0]
    rest = np.setdiff1d(np.arange(n_total), pos)
    assert np.all(peak[rest] == np.where(lens[rest] > 0, c, 0)) and not bad[rest].any()
    k = int(rest[np.argmax(lens[rest])])
    assert same_bits(sumsq[k:k + 1], np.array([row_model(np.full(lens[k], c, np.float32))[0]]))


def _oracle(voices, segs, offs, vids, seeds, stride):
    ref, ref_len, _ = O.synthesize_batch_threads([O.Voice.from_buffer_copy(bytes(v)) for v in voices], segs, offs, vids, seeds,
                                                 stride, 16)
    return ref, ref_len


@pytest.mark.parametrize("corpus", ["speech", "presets"])
def test_rendered_rows_against_the_model_over_the_oracles_rendering(gpu_ctx, dev, corpus):
    """64 speech-like rows, and 64 rows of the eight preset voices (all eight formants live): rendered by the library,
    measured where they lie, against the model applied to the oracle's rendering of the same rows"""
    n = 64
    if corpus == "speech":
        voices = W.preset_voices(2)
        segs, offs, vids, seeds, stride = W.speech_like_batch(n, np.random.default_rng(21), n_voices=2)
    else:
        voices = W.preset_voices(8)
        segs, offs, vids, seeds = W.make_batch(n, n_voices=8)
        stride = W.max_samples()
    gpu_ctx.set_voices(voices)
    b = gpu_ctx.upload(segs, offs, vids, seeds)
    try:
        d_rows, d_len = dev.alloc(n * stride * 4), dev.alloc(n * 4)
        b.synthesize_async(d_rows, stride, d_len)
        sumsq, peak, bad = gpu_ctx.levels(d_rows, stride, d_len, n)            # queued behind the rendering, no sync
        fs, fp = gpu_ctx.frame_levels(d_rows, stride, d_len, n, 480, fill=CANARY)
    finally:
        b.free()
    ref, ref_len = _oracle(voices, segs, offs, vids, seeds, stride)
    assert np.array_equal(dev.down(d_len, n, np.uint32), ref_len)
    assert not bad.any() and sumsq.max() > 0
    for u in range(n):
        x = ref[u, :ref_len[u]]
        ws, wp, wb = row_model(x)
        assert same_bits(sumsq[u:u + 1], np.array([ws])) and peak[u] == wp and wb == 0, u
        ms, mp, _ = frame_model(x, 480)
        assert same_bits(fs[u, :len(ms)], ms) and same_bits(fp[u, :len(mp)], mp), u
        assert np.all(fs[u, len(ms):] == CANARY)


def _babble(n, lens, rng, extra):
    """babble-like items: every row once and `extra` rows again, 16 to a track at random offsets, levels -30 ... -6 dB"""
    item_rows = np.concatenate([np.arange(n), rng.integers(0, n, extra)]).astype(np.uint32)
    item_rows = item_rows[rng.permutation(len(item_rows))]
    n_tracks = max(1, n // 16)
    item_tracks = (item_rows // 16 % n_tracks).astype(np.uint32)
    item_offs = rng.integers(0, 4000, len(item_rows)).astype(np.uint64)
    level_db = rng.uniform(-30.0, -6.0, len(item_rows)).astype(np.float32)
    return item_rows, item_tracks, item_offs, level_db, n_tracks, 4000 + int(lens.max())


@pytest.fixture(scope="module")
def speech_rows():
    """1 300 speech-like rows of two voices (0.05 - 0.4 s) and the oracle's rendering of them with the model's numbers"""
    voices = W.preset_voices(2)
    n = 1300
    segs, offs, vids, seeds, stride = W.speech_like_batch(n, np.random.default_rng(31), n_voices=2, scale=0.1)
    ref, ref_len = _oracle(voices, segs, offs, vids, seeds, stride)
    model = [row_model(ref[u, :ref_len[u]]) for u in range(n)]
    frames = [frame_model(ref[u, :ref_len[u]], 4096)[0] for u in range(n)]
    return dict(voices=voices, n=n, batch=(segs, offs, vids, seeds), ref=ref, ref_len=ref_len,
                sumsq=np.array([m[0] for m in model]), peak=np.array([m[1] for m in model], np.float32),
                active=np.array([active_model(frames[u], ref_len[u]) for u in range(n)]))


@pytest.mark.parametrize("mode", ["rms", "peak", "active"])
def test_leveled_mix(gpu_ctx, dev, speech_rows, mode):
    """grail_batch_mix_leveled on 1 300 rendered rows, babble-like items at -30 ... -6 dB: the tracks equal grail_batch_mix
    given item_gains_out and the numpy fold over the oracle's rows with those gains; the gains are within one binary32 unit
    in the last place of the gains numpy derives from the model's levels; planned as ONE compute unit (blocks of 512 rows:
    three of them) the same tracks and gains; and every item's row then measures its target level (RMS and peak mode:
    within 1e-5 relative of 10^(dB / 20); the gain's rounding to binary32 is 6e-8)"""
    S = speech_rows
    gmode = {"rms": G.LEVEL_RMS, "peak": G.LEVEL_PEAK, "active": G.LEVEL_ACTIVE}[mode]
    gpu_ctx.set_voices(S["voices"])
    b = gpu_ctx.upload(*S["batch"])
    n, ref, ref_len = S["n"], S["ref"], S["ref_len"]
    try:
        assert np.array_equal(b.lengths(), ref_len)
        item_rows, item_tracks, item_offs, level_db, n_tracks, track_len = _babble(n, ref_len, np.random.default_rng(32), 300)
        track_stride = (track_len + 63) // 64 * 64
        d_a, d_b, d_c = (dev.alloc(n_tracks * track_stride * 4) for _ in range(3))
        out_len, gains, unleveled = b.mix_leveled(item_rows, item_offs, level_db, d_a, track_stride, n_tracks, track_len,
                                                  item_tracks=item_tracks, mode=gmode)
        assert np.array_equal(out_len, ref_len) and unleveled == 0
        A = dev.down(d_a, (n_tracks, track_stride), np.float32)[:, :track_len]
        # the same bits as grail_batch_mix with the gains that were used
        b.mix(item_rows, item_offs, d_b, track_stride, n_tracks, track_len, item_tracks=item_tracks, item_gains=gains)
        assert same_bits(A, dev.down(d_b, (n_tracks, track_stride), np.float32)[:, :track_len])
        # ... and as the numpy fold over the oracle's rows
        assert same_bits(A, fold(ref, ref_len, item_rows, item_tracks, item_offs, gains, n_tracks, track_len))
        # the gains against numpy's, from the model's levels of the oracle's rows
        want, want_out = gains_model(gmode, level_db, item_rows, sumsq=S["sumsq"], peak=S["peak"], row_len=ref_len,
                                     active=S["active"])
        assert want_out == 0 and within_one_ulp(gains, want), np.max(np.abs(gains / want - 1))
        # several blocks: the same tracks and gains
        saved = gpu_ctx.get_option("assume_compute_units")
        try:
            gpu_ctx.set_option("assume_compute_units", 1)
            assert n > 2 * 2 * 256
            out_len2, gains2, unleveled2 = b.mix_leveled(item_rows, item_offs, level_db, d_c, track_stride, n_tracks,
                                                         track_len, item_tracks=item_tracks, mode=gmode)
        finally:
            gpu_ctx.set_option("assume_compute_units", saved)
        assert np.array_equal(out_len2, ref_len) and unleveled2 == 0 and same_bits(gains2, gains)
        assert same_bits(A, dev.down(d_c, (n_tracks, track_stride), np.float32)[:, :track_len])
        # every item's row now measures its target: the level of gain * row, computed in numpy's binary64
        if mode != "active":
            target = 10.0 ** (level_db.astype(np.float64) / 20.0)
            worst = 0.0
            for i in range(len(item_rows)):
                x = ref[item_rows[i], :ref_len[item_rows[i]]].astype(np.float64) * np.float64(gains[i])
                got = np.sqrt(np.mean(x * x)) if mode == "rms" else np.abs(x).max()
                worst = max(worst, abs(got / target[i] - 1))
            print(f"\n{mode}: worst relative miss of the target level {worst:.2e}")
            assert worst <= 1e-5, worst
    finally:
        b.free()


def test_leveled_mix_of_a_batch_with_an_empty_utterance(gpu_ctx, dev):
    """an utterance of no segments renders no samples: its items get gain 0 and are counted, nothing else is disturbed"""
    voices = W.preset_voices(2)
    gpu_ctx.set_voices(voices)
    n = 40
    segs, offs, vids, seeds, stride = W.speech_like_batch(n, np.random.default_rng(41), n_voices=2, scale=0.1)
    cut = int(offs[7])
    segs = np.concatenate([segs[:cut], segs[int(offs[8]):]])             # utterance 7 loses its segments
    offs = offs.copy()
    offs[8:] -= offs[8] - cut
    b = gpu_ctx.upload(segs, offs, vids, seeds)
    try:
        lens = b.lengths()
        assert lens[7] == 0 and np.count_nonzero(lens) == n - 1
        item_rows = np.array(list(range(n)) + [7, 7, 3], np.uint32)
        item_tracks = (item_rows % 2).astype(np.uint32)
        item_offs = (np.arange(len(item_rows)) * 100).astype(np.uint64)
        level_db = np.full(len(item_rows), -20.0, np.float32)
        track_len = int(item_offs.max()) + int(lens.max())
        track_stride = (track_len + 63) // 64 * 64
        d_t = dev.alloc(2 * track_stride * 4)
        for mode in (G.LEVEL_RMS, G.LEVEL_PEAK, G.LEVEL_ACTIVE):
            _, gains, unleveled = b.mix_leveled(item_rows, item_offs, level_db, d_t, track_stride, 2, track_len,
                                                item_tracks=item_tracks, mode=mode)
            assert unleveled == 3 and np.array_equal(np.nonzero(gains == 0)[0], np.nonzero(item_rows == 7)[0])
            T = dev.down(d_t, (2, track_stride), np.float32)[:, :track_len]
            assert np.isfinite(T).all() and np.abs(T).max() > 0
        ref, ref_len = _oracle(voices, segs, offs, vids, seeds, stride)
        assert same_bits(T, fold(ref, ref_len, item_rows, item_tracks, item_offs, gains, 2, track_len))
        # invalid arguments: as grail_batch_mix, and the outputs stay as they were
        lib = G.load()
        g = np.full(len(item_rows), CANARY, np.float32)
        out = C.c_uint32(99)
        bad_rows = item_rows.copy()
        bad_rows[0] = n
        for rows, mode, db in ((bad_rows, G.LEVEL_RMS, level_db), (item_rows, 5, level_db), (item_rows, G.LEVEL_RMS, None)):
            rc = lib.grail_batch_mix_leveled(gpu_ctx.handle, b.handle, rows.ctypes.data, item_tracks.ctypes.data,
                                             item_offs.ctypes.data, None if db is None else db.ctypes.data, mode, len(rows),
                                             d_t, track_stride, 2, track_len, None, g.ctypes.data, C.addressof(out), 0)
            assert rc == G.ERR_INVALID_ARG and np.all(g == CANARY) and out.value == 99
        assert same_bits(T, dev.down(d_t, (2, track_stride), np.float32)[:, :track_len])
    finally:
        b.free()


# ---- full size: config 3 -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def config3(gpu_ctx):
    gpu_ctx.set_voices(W.single_voice())
    n = 65536
    segs, offs, vids, seeds = W.make_batch(n)
    stride = W.max_samples()
    b = gpu_ctx.upload(segs, offs, vids, seeds)
    d_rows, d_len = gpu_ctx.device_alloc(n * stride * 4), gpu_ctx.device_alloc(n * 4)
    d_out = [gpu_ctx.device_alloc(n * k) for k in (8, 4, 4)]
    yield dict(batch=b, d_rows=d_rows, d_len=d_len, d_out=d_out, stride=stride, n=n)
    for p in [d_rows, d_len] + d_out:
        gpu_ctx.device_free(p)
    b.free()


def test_full_size_levels_right_behind_the_rendering(gpu_ctx, dev, config3):
    """65 536 x 96 006: levels_async queued behind synthesize_async with no sync in between; peak equals
    grail_batch_digest's maxabs for every row, nonfinite is 0; 32 sampled rows copied back against the model"""
    c = config3
    n, stride = c["n"], c["stride"]
    gpu_ctx.set_voices(W.single_voice())
    gpu_ctx.memset(c["d_rows"], 0xFF, n * stride * 4)                      # NaNs until the rendering has run
    c["batch"].synthesize_async(c["d_rows"], stride, c["d_len"])
    gpu_ctx.levels_async(c["d_rows"], stride, c["d_len"], n, *c["d_out"])
    gpu_ctx.sync()
    sumsq = dev.down(c["d_out"][0], n, np.float64)
    peak = dev.down(c["d_out"][1], n, np.float32)
    bad = dev.down(c["d_out"][2], n, np.uint32)
    lens = dev.down(c["d_len"], n, np.uint32)
    _, maxabs, dbad = gpu_ctx.digest(c["d_rows"], stride, c["d_len"], n)
    assert not bad.any() and not dbad.any()
    assert same_bits(peak, maxabs)
    assert np.count_nonzero(sumsq) > n // 2 and np.all(lens == 96006)      # (a row of silences alone is silent)
    rng = np.random.default_rng(3)
    fixed = [0, n - 1, 63, 64, 65, 255, 256, 257, 4095, 4096]             # first, last, wave and workgroup boundaries
    sample = fixed + [int(u) for u in rng.permutation(n) if u not in fixed][:22]
    for u in sample:
        x = dev.down(c["d_rows"], int(lens[u]), np.float32, offset=u * stride * 4)
        ws, wp, wb = row_model(x)
        assert same_bits(sumsq[u:u + 1], np.array([ws])) and peak[u] == wp and wb == 0, u
    assert len(set(sample)) == 32


@pytest.mark.perf
def test_levels_cost_no_more_than_the_digest_and_the_leveled_mix_two_more(gpu_ctx, dev, config3):
    """wall clock around call + sync, best of three after a warm-up, on the config-3 rows:
    1. levels_async + sync at most 1.10 x grail_batch_digest on the same buffer (the parent commit's code reading the
       same bytes; 10 % is the spread of this pool's boxes and of consecutive runs);
    2. grail_batch_mix_leveled of the babble case (RMS) at most grail_batch_mix of the same items plus twice that digest
       time (one extra read of every rendered sample, and the per-block copy and wait)."""
    from conftest import skip_if_clocks_unstable
    c = config3
    n, stride = c["n"], c["stride"]
    gpu_ctx.set_voices(W.single_voice())
    c["batch"].synthesize_async(c["d_rows"], stride, c["d_len"])
    gpu_ctx.sync()
    lens = dev.down(c["d_len"], n, np.uint32)

    def best(fn):
        ms = []
        for rep in range(4):
            t0 = time.perf_counter()
            fn()
            if rep:
                ms.append(1e3 * (time.perf_counter() - t0))
        return min(ms)

    def levels():
        gpu_ctx.levels_async(c["d_rows"], stride, c["d_len"], n, *c["d_out"])
        gpu_ctx.sync()

    digest_ms = best(lambda: gpu_ctx.digest(c["d_rows"], stride, c["d_len"], n))
    levels_ms = best(levels)
    gb = n * 96006 * 4 / 1e9
    lines = [f"levels_async + sync {levels_ms:.2f} ms ({gb / levels_ms:.2f} TB/s) against grail_batch_digest "
             f"{digest_ms:.2f} ms ({gb / digest_ms:.2f} TB/s) = {levels_ms / digest_ms:.3f} x"]
    misses = [lines[-1]] if levels_ms > 1.10 * digest_ms else []
    item_rows, item_tracks, offs, gains, n_tracks, track_len = W.mix_case("babble", lens)
    level_db = np.random.default_rng(5).uniform(-30.0, -6.0, len(item_rows)).astype(np.float32)
    track_stride = (track_len + 63) // 64 * 64
    d_t = dev.alloc(n_tracks * track_stride * 4)
    b = c["batch"]
    mix_ms = best(lambda: b.mix(item_rows, offs, d_t, track_stride, n_tracks, track_len, item_tracks=item_tracks,
                                item_gains=gains))
    leveled_ms = best(lambda: b.mix_leveled(item_rows, offs, level_db, d_t, track_stride, n_tracks, track_len,
                                            item_tracks=item_tracks, mode=G.LEVEL_RMS))
    lines.append(f"grail_batch_mix_leveled {leveled_ms:.2f} ms against grail_batch_mix {mix_ms:.2f} ms + 2 x {digest_ms:.2f} ms "
                 f"= {mix_ms + 2 * digest_ms:.2f} ms")
    if leveled_ms > mix_ms + 2 * digest_ms:
        misses.append(lines[-1])
    print("\n" + "\n".join(lines))
    if misses:
        skip_if_clocks_unstable(gpu_ctx, "a level measurement missed its bar:\n" + "\n".join(misses))
    assert not misses, misses


# ---- the example ---------------------------------------------------------------------------------------------------------
def test_grail_dialogue_level_option(gpu_ctx, tmp_path):
    """--level -20: both lines' RMS in the written file within 0.1 dB of each other, and of -20 dB, after undoing the channel
    placement (0.8 of a line on its own side; the tolerance is for the rounding to 16 bits); without the option the bytes
    the program writes do not depend on this feature (tests/test_mix_gpu.py compares them with the plain mix)"""
    exe = os.path.join(ROOT, "grail-rs_amd", "lib", "grail_dialogue")
    lines = ["hello there", "a fine day to you"]
    paths = [str(tmp_path / name) for name in ("level.wav", "plain.wav", "plain2.wav")]
    for path, opt in zip(paths, (["--level", "-20"], [], [])):
        r = subprocess.run([exe, "-o", path] + opt + lines, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
    assert open(paths[1], "rb").read() == open(paths[2], "rb").read()
    data = open(paths[0], "rb").read()
    assert len(data) == len(open(paths[1], "rb").read())
    _, _, ch, rate, _, align, bits = struct.unpack("<IHHIIHH", data[16:36])
    assert (ch, rate, align, bits) == (2, 44100, 4, 16)
    frames = np.frombuffer(data[44:], "<i2").reshape(-1, 2).astype(np.float64) / 32767.0
    # where each line lies on the timeline, from the library's own clock
    v0 = G.voice_generic()
    v1 = v0.copy()
    v1.center_frequency = float(np.float32(v0.center_frequency) * np.float32(1.5))
    gpu_ctx.set_voices([v0, v1])
    s0, s1 = G.text_to_phoneme_elems(v0, lines[0]), G.text_to_phoneme_elems(v1, lines[1])
    b = gpu_ctx.upload(np.concatenate([s0, s1]), [0, len(s0), len(s0) + len(s1)], [0, 1], [0, 0])
    try:
        lens = b.lengths()
    finally:
        b.free()
    at, end = G.mix_place_sequential(lens, [0, 1], None, [0, int(np.float32(44100.0) * np.float32(3.0) / np.float32(10.0))], 1)
    assert len(frames) == int(end[0]) and at[1] >= at[0] + lens[0]            # the lines do not overlap
    db = []
    for line, side in ((0, 0), (1, 1)):
        x = frames[int(at[line]):int(at[line]) + int(lens[line]), side] / 0.8
        db.append(10 * np.log10(np.mean(x * x)))
    print(f"\nlines at {db[0]:.3f} dB and {db[1]:.3f} dB")
    assert abs(db[0] - db[1]) <= 0.1 and abs(db[0] + 20.0) <= 0.1 and abs(db[1] + 20.0) <= 0.1
