"""Mixing on the device (include/grail_hip.h, "mixing"): grail_mix_async, grail_batch_mix, grail_pcm16_frames_async and the
dialogue example.  Every track sample is the left fold, in ascending row order (ties in the order given), of gain * x over
the items that cover it — compared bit for bit, NaN positions included, with numpy's float32 fold
acc[o:o+n] = acc[o:o+n] + float32(g) * row[:n] (a product rounded, then a sum rounded)."""
import os
import struct
import subprocess
import time

import numpy as np
import pytest

import grail_hip as G
import oracle_lib as O
from grail_hip import workload as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fold(rows, row_len, item_rows, item_tracks, item_offsets, item_gains, n_tracks, track_len, init=None, stats=False):
    """the contract in numpy (init: the tracks' contents for GRAIL_MIX_ACCUMULATE).  stats: also per sample the covering
    items, the sum of their |gain| and the largest |partial sum| of the fold"""
    acc = np.zeros((n_tracks, track_len), np.float32) if init is None else np.array(init[:, :track_len], np.float32)
    n = len(item_rows)
    tracks = np.zeros(n, np.uint32) if item_tracks is None else np.asarray(item_tracks)
    gains = np.ones(n, np.float32) if item_gains is None else np.asarray(item_gains, np.float32)
    if stats:
        cnt, sabs, part = np.zeros(acc.shape, np.int64), np.zeros(acc.shape), np.abs(acc.astype(np.float64))
    for i in np.argsort(np.asarray(item_rows), kind="stable"):
        o, r, t = int(item_offsets[i]), int(item_rows[i]), int(tracks[i])
        if o >= track_len:
            continue
        k = min(int(row_len[r]), track_len - o)
        acc[t, o:o + k] = acc[t, o:o + k] + np.float32(gains[i]) * rows[r, :k]
        if stats:
            cnt[t, o:o + k] += 1
            sabs[t, o:o + k] += abs(float(gains[i]))
            part[t, o:o + k] = np.maximum(part[t, o:o + k], np.abs(acc[t, o:o + k]))
    return (acc, cnt, sabs, part) if stats else acc


def same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


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


def _special(rng, shape):
    """mixed magnitudes (denormals to 2^100) with -0.0, +-Inf, NaN and the smallest denormal sprinkled in"""
    x = (rng.uniform(-1.0, 1.0, shape) * np.exp2(rng.integers(-140, 100, shape).astype(np.float64))).astype(np.float32)
    specials = np.array([-0.0, 0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1.0], np.float32)
    mask = rng.random(shape) < 0.03
    x[mask] = specials[rng.integers(0, len(specials), int(mask.sum()))]
    return x


@pytest.mark.parametrize("accumulate", [False, True])
def test_arithmetic_bit_for_bit_against_numpy(gpu_ctx, dev, accumulate):
    """random rows with -0.0, denormals, +-Inf, NaN and mixed magnitudes; items across and past track_len, zero-length rows,
    gains 0 / -0.0 / 1 / negative / denormal, passed shuffled; canaries between track_len and track_stride untouched; the
    same bits on a device planned as 4 compute units (other spans, tiles, samples per lane)"""
    rng = np.random.default_rng(11 + accumulate)
    n_rows, row_stride = 40, 3007
    row_len = rng.integers(0, row_stride + 1, n_rows).astype(np.uint32)
    row_len[:3] = [0, row_stride, 1]
    rows = _special(rng, (n_rows, row_stride))
    n_tracks, track_len, track_stride = 5, 9003, 9064
    n = 300
    item_rows = rng.integers(0, n_rows, n).astype(np.uint32)
    item_tracks = rng.integers(0, n_tracks, n).astype(np.uint32)
    offs = rng.integers(0, track_len, n).astype(np.uint64)
    offs[::7] = track_len - rng.integers(1, 500, len(offs[::7]))                 # across track_len
    offs[::11] = track_len + rng.integers(0, 1000, len(offs[::11]))              # wholly past it
    offs[5] = 2 ** 63
    gains = rng.uniform(-2.0, 2.0, n).astype(np.float32)
    gains[:6] = [0.0, -0.0, 1.0, -1.0, 1e-40, -3e-39]
    perm = rng.permutation(n)
    item_rows, item_tracks, offs, gains = item_rows[perm], item_tracks[perm], offs[perm], gains[perm]
    init = _special(rng, (n_tracks, track_stride))
    init[:, track_len:] = np.float32(-7.25)                                       # canaries
    d_rows = dev.up(rows)
    want = fold(rows, row_len, item_rows, item_tracks, offs, gains, n_tracks, track_len, init if accumulate else None)
    saved = gpu_ctx.get_option("assume_compute_units")
    try:
        for cus in (0, 4):
            gpu_ctx.set_option("assume_compute_units", cus)
            d_tracks = dev.up(init)
            gpu_ctx.mix_async(d_rows, row_stride, row_len, item_rows, offs, d_tracks, track_stride, n_tracks, track_len,
                              item_tracks=item_tracks, item_gains=gains, accumulate=accumulate)
            gpu_ctx.sync()
            got = dev.down(d_tracks, (n_tracks, track_stride), np.float32)
            assert same_bits(got[:, :track_len], want), cus
            assert np.array_equal(got[:, track_len:].view(np.uint32), init[:, track_len:].view(np.uint32)), "canary written"
    finally:
        gpu_ctx.set_option("assume_compute_units", saved)
    # NULL tracks and gains: every item on track 0 with gain 1.0
    d_tracks = dev.up(init)
    gpu_ctx.mix_async(d_rows, row_stride, row_len, item_rows, offs, d_tracks, track_stride, n_tracks, track_len,
                      accumulate=accumulate)
    gpu_ctx.sync()
    got = dev.down(d_tracks, (n_tracks, track_stride), np.float32)
    assert same_bits(got[:, :track_len], fold(rows, row_len, item_rows, None, offs, None, n_tracks, track_len,
                                              init if accumulate else None))


def _rendered(gpu_ctx, dev, n, length):
    gpu_ctx.set_voices(W.single_voice())
    segs, offs, vids, seeds = W.make_batch(n, length=length, blend_length=length)
    stride = W.max_samples(length=length)
    b = gpu_ctx.upload(segs, offs, vids, seeds)
    d_rows, d_len = dev.alloc(n * stride * 4), dev.alloc(n * 4)
    b.synthesize_async(d_rows, stride, d_len)
    gpu_ctx.sync()
    b.free()
    return d_rows, stride, dev.down(d_len, n, np.uint32), dev.down(d_rows, (n, stride), np.float32)


def _mix_and_check(gpu_ctx, dev, d_rows, stride, lens, rows, item_rows, item_tracks, offs, gains, n_tracks, track_len):
    track_stride = (track_len + 63) // 64 * 64 + 64
    d_t = dev.alloc(n_tracks * track_stride * 4)
    gpu_ctx.mix_async(d_rows, stride, lens, item_rows, offs, d_t, track_stride, n_tracks, track_len, item_tracks=item_tracks,
                      item_gains=gains)
    gpu_ctx.sync()
    got = dev.down(d_t, (n_tracks, track_stride), np.float32)[:, :track_len]
    assert same_bits(got, fold(rows, lens, item_rows, item_tracks, offs, gains, n_tracks, track_len))


def test_sparse_dense_and_stereo_regimes_on_rendered_rows(gpu_ctx, dev):
    """device-rendered rows: 4 096 rows concatenated on 4 tracks with overlaps (long spans, 8 samples per lane), 2 048 rows
    stacked on one track within a 1 000-sample window (short spans), and a stereo pan (two items per row)"""
    rng = np.random.default_rng(21)
    n = 4096
    d_rows, stride, lens, rows = _rendered(gpu_ctx, dev, n, 0.05)
    item_rows = np.arange(n, dtype=np.uint32)
    item_tracks = (item_rows % 4).astype(np.uint32)
    gaps = rng.integers(-3000, 3000, n).astype(np.int64)
    gaps[:4] = np.abs(gaps[:4])
    offs, tl = G.mix_place_sequential(lens, item_rows, item_tracks, gaps, 4)
    gains = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    _mix_and_check(gpu_ctx, dev, d_rows, stride, lens, rows, item_rows, item_tracks, offs, gains, 4, int(tl.max()))
    # dense: 2 048 rows on one track
    pick = rng.permutation(n)[:2048].astype(np.uint32)
    offs = rng.integers(0, 1000, 2048).astype(np.uint64)
    _mix_and_check(gpu_ctx, dev, d_rows, stride, lens, rows, pick, None, offs, rng.uniform(-1, 1, 2048).astype(np.float32), 1,
                   1000 + int(lens.max()))
    # stereo: 512 rows on a timeline, each on both tracks (left gain, right gain), items interleaved
    m = 512
    at, tl = G.mix_place_sequential(lens[:m], np.arange(m), None, rng.integers(-500, 2000, m).clip(0, None), 1)
    pan = rng.uniform(0, 1, m).astype(np.float32)
    item_rows = np.repeat(np.arange(m, dtype=np.uint32), 2)
    item_tracks = np.tile(np.array([0, 1], np.uint32), m)
    gains = np.stack([np.float32(1) - pan, pan], 1).reshape(-1).astype(np.float32)
    _mix_and_check(gpu_ctx, dev, d_rows, stride, lens, rows, item_rows, item_tracks, np.repeat(at, 2), gains, 2, int(tl[0]))


def test_long_spans_with_list_tiles_of_several_spans(gpu_ctx, dev):
    """the long regime where a list tile holds several workgroup spans: planned for 256 compute units, 4 tracks of 800 000
    samples take 8 samples per lane in spans of 2 048, and items of 40 000 samples make list tiles of 4 spans (mix_plan.cpp:
    up to a quarter of the items' mean length) — so the workgroups of a tile skip the items that miss their span"""
    rng = np.random.default_rng(31)
    n_rows, row_stride = 80, 40000
    row_len = np.full(n_rows, row_stride, np.uint32)
    row_len[::9] = rng.integers(16385, row_stride, len(row_len[::9]))
    rows = _special(rng, (n_rows, row_stride))
    n_tracks, track_len, track_stride = 4, 800000, 800064
    n = 200
    item_rows = rng.integers(0, n_rows, n).astype(np.uint32)
    item_tracks = rng.integers(0, n_tracks, n).astype(np.uint32)
    offs = rng.integers(0, track_len - 30000, n).astype(np.uint64)
    gains = rng.uniform(-1.5, 1.5, n).astype(np.float32)
    init = _special(rng, (n_tracks, track_stride))
    d_rows = dev.up(rows)
    saved = gpu_ctx.get_option("assume_compute_units")
    try:
        gpu_ctx.set_option("assume_compute_units", 256)
        for accumulate in (False, True):
            d_t = dev.up(init)
            gpu_ctx.mix_async(d_rows, row_stride, row_len, item_rows, offs, d_t, track_stride, n_tracks, track_len,
                              item_tracks=item_tracks, item_gains=gains, accumulate=accumulate)
            gpu_ctx.sync()
            got = dev.down(d_t, (n_tracks, track_stride), np.float32)
            want = fold(rows, row_len, item_rows, item_tracks, offs, gains, n_tracks, track_len, init if accumulate else None)
            assert same_bits(got[:, :track_len], want), accumulate
            assert np.array_equal(got[:, track_len:].view(np.uint32), init[:, track_len:].view(np.uint32))
    finally:
        gpu_ctx.set_option("assume_compute_units", saved)


def test_batch_mix_skips_blocks_no_item_reads(gpu_ctx, dev):
    """three blocks of 2 048 rows ("assume_compute_units" = 4), items only on rows of the first and the last: the middle block
    is not rendered, and the tracks equal mix_async over the batch rendered in one piece (with and without accumulate)"""
    gpu_ctx.set_voices(W.single_voice())
    n = 5000
    segs, offs, vids, seeds = W.make_batch(n, length=0.02, blend_length=0.02)
    b = gpu_ctx.upload(segs, offs, vids, seeds)
    try:
        lens = b.lengths()
        rng = np.random.default_rng(12)
        item_rows = np.concatenate([rng.integers(0, 2048, 300), rng.integers(4096, n, 300)]).astype(np.uint32)
        item_rows = item_rows[rng.permutation(len(item_rows))]
        k = len(item_rows)
        item_tracks = rng.integers(0, 2, k).astype(np.uint32)
        track_len, track_stride = 30000, 30016
        item_offs = rng.integers(0, track_len, k).astype(np.uint64)
        gains = rng.uniform(-1, 1, k).astype(np.float32)
        init = _special(rng, (2, track_stride))
        rstride = (int(lens.max()) + 63) // 64 * 64
        d_rows, d_len = dev.alloc(n * rstride * 4), dev.alloc(n * 4)
        b.synthesize_async(d_rows, rstride, d_len)
        gpu_ctx.sync()
        for accumulate in (False, True):
            d_a, d_b = dev.up(init), dev.up(init)
            saved = gpu_ctx.get_option("assume_compute_units")
            try:
                gpu_ctx.set_option("assume_compute_units", 4)
                out_len = b.mix(item_rows, item_offs, d_a, track_stride, 2, track_len, item_tracks=item_tracks,
                                item_gains=gains, accumulate=accumulate)
            finally:
                gpu_ctx.set_option("assume_compute_units", saved)
            assert np.array_equal(out_len, lens)
            gpu_ctx.mix_async(d_rows, rstride, lens, item_rows, item_offs, d_b, track_stride, 2, track_len,
                              item_tracks=item_tracks, item_gains=gains, accumulate=accumulate)
            gpu_ctx.sync()
            A = dev.down(d_a, (2, track_stride), np.float32)
            B = dev.down(d_b, (2, track_stride), np.float32)
            assert same_bits(A, B), accumulate
    finally:
        b.free()


def test_batch_mix_in_blocks_equals_the_whole_batch_mixed_and_the_oracle(gpu_ctx, dev):
    """a speech-like batch of two voices, 5 000 rows: with "assume_compute_units" = 4 the header's block rule gives blocks of
    2 048 rows (three blocks); Batch.mix equals mix_async over the batch rendered in one piece, and both equal the numpy mix
    of the oracle's rows; out_len equals Batch.lengths()"""
    voices = W.preset_voices(2)
    gpu_ctx.set_voices(voices)
    n = 5000
    segs, offs, vids, seeds, _ = W.speech_like_batch(n, np.random.default_rng(5), n_voices=2, scale=0.1)
    b = gpu_ctx.upload(segs, offs, vids, seeds)
    try:
        lens = b.lengths()
        rng = np.random.default_rng(6)
        item_rows = np.concatenate([np.arange(n), rng.integers(0, n, 700)]).astype(np.uint32)
        k = len(item_rows)
        perm = rng.permutation(k)
        item_rows = item_rows[perm]
        item_tracks = rng.integers(0, 3, k).astype(np.uint32)
        track_len = 60000
        item_offs = rng.integers(0, track_len - 2000, k).astype(np.uint64)
        gains = rng.uniform(-1, 1, k).astype(np.float32)
        track_stride = track_len + 64
        d_a, d_b = dev.alloc(3 * track_stride * 4), dev.alloc(3 * track_stride * 4)
        saved = gpu_ctx.get_option("assume_compute_units")
        try:
            gpu_ctx.set_option("assume_compute_units", 4)
            assert n > 2 * 2 * 256 * 4                       # at least three blocks of 2 x 256 x 4 rows
            out_len = b.mix(item_rows, item_offs, d_a, track_stride, 3, track_len, item_tracks=item_tracks, item_gains=gains)
        finally:
            gpu_ctx.set_option("assume_compute_units", saved)
        assert np.array_equal(out_len, lens)
        rstride = (int(lens.max()) + 63) // 64 * 64
        d_rows, d_len = dev.alloc(n * rstride * 4), dev.alloc(n * 4)
        b.synthesize_async(d_rows, rstride, d_len)
        gpu_ctx.mix_async(d_rows, rstride, lens, item_rows, item_offs, d_b, track_stride, 3, track_len,
                          item_tracks=item_tracks, item_gains=gains)
        gpu_ctx.sync()
        A = dev.down(d_a, (3, track_stride), np.float32)[:, :track_len]
        B = dev.down(d_b, (3, track_stride), np.float32)[:, :track_len]
        assert same_bits(A, B)
        ref, ref_len, _ = O.synthesize_batch_threads([O.Voice.from_buffer_copy(bytes(v)) for v in voices], segs, offs, vids, seeds,
                                                  rstride, 16)
        assert np.array_equal(ref_len, lens)
        assert same_bits(A, fold(ref, ref_len, item_rows, item_tracks, item_offs, gains, 3, track_len))
    finally:
        b.free()


def test_batch_mix_in_fast_arithmetic_within_the_stated_bound(gpu_ctx, dev):
    """per sample |fast - exact| <= sum |g| * GRAIL_FAST_TOLERANCE + k * 2^-24 * max |partial sum| over the k covering items"""
    gpu_ctx.set_voices(W.single_voice())
    n = 3000
    segs, offs, vids, seeds = W.make_batch(n, length=0.05, blend_length=0.05)
    b = gpu_ctx.upload(segs, offs, vids, seeds)
    try:
        lens = b.lengths()
        rng = np.random.default_rng(8)
        item_rows = rng.permutation(n).astype(np.uint32)
        item_tracks = rng.integers(0, 2, n).astype(np.uint32)
        track_len = 40000
        item_offs = rng.integers(0, track_len, n).astype(np.uint64)
        gains = rng.uniform(-1, 1, n).astype(np.float32)
        track_stride = track_len + 64
        d_e, d_f = dev.alloc(2 * track_stride * 4), dev.alloc(2 * track_stride * 4)
        b.mix(item_rows, item_offs, d_e, track_stride, 2, track_len, item_tracks=item_tracks, item_gains=gains)
        saved = gpu_ctx.get_option("arithmetic")
        try:
            gpu_ctx.set_option("arithmetic", 1)
            b.mix(item_rows, item_offs, d_f, track_stride, 2, track_len, item_tracks=item_tracks, item_gains=gains)
        finally:
            gpu_ctx.set_option("arithmetic", saved)
        E = dev.down(d_e, (2, track_stride), np.float32)[:, :track_len].astype(np.float64)
        F = dev.down(d_f, (2, track_stride), np.float32)[:, :track_len].astype(np.float64)
        rstride = (int(lens.max()) + 63) // 64 * 64
        d_rows, d_len = dev.alloc(n * rstride * 4), dev.alloc(n * 4)
        b.synthesize_async(d_rows, rstride, d_len)
        gpu_ctx.sync()
        rows = dev.down(d_rows, (n, rstride), np.float32)
        acc, cnt, sabs, part = fold(rows, lens, item_rows, item_tracks, item_offs, gains, 2, track_len, stats=True)
        assert same_bits(acc, E.astype(np.float32))
        bound = sabs * G.FAST_TOLERANCE + cnt * 2.0 ** -24 * part
        assert np.all(np.abs(F - E) <= bound), float(np.max(np.abs(F - E) - bound))
        assert np.any(F != E)                               # (the fast rows are not the exact ones)
    finally:
        b.free()


@pytest.mark.parametrize("n_tracks", [1, 2, 6])
def test_pcm16_frames_interleave(gpu_ctx, dev, n_tracks):
    rng = np.random.default_rng(n_tracks)
    n_frames, track_stride = 10007, 10048
    tracks = rng.uniform(-1.5, 1.5, (n_tracks, track_stride)).astype(np.float32)
    specials = np.array([np.nan, np.inf, -np.inf, -0.0, 1.0, -1.0, 1.00002, -1.00004, 3e-5, -3e-5], np.float32)
    mask = rng.random(tracks.shape) < 0.05
    tracks[mask] = specials[rng.integers(0, len(specials), int(mask.sum()))]
    d_t = dev.up(tracks)
    d_f = dev.alloc(n_frames * n_tracks * 2)
    gpu_ctx.pcm16_frames_async(d_t, track_stride, n_tracks, n_frames, d_f)
    gpu_ctx.sync()
    got = dev.down(d_f, (n_frames, n_tracks), np.int16)
    v = tracks[:, :n_frames].T * np.float32(32767.0)
    want = np.where(np.isnan(v), 0, np.clip(np.trunc(np.nan_to_num(v, nan=0.0, posinf=1e9, neginf=-1e9)), -32768, 32767))
    assert np.array_equal(got, want.astype(np.int16))


FRAMES_GRID_CAP = 65536          # launch_pcm16_frames' largest grid (test_kernel_paths_host.py): workgroups of 256 lanes, one element each


@pytest.fixture(scope="module")
def samples_for_two_laps():
    """2^24 + 262 samples with the contents of test_pcm16_frames_interleave (specials mixed in), made once and never changed"""
    rng = np.random.default_rng(24)
    n = 2 * (8_388_608 + 131)
    x = rng.uniform(-1.5, 1.5, n).astype(np.float32)
    specials = np.array([np.nan, np.inf, -np.inf, -0.0, 1.0, -1.0, 1.00002, -1.00004, 3e-5, -3e-5], np.float32)
    mask = rng.random(n) < 0.05
    x[mask] = specials[rng.integers(0, len(specials), int(mask.sum()))]
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("n_tracks,n_frames", [(2, 8_388_608 + 131), (3, 5_592_406)])
def test_pcm16_frames_second_lap_of_the_grid(gpu_ctx, dev, samples_for_two_laps, n_tracks, n_frames):
    """more elements than the capped grid has lanes: a lane takes a second element, gridDim.x * 256 further on (262 of them,
    and exactly two).  The whole result against the expression of test_pcm16_frames_interleave"""
    lanes = FRAMES_GRID_CAP * 256
    total = n_frames * n_tracks
    assert total > lanes and total - lanes == (262 if n_tracks == 2 else 2) and total <= len(samples_for_two_laps)
    tracks = samples_for_two_laps[:total].reshape(n_tracks, n_frames)
    d_t = dev.up(tracks)
    d_f = dev.alloc(total * 2)
    gpu_ctx.memset(d_f, 0x5A, total * 2)
    gpu_ctx.pcm16_frames_async(d_t, n_frames, n_tracks, n_frames, d_f)
    gpu_ctx.sync()
    got = dev.down(d_f, total, np.int16)
    with np.errstate(invalid="ignore"):
        v = np.ascontiguousarray(tracks.T).reshape(-1) * np.float32(32767.0)
        want = np.where(np.isnan(v), 0, np.clip(np.trunc(np.nan_to_num(v, nan=0.0, posinf=1e9, neginf=-1e9)), -32768, 32767)).astype(np.int16)
    assert np.count_nonzero(want[lanes:]) >= 1                           # (0x5A5A is what an unwritten element would hold)
    differ = np.flatnonzero(got != want)
    assert len(differ) == 0, (f"{len(differ)} elements differ, the first at {differ[0]} "
                              f"({'at or above' if differ[0] >= lanes else 'below'} 2^24): {got[differ[:4]]} for {want[differ[:4]]}")


def test_invalid_arguments_leave_the_tracks_unwritten(gpu_ctx, dev):
    L = G.load()
    rng = np.random.default_rng(4)
    rows = rng.uniform(-1, 1, (4, 100)).astype(np.float32)
    d_rows = dev.up(rows)
    init = np.full((2, 300), 7.0, np.float32)
    d_t = dev.up(init)
    arrays = dict(row_len=np.full(4, 100, np.uint32), item_rows=np.array([0, 3], np.uint32),
                  item_tracks=np.array([0, 1], np.uint32), item_offsets=np.array([0, 250], np.uint64))

    def call(rows_dev=d_rows, row_stride=100, n_rows=4, tracks_dev=d_t, track_stride=300, n_tracks=2, track_len=300, **over):
        a = dict(arrays, **over)
        ptr = lambda k: None if a[k] is None else a[k].ctypes.data
        return L.grail_mix_async(gpu_ctx.handle, rows_dev, row_stride, ptr("row_len"), n_rows, ptr("item_rows"),
                                 ptr("item_tracks"), ptr("item_offsets"), None, 2, tracks_dev, track_stride, n_tracks,
                                 track_len, 0)

    assert call() == G.OK
    gpu_ctx.sync()
    want = dev.down(d_t, (2, 300), np.float32)
    assert not np.array_equal(want, init)
    gpu_ctx.h2d(d_t, init, init.nbytes)
    cases = [dict(item_rows=np.array([0, 4], np.uint32)), dict(item_tracks=np.array([0, 2], np.uint32)),
             dict(track_len=301), dict(row_len=np.array([100, 101, 100, 100], np.uint32)), dict(row_stride=99),
             dict(rows_dev=None), dict(row_len=None), dict(item_rows=None), dict(item_offsets=None), dict(tracks_dev=None)]
    for case in cases:
        assert call(**case) == G.ERR_INVALID_ARG, case
        gpu_ctx.sync()
        assert np.array_equal(dev.down(d_t, (2, 300), np.float32), init), case
    # grail_batch_mix: a row past the batch
    gpu_ctx.set_voices(W.single_voice())
    segs, offs, vids, seeds = W.make_batch(4, length=0.01, blend_length=0.01)
    b = gpu_ctx.upload(segs, offs, vids, seeds)
    try:
        with pytest.raises(G.GrailError) as ei:
            b.mix([0, 4], [0, 0], d_t, 300, 2, 300)
        assert ei.value.status == G.ERR_INVALID_ARG
        with pytest.raises(G.GrailError) as ei:
            b.mix([0, 1], [0, 0], d_t, 300, 2, 301)
        assert ei.value.status == G.ERR_INVALID_ARG
        assert np.array_equal(dev.down(d_t, (2, 300), np.float32), init)
    finally:
        b.free()


# ---- config 3: 65 536 rows x 96 006 samples (25.2 GB) ------------------------------------------------------------------
@pytest.fixture(scope="module")
def config3(gpu_ctx):
    gpu_ctx.set_voices(W.single_voice())
    n = 65536
    segs, offs, vids, seeds = W.make_batch(n)
    stride = W.max_samples()
    b = gpu_ctx.upload(segs, offs, vids, seeds)
    d_rows, d_len = gpu_ctx.device_alloc(n * stride * 4), gpu_ctx.device_alloc(n * 4)
    ms = []
    for _ in range(3):
        b.synthesize_async(d_rows, stride, d_len)
        gpu_ctx.sync()
        ms.append(gpu_ctx.last_kernel_ms())
    lens = np.zeros(n, np.uint32)
    gpu_ctx.d2h(lens, d_len, n * 4)
    yield dict(batch=b, d_rows=d_rows, d_len=d_len, stride=stride, lens=lens, n=n, render_ms=min(ms[1:]))
    gpu_ctx.device_free(d_rows)
    gpu_ctx.device_free(d_len)
    b.free()


def _full_case(gpu_ctx, config3, case):
    item_rows, item_tracks, offs, gains, n_tracks, track_len = W.mix_case(case, config3["lens"])
    track_stride = (track_len + 63) // 64 * 64
    d_t = gpu_ctx.device_alloc(n_tracks * track_stride * 4)
    return d_t, (item_rows, item_tracks, offs, gains, n_tracks, track_len, track_stride)


@pytest.mark.parametrize("case", ["concat", "babble"])
def test_full_size_mix(gpu_ctx, dev, config3, case):
    """config-3 rows, cases (a) and (b) of tools/mix_bench.py: on-device digests say every track sample is finite and
    max |x| of a track is at most the sum of |g| over its items (rows stay within +-1); 8 sampled tracks exactly"""
    d_t, (item_rows, item_tracks, offs, gains, n_tracks, track_len, track_stride) = _full_case(gpu_ctx, config3, case)
    dev.ptrs.append(d_t)
    gpu_ctx.mix_async(config3["d_rows"], config3["stride"], config3["lens"], item_rows, offs, d_t, track_stride, n_tracks,
                      track_len, item_tracks=item_tracks, item_gains=gains)
    gpu_ctx.sync()
    d_tl = dev.up(np.full(n_tracks, track_len, np.uint32))
    _, maxabs, bad = gpu_ctx.digest(d_t, track_stride, d_tl, n_tracks)
    g = np.ones(len(item_rows)) if gains is None else np.abs(gains.astype(np.float64))
    sabs = np.bincount(item_tracks, weights=g, minlength=n_tracks)
    assert bad.sum() == 0
    assert np.all(maxabs <= sabs * (1.0 + 2.0 ** -20)), float(np.max(maxabs / sabs))
    stride = config3["stride"]
    for t in sorted(set([0, n_tracks - 1] + [int(x) for x in np.random.default_rng(1).integers(0, n_tracks, 6)])):
        mine = np.nonzero(item_tracks == t)[0]
        used = np.unique(item_rows[mine])
        rows = np.empty((len(used), stride), np.float32)
        for k, r in enumerate(used):
            gpu_ctx.d2h(rows[k], config3["d_rows"], stride * 4, int(r) * stride * 4)
        local = np.searchsorted(used, item_rows[mine]).astype(np.uint32)
        want = fold(rows, config3["lens"][used], local, None, offs[mine], None if gains is None else gains[mine], 1, track_len)
        got = dev.down(d_t, (1, track_len), np.float32, offset=t * track_stride * 4)
        assert same_bits(got, want), t


def test_full_size_stacked_mix(gpu_ctx, dev, config3):
    """config-3 rows, case (c) of tools/mix_bench.py: all 65 536 rows on ONE track at offsets in [0, 1 s) — the short-span
    regime with list tiles of many items.  Every sample finite and within the sum of |g|; two windows of 256 samples checked
    exactly against numpy, one where every item covers it and the last samples of the track"""
    d_t, (item_rows, item_tracks, offs, gains, n_tracks, track_len, track_stride) = _full_case(gpu_ctx, config3, "stacked")
    dev.ptrs.append(d_t)
    gpu_ctx.mix_async(config3["d_rows"], config3["stride"], config3["lens"], item_rows, offs, d_t, track_stride, n_tracks,
                      track_len, item_tracks=item_tracks, item_gains=gains)
    gpu_ctx.sync()
    d_tl = dev.up(np.full(1, track_len, np.uint32))
    _, maxabs, bad = gpu_ctx.digest(d_t, track_stride, d_tl, 1)
    assert bad.sum() == 0 and maxabs[0] <= np.abs(gains.astype(np.float64)).sum() * (1.0 + 2.0 ** -20)
    stride, lens = config3["stride"], config3["lens"]
    W_ = 256
    for s0 in (72000, track_len - W_):
        acc = np.zeros(W_, np.float32)
        piece = np.empty(W_, np.float32)
        covering = 0
        for i in np.argsort(item_rows, kind="stable"):
            o, r = int(offs[i]), int(item_rows[i])
            lo, hi = max(s0, o), min(s0 + W_, o + int(lens[r]), track_len)
            if lo >= hi:
                continue
            covering += 1
            gpu_ctx.d2h(piece, config3["d_rows"], (hi - lo) * 4, (r * stride + lo - o) * 4)
            acc[lo - s0:hi - s0] = acc[lo - s0:hi - s0] + np.float32(gains[i]) * piece[:hi - lo]
        got = dev.down(d_t, W_, np.float32, offset=s0 * 4)
        assert covering > 0 and same_bits(got, acc), (s0, covering)
        if s0 == 72000:
            assert covering == len(item_rows)                  # every item covers the middle of the track


@pytest.mark.perf
def test_mix_costs_a_fraction_of_the_render(gpu_ctx, dev, config3):
    """mix_async of cases (a) and (b) at most 0.5 x the render of those rows; grail_batch_mix of case (b) at most 1.5 x
    rendering the batch alone (wall clock around each call and its sync, best of three after a warm-up)"""
    from conftest import skip_if_clocks_unstable
    render = config3["render_ms"]
    lines, misses = [], []
    for case in ("concat", "babble"):
        d_t, (item_rows, item_tracks, offs, gains, n_tracks, track_len, track_stride) = _full_case(gpu_ctx, config3, case)
        try:
            ms = []
            for rep in range(4):
                t0 = time.perf_counter()
                gpu_ctx.mix_async(config3["d_rows"], config3["stride"], config3["lens"], item_rows, offs, d_t, track_stride,
                                  n_tracks, track_len, item_tracks=item_tracks, item_gains=gains)
                gpu_ctx.sync()
                if rep:
                    ms.append(1e3 * (time.perf_counter() - t0))
        finally:
            gpu_ctx.device_free(d_t)
        lines.append(f"{case}: mix {min(ms):.2f} ms against the render's {render:.2f} ms = {min(ms) / render:.3f} x")
        if min(ms) > 0.5 * render:
            misses.append(lines[-1])
    gpu_ctx.set_voices(W.single_voice())
    b = config3["batch"]
    item_rows, item_tracks, offs, gains, n_tracks, track_len = W.mix_case("babble", config3["lens"])
    track_stride = (track_len + 63) // 64 * 64
    d_t = dev.alloc(n_tracks * track_stride * 4)
    d_rows, d_len = config3["d_rows"], config3["d_len"]
    both, alone = [], []
    for rep in range(3):
        t0 = time.perf_counter()
        b.synthesize_async(d_rows, config3["stride"], d_len)
        gpu_ctx.sync()
        alone.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        b.mix(item_rows, offs, d_t, track_stride, n_tracks, track_len, item_tracks=item_tracks, item_gains=gains)
        both.append(1e3 * (time.perf_counter() - t0))
    lines.append(f"babble: grail_batch_mix {min(both[1:]):.2f} ms against rendering alone {min(alone[1:]):.2f} ms")
    if min(both[1:]) > 1.5 * min(alone[1:]):
        misses.append(lines[-1])
    print("\n" + "\n".join(lines))
    if misses:
        skip_if_clocks_unstable(gpu_ctx, "a mix missed its bar:\n" + "\n".join(misses))
    assert not misses, misses


def test_grail_dialogue_writes_the_stereo_mix(gpu_ctx, dev, tmp_path):
    """examples/grail_dialogue: 2 channels, and its frames equal the same mix made through the Python binding"""
    exe = os.path.join(ROOT, "grail-rs_amd", "lib", "grail_dialogue")
    path = str(tmp_path / "dialogue.wav")
    lines = ["hello there", "a fine day to you"]
    r = subprocess.run([exe, "-o", path] + lines, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    data = open(path, "rb").read()
    _, _, ch, rate, _, align, bits = struct.unpack("<IHHIIHH", data[16:36])
    assert (ch, rate, align, bits) == (2, 44100, 4, 16)
    frames = np.frombuffer(data[44:], "<i2").reshape(-1, 2)
    v0 = G.voice_generic()
    v1 = v0.copy()
    v1.center_frequency = float(np.float32(v0.center_frequency) * np.float32(1.5))
    gpu_ctx.set_voices([v0, v1])
    s0, s1 = G.text_to_phoneme_elems(v0, lines[0]), G.text_to_phoneme_elems(v1, lines[1])
    b = gpu_ctx.upload(np.concatenate([s0, s1]), [0, len(s0), len(s0) + len(s1)], [0, 1], [0, 0])
    try:
        lens = b.lengths()
        at, end = G.mix_place_sequential(lens, [0, 1], None, [0, int(np.float32(44100.0) * np.float32(3.0) / np.float32(10.0))], 1)
        n = int(end[0])
        stride = (n + 63) // 64 * 64
        d_t = dev.alloc(2 * stride * 4)
        b.mix([0, 0, 1, 1], [at[0], at[0], at[1], at[1]], d_t, stride, 2, n, item_tracks=[0, 1, 0, 1],
              item_gains=[0.8, 0.2, 0.2, 0.8])
        tracks = dev.down(d_t, (2, stride), np.float32)[:, :n]
        d_in, d_f = dev.up(np.ascontiguousarray(tracks)), dev.alloc(n * 4)
        gpu_ctx.pcm16_frames_async(d_in, n, 2, n, d_f)
        gpu_ctx.sync()
        want = dev.down(d_f, (n, 2), np.int16)
    finally:
        b.free()
    assert np.array_equal(frames, want)
    assert np.abs(frames[:, 0].astype(np.int64)).sum() > 0 and np.abs(frames[:, 1].astype(np.int64)).sum() > 0
