"""Set-up, regrowth and tear-down of everything a context holds (its stream, events and voice tables, the host-output pipe
with its two device blocks and pinned ring, the mix and level scratch) and of what streams and batches hold: one process
creates a context, drives every holder and destroys it, three times over.  No new kernel shapes; the rows are the
oracle's bits and every round reproduces the first bit for bit."""
import numpy as np
import pytest

import grail_hip as G
import oracle_lib as O
from grail_hip import workload as W
from footprint import ovoices, pcm16_of
from test_levels_gpu import Dev, fold, same_bits

pytestmark = pytest.mark.gpu
N = 8193                    # the host forms render blocks of 4 096 rows: 4 096 / 4 096 / 1, both device slots reused
STRIDE = 256
PROBES = [0, 4095, 4096, 8192]
N_DEV = 64                  # rows of the device-destination call
RATE = 48000


def _rows(first, count):
    """`count` utterances from `first` on: one voiced segment of 192 samples and a few, pitch and seed by the row"""
    u = np.arange(first, first + count)
    segs = G.segments([(G.PH_A if k % 2 else G.PH_E, 0.004, 2.0 ** -8, (100.0 + k % 97) / RATE) for k in u.tolist()])
    return segs, np.arange(count + 1, dtype=np.uint32), np.zeros(count, np.uint32), (u * 7919 + 3).astype(np.uint32)


@pytest.fixture(scope="module")
def corpus():
    """the batch, and the oracle's rendering of the probed rows and of the first N_DEV: computed once, never changed"""
    voice = W.single_voice()
    segs, offs, vids, seeds = _rows(0, N)
    ref, ref_len = {}, {}
    for r in PROBES:
        out, n = O.synthesize_phonemes(ovoices(voice)[0], segs[r:r + 1], int(seeds[r]))
        assert 192 <= n < STRIDE
        ref[r] = np.zeros(STRIDE, np.float32)
        ref[r][:n] = out[:n]
        ref_len[r] = n
        ref[r].setflags(write=False)
    head, head_len = O.synthesize_batch(ovoices(voice), segs[:N_DEV], offs[:N_DEV + 1], vids[:N_DEV], seeds[:N_DEV], STRIDE)
    head.setflags(write=False)
    return dict(voice=voice, batch=(segs, offs, vids, seeds), ref=ref, ref_len=ref_len, head=head, head_len=head_len)


def _round(corpus):
    """one context from grail_create to grail_destroy -> everything it computed"""
    segs, offs, vids, seeds = corpus["batch"]
    got = {}
    with G.Context(0) as ctx:
        dev = Dev(ctx)
        try:
            # a table of two voices that a kernel has read, replaced by a table of one
            two = W.preset_voices(2)
            ctx.set_voices(two)
            s2, o2, _, q2 = _rows(0, 4)
            got["two_voices"] = ctx.synthesize(s2, o2, np.array([0, 1, 1, 0], np.uint32), q2, out_stride=STRIDE)[0]
            ctx.set_voices(corpus["voice"])
            # the one-call f32 form into pageable memory (staging ring, copier threads) and into pinned memory (direct)
            lens = np.zeros(N, np.uint32)
            pageable = np.full((N, STRIDE), 7.0, np.float32)
            ctx.synthesize_into(pageable, lens, segs, offs, vids, seeds)
            got["f32"], got["len"] = pageable, lens.copy()
            pinned = ctx.host_alloc((N, STRIDE), np.float32)
            try:
                pinned[:] = 7.0
                ctx.synthesize_into(pinned, lens, segs, offs, vids, seeds)
                got["f32_pinned"], got["len_pinned"] = pinned.copy(), lens.copy()
            finally:
                ctx.host_free(pinned)
            # the same batch as i16
            got["i16"], got["len_i16"] = ctx.synthesize_pcm16(segs, offs, vids, seeds, out_stride=STRIDE)
            # N_DEV of the rows to a device destination: the one-call form that is one launch, not blocks
            d_out = dev.alloc(N_DEV * STRIDE * 4)
            ctx.memset(d_out, 0, N_DEV * STRIDE * 4)
            dev_len = np.zeros(N_DEV, np.uint32)
            G._check(G.load().grail_synthesize_batch(ctx.handle, segs.ctypes.data, offs.ctypes.data, vids.ctypes.data,
                                                     seeds.ctypes.data, N_DEV, d_out, STRIDE, dev_len.ctypes.data, G.OUT_DEVICE))
            got["f32_device"], got["len_device"] = dev.down(d_out, (N_DEV, STRIDE), np.float32), dev_len
            # a mix of 8 rows on two tracks
            item_rows, item_tracks = np.arange(8, dtype=np.uint32), (np.arange(8) % 2).astype(np.uint32)
            item_offs, track_len = (np.arange(8) * 100).astype(np.uint64), 1024
            d_tracks = dev.alloc(2 * track_len * 4)
            b = ctx.upload(segs[:8], offs[:9], vids[:8], seeds[:8])
            try:
                got["mix_len"] = b.mix(item_rows, item_offs, d_tracks, track_len, 2, track_len, item_tracks=item_tracks)
                got["mix"] = dev.down(d_tracks, (2, track_len), np.float32)
                # one of each measurement and a limiter call on 3 rows
                d_rows, d_len = dev.alloc(3 * STRIDE * 4), dev.alloc(3 * 4)
                b3 = ctx.upload(segs[:3], offs[:4], vids[:3], seeds[:3])
                try:
                    b3.synthesize_async(d_rows, STRIDE, d_len)
                    got["levels"] = ctx.levels(d_rows, STRIDE, d_len, 3)
                    gated, _, bad = ctx.loudness(d_rows, STRIDE, d_len, 3, RATE, hops=False)
                    got["loudness"] = (gated, bad)
                    got["true_peak"] = ctx.true_peak(d_rows, STRIDE, d_len, 3)
                    d_lim = dev.alloc(3 * STRIDE * 4)
                    ctx.memset(d_lim, 0, 3 * STRIDE * 4)
                    got["limit"] = ctx.limit(d_rows, STRIDE, d_len, 3, 0.05, 5, d_lim, STRIDE, 1)
                    got["limited"] = dev.down(d_lim, (3, STRIDE), np.float32)
                    # a resumable stream, pulled once
                    d_chunk, d_chunk_len = dev.alloc(3 * 64 * 4), dev.alloc(3 * 4)
                    st = G.Stream(b3)
                    try:
                        st.next_async(64, d_chunk, 64, d_chunk_len)
                        ctx.sync()
                        got["stream"] = dev.down(d_chunk, (3, 64), np.float32)
                        got["stream_len"] = dev.down(d_chunk_len, 3, np.uint32)
                    finally:
                        st.close()
                finally:
                    b3.free()
            finally:
                b.free()
            # a live stream: two appends (both pinned staging buffers), one pull, closed with samples left
            live = G.LiveStream(ctx, 2, None, seeds[:2], ring_segments=8)
            try:
                live.append(segs[:2], [0, 1, 2])
                live.append(segs[2:4], [0, 1, 2])
                live.finish()
                d_live, d_live_len = dev.alloc(2 * 512 * 4), dev.alloc(2 * 4)
                live.next_async(300, d_live, 512, d_live_len)
                ctx.sync()
                got["live_len"] = dev.down(d_live_len, 2, np.uint32)
                got["live"] = dev.down(d_live, (2, 512), np.float32)[:, :300]
            finally:
                live.close()
        finally:
            dev.free()
    return got


def _flat(got):
    out = {}
    for k, v in got.items():
        for i, a in enumerate(v if isinstance(v, tuple) else (v,)):
            out[f"{k}[{i}]"] = np.ascontiguousarray(a)
    return out


def test_three_contexts_in_one_process_set_up_regrow_and_tear_down(built, corpus):
    if G.device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests must run on the GPU box")
    first = _round(corpus)
    # the host destinations: the oracle's bits on the rows at both ends of every block, zero tails included
    for r in PROBES:
        for key in ("f32", "f32_pinned"):
            assert same_bits(first[key][r], corpus["ref"][r]), (key, r)
        assert first["len"][r] == corpus["ref_len"][r], r
    assert same_bits(first["f32"], first["f32_pinned"]) and np.array_equal(first["len"], first["len_pinned"])
    assert same_bits(first["f32"][:N_DEV], corpus["head"]) and np.array_equal(first["len"][:N_DEV], corpus["head_len"])
    assert np.all((first["len"] >= 192) & (first["len"] < STRIDE))
    # i16: the conversion of the f32 rows
    assert np.array_equal(first["len_i16"], first["len"])
    assert np.array_equal(first["i16"], pcm16_of(first["f32"]))
    # the device destination
    assert same_bits(first["f32_device"], corpus["head"]) and np.array_equal(first["len_device"], corpus["head_len"])
    # the mix: the contract's fold of the rows
    assert np.array_equal(first["mix_len"], first["len"][:8])
    assert same_bits(first["mix"], fold(first["f32"], first["len"], np.arange(8), np.arange(8) % 2, np.arange(8) * 100,
                                        np.ones(8, np.float32), 2, 1024))
    # what was streamed and measured was these rows
    assert np.array_equal(first["stream_len"], [64, 64, 64]) and same_bits(first["stream"], first["f32"][:3, :64])
    assert same_bits(first["levels"][1], np.abs(first["f32"][:3]).max(axis=1)) and not first["levels"][2].any()
    assert np.array_equal(first["live_len"], [300, 300]) and np.count_nonzero(first["live"]) > 300
    # rounds two and three: a context made after another was destroyed computes the same bits
    want = _flat(first)
    for again in (2, 3):
        got = _flat(_round(corpus))
        assert got.keys() == want.keys()
        for k in want:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (again, k)
            assert got[k].tobytes() == want[k].tobytes(), (again, k)
