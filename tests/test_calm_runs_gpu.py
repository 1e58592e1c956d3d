"""Runs of calm tiles in the one-lane exact kernels (synth_kernel_tile_loop.h, CALM_RUNS): one tile head for up to
CALM_RUN_MAX_TILES = 64 calm tiles, the tiles inside a run flushed by the run itself.  A run may not move a bit, store for a
lane that does not render, or store past a row's count.  Everything here runs with "lanes_per_utterance" pinned to 1 and is
judged against the oracle; the rows are rendered into device buffers filled with a canary pattern beforehand.
Only the four-formant one-shot kernel for power-of-two blend lengths, writing 16-byte-aligned f32 rows, takes runs; the cases
with other blend lengths (the ANYBL kernel, which the name check accepts too), eight formants, streams, i16 rows and
unaligned strides exercise kernels and paths that are gated out and must be what they were."""
import numpy as np
import pytest

import grail_hip as G
import oracle_lib as O
from grail_hip import workload as W

pytestmark = pytest.mark.gpu

CANARY = 0x7FC0DEAD            # a quiet NaN no arithmetic of the kernels produces
CANARY16 = 0x5A5A
SPARE_ROWS = 3                 # rows behind the batch's own: no launch may touch them
TILE = 32
RUN = 64 * TILE                # samples of the longest run


def ovoices(voices):
    return [O.Voice.from_buffer_copy(bytes(v)) for v in voices]


def pcm16_of(x):
    v = x.astype(np.float32) * np.float32(32767.0)
    return np.where(np.isnan(v), 0, np.clip(np.trunc(np.nan_to_num(v, nan=0.0, posinf=1e9, neginf=-1e9)), -32768, 32767)).astype(np.int16)


def render_into_canary(ctx, batch, n_utt, stride, pcm16=False, truncating=False):
    """The batch rendered on one lane per utterance into a canary-filled buffer of n_utt + SPARE_ROWS rows.
    Returns (rows as uint32 or int16 [n_utt + SPARE_ROWS, stride], lengths, the kernel's name)."""
    rows = n_utt + SPARE_ROWS
    item = 2 if pcm16 else 4
    d_out, d_len = ctx.device_alloc(rows * stride * item), ctx.device_alloc(n_utt * 4)
    try:
        fill = np.full(rows * stride, CANARY16 if pcm16 else CANARY, dtype=np.uint16 if pcm16 else np.uint32)
        ctx.h2d(d_out, fill, fill.nbytes)
        (batch.synthesize_pcm16_async if pcm16 else batch.synthesize_async)(d_out, stride, d_len)
        try:
            ctx.sync()
        except G.GrailError as e:
            assert truncating and e.status == G.ERR_BUFFER_TOO_SMALL
        name = ctx.last_kernel_name()
        got = np.zeros((rows, stride), dtype=np.uint16 if pcm16 else np.uint32)
        lens = np.zeros(n_utt, dtype=np.uint32)
        ctx.d2h(got, d_out, got.nbytes)
        ctx.d2h(lens, d_len, lens.nbytes)
    finally:
        ctx.device_free(d_out)
        ctx.device_free(d_len)
    return got, lens, name


def assert_rows_and_canary(got, lens, ref, ref_len, what, pcm16=False):
    n_utt = len(ref_len)
    assert np.array_equal(lens, ref_len), f"{what}: lengths differ {lens[:8]} vs {ref_len[:8]}"
    canary = CANARY16 if pcm16 else CANARY
    for u in range(n_utt):
        n = int(ref_len[u])
        want = pcm16_of(ref[u, :n]).view(np.uint16) if pcm16 else ref[u, :n].view(np.uint32)
        if not np.array_equal(got[u, :n], want):
            i = int(np.argmax(got[u, :n] != want))
            raise AssertionError(f"{what}: utterance {u} first differs at sample {i} of {n} "
                                 f"({int((got[u, :n] != want).sum())} differ)")
        past = got[u, n:]
        if not np.all(past == canary):
            i = n + int(np.argmax(past != canary))
            raise AssertionError(f"{what}: row {u} of {n} samples was written at {i} ({int((past != canary).sum())} words past its count)")
    assert np.all(got[n_utt:] == canary), f"{what}: a row the batch does not own was written"


def one_lane(ctx):
    ctx.set_option("lanes_per_utterance", 1)


def check_batch(ctx, voices, segs, offs, vids, seeds, strides, what, formants=4, pcm16_strides=(), truncating=False):
    """One batch on one lane per utterance, f32 rows for every stride of `strides` and i16 rows for `pcm16_strides`,
    against the oracle and the canary."""
    n_utt = len(offs) - 1
    ctx.set_voices(voices)
    batch = ctx.upload(segs, offs, vids, seeds)
    try:
        for pcm16, stride in [(False, s) for s in strides] + [(True, s) for s in pcm16_strides]:
            ref, ref_len = O.synthesize_batch(ovoices(voices), segs, offs, vids, seeds, stride)
            ref_len = np.minimum(ref_len, stride)
            got, lens, name = render_into_canary(ctx, batch, n_utt, stride, pcm16, truncating)
            assert name.startswith("synth_kernel<L=1,T=32,W=1,1,") and f"NFA={formants}" in name and "FAST" not in name, name
            assert_rows_and_canary(got, lens, ref, ref_len, f"{what}, {'i16' if pcm16 else 'f32'} rows of stride {stride} ({name})", pcm16)
    finally:
        batch.free()


def quiet_voice(jitter_every):
    v = G.voice_generic(48000.0)
    v.jitter_frequency = float(np.float32(1.0) / np.float32(jitter_every))
    return v


@pytest.mark.parametrize("sort", [0, 1])
def test_rows_of_different_lengths_share_a_wave(gpu_ctx, sort):
    """Utterances of 0.02 - 0.5 s side by side (in the caller's order, and in the length-sorted slot assignment, where a
    lane's row is not its slot): lanes idle through whole runs, lanes finishing while the others go on, a last wave with
    empty slots; aligned rows, rows whose stride is not a multiple of four samples, i16 rows."""
    rng = np.random.default_rng(5)
    n_utt = 200
    voices = [quiet_voice(100000.0)]
    segs, offs, vids, seeds = W.make_batch(n_utt, length=0.02, blend_length=2.0 ** -6)
    segs["length"] = rng.uniform(0.005, 0.125, len(segs)).astype(np.float32)
    segs["length"][offs[17]:offs[18]] = np.float32(0.0004)        # a row that ends inside the first tile
    stride = (int(4 * 0.125 * 48000) + 8 + 3) // 4 * 4
    one_lane(gpu_ctx)
    gpu_ctx.set_option("sort_by_length", sort)
    try:
        check_batch(gpu_ctx, voices, segs, offs, vids, seeds, (stride, stride + 2, stride + 1), f"ragged rows, sort_by_length={sort}",
                    pcm16_strides=(stride, stride + 1))
    finally:
        gpu_ctx.set_option("sort_by_length", 1)
        gpu_ctx.set_option("lanes_per_utterance", 0)


def test_whole_waves_of_equal_rows_and_a_truncating_stride(gpu_ctx):
    """The bench corpus in small: every lane of a wave renders from the first tile to the last (every tile of a run takes
    the full-tile flush), a last wave with empty slots, blend lengths that are (runs) and are not (the ANYBL kernel, no
    runs) powers of two, and a stride that cuts every row inside a run."""
    n_utt = 150
    voices = W.single_voice()
    one_lane(gpu_ctx)
    try:
        for blend in (2.0 ** -5, 0.03):
            segs, offs, vids, seeds = W.make_batch(n_utt, length=0.06, blend_length=blend)
            full = (W.max_samples(length=0.06) + 3) // 4 * 4
            check_batch(gpu_ctx, voices, segs, offs, vids, seeds, (full, full + 3), f"equal rows, blend {blend}", pcm16_strides=(full,))
            check_batch(gpu_ctx, voices, segs, offs, vids, seeds, (5000, 4999, 4112), f"truncated rows, blend {blend}", truncating=True)
    finally:
        gpu_ctx.set_option("lanes_per_utterance", 0)


@pytest.mark.parametrize("n_utt", [3, 64, 130])
def test_events_around_tile_and_run_boundaries(gpu_ctx, n_utt):
    """Segment ends and jitter wraps on every offset around the end of a run of the maximum length (64 tiles, 2 048
    samples), and around tile edges inside shorter runs: a wrap every 2 040 ... 2 120 steps puts the event into the tile right
    after the longest run, into the one after that, or ends the run early; segments of 2 030.5 ... 2 160.5 samples do the same
    with the clock.  Three utterances (the other lanes idle: the staged tile), one full wave whose lanes have their events
    together, and waves whose lanes have them at different samples."""
    rate = np.float32(48000.0)
    one_lane(gpu_ctx)
    try:
        for every in (2040.0, 2049.0, 2063.0, 2070.0, 2079.0, 2080.0, 2081.0, 2095.0, 2112.0, 2120.0, 1.0e6):
            voices = [quiet_voice(every)]
            segs, offs, vids, seeds = [], [0], [], []
            for u in range(n_utt):
                k = (2030 + u) if n_utt > 64 else (2030 + 5 * int(every) % 131)     # one wave: the same events in every lane
                length = float((np.float32(k) + np.float32(0.5)) / rate)
                for i in range(3):
                    ph = (G.PH_A, G.PH_E, G.PH_SILENCE)[(k + i) % 3]
                    segs.append((ph, length, 2.0 ** -8, float(np.float32(90 + k % 100) / rate)))
                offs.append(len(segs))
                vids.append(0)
                seeds.append(u * 7919 + 1)
            segs = G.segments(segs)
            offs, vids, seeds = (np.array(a, dtype=np.uint32) for a in (offs, vids, seeds))
            check_batch(gpu_ctx, voices, segs, offs, vids, seeds, (6600,), f"jitter wrap every {every} steps, {n_utt} utterances")
        # rows that fill up inside a run, at every offset of a tile
        voices = [quiet_voice(1.0e6)]
        segs, offs, vids, seeds = W.make_batch(n_utt, length=0.1, blend_length=2.0 ** -4)
        check_batch(gpu_ctx, voices, segs, offs, vids, seeds, tuple(range(RUN + 4 * TILE, RUN + 5 * TILE + 1, 4)) + (RUN + 4 * TILE + 1,),
                    f"rows full inside a run, {n_utt} utterances", truncating=True)
    finally:
        gpu_ctx.set_option("lanes_per_utterance", 0)


def test_eight_formant_voices_on_one_lane(gpu_ctx):
    """Voices with eight live formants keep the kernels they had (every tile decides for itself): same rows, same canary."""
    voices = W.preset_voices(8)
    n_utt = 100
    segs, offs, vids, seeds = W.make_batch(n_utt, n_voices=8, length=0.05, blend_length=2.0 ** -5)
    full = (W.max_samples(length=0.05) + 3) // 4 * 4
    one_lane(gpu_ctx)
    try:
        check_batch(gpu_ctx, voices, segs, offs, vids, seeds, (full, full + 1), "eight formants", formants=8, pcm16_strides=(full,))
    finally:
        gpu_ctx.set_option("lanes_per_utterance", 0)


@pytest.mark.parametrize("n_voices", [1, 8])
def test_a_resumable_stream_on_one_lane(gpu_ctx, n_voices):
    """Chunks pulled through a stream (quotas that end inside runs, on tile edges and one sample at a time) concatenate to the
    oracle's rows; no chunk writes past its quota's count."""
    voices = [quiet_voice(100000.0)] if n_voices == 1 else W.preset_voices(8)
    n_utt = 70
    segs, offs, vids, seeds = W.make_batch(n_utt, n_voices=n_voices, length=0.06, blend_length=2.0 ** -5)
    segs["length"][offs[5]:offs[6]] = np.float32(0.011)
    stride = 4096
    ref, ref_len = O.synthesize_batch(ovoices(voices), segs, offs, vids, seeds, 4 * 2880 + 64)
    gpu_ctx.set_voices(voices)
    one_lane(gpu_ctx)
    batch = gpu_ctx.upload(segs, offs, vids, seeds)
    st = G.Stream(batch)
    d_out, d_len = gpu_ctx.device_alloc((n_utt + SPARE_ROWS) * stride * 4), gpu_ctx.device_alloc(n_utt * 4)
    rows = [[] for _ in range(n_utt)]
    try:
        fill = np.full((n_utt + SPARE_ROWS) * stride, CANARY, dtype=np.uint32)
        for k in range(10000):
            q = (RUN + 4 * TILE, 37, 4096, 64, 1, 2049)[k % 6]
            gpu_ctx.h2d(d_out, fill, fill.nbytes)
            st.next_async(q, d_out, stride, d_len)
            gpu_ctx.sync()
            assert gpu_ctx.last_kernel_name().startswith("synth_kernel<L=1,T=32,W=1,1,STREAM,"), gpu_ctx.last_kernel_name()
            lens = np.zeros(n_utt, dtype=np.uint32)
            gpu_ctx.d2h(lens, d_len, lens.nbytes)
            assert lens.max() <= q
            if lens.max() == 0:
                break
            buf = np.zeros((n_utt + SPARE_ROWS, stride), dtype=np.uint32)
            gpu_ctx.d2h(buf, d_out, buf.nbytes)
            for u in range(n_utt):
                rows[u].append(buf[u, :lens[u]].copy())
                assert np.all(buf[u, lens[u]:] == CANARY), (k, u)
            assert np.all(buf[n_utt:] == CANARY), k
    finally:
        st.close()
        batch.free()
        gpu_ctx.device_free(d_out)
        gpu_ctx.device_free(d_len)
        gpu_ctx.set_option("lanes_per_utterance", 0)
    for u in range(n_utt):
        got = np.concatenate(rows[u])
        assert len(got) == ref_len[u], (u, len(got), ref_len[u])
        assert np.array_equal(got, ref[u, :ref_len[u]].view(np.uint32)), u
