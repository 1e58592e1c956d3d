"""The flush of a tile inside a run of calm tiles (synth_kernel_tile_loop.h, flush_full_tile): a wave whose 64 rows all take
whole tiles as 16-byte stores addresses its rows once — the lane's row pointer, then one step per group of eight rows —
instead of once per row group and tile.  The same bytes have to land at the same addresses: every case renders on one lane
per utterance into a canary-filled buffer and is held to the oracle bit for bit (fast arithmetic: within its tolerance), the
words between a row's count and the stride untouched.  Waves with idle lanes, rows that are not 16-byte aligned and rows
placed by the length-sorted slot order keep the flushes they had and are checked beside the new path; strides on both sides
of 2^26 samples (where the step from one row group to the next reaches 2^31 bytes and a lane's offset from the wave's first row
no longer fits 32 bits: nothing in the addressing may be narrower than 64) go into a buffer of 17 GB of which only the rows'
own samples and 64 words behind them are filled and read."""
import ctypes as C

import numpy as np
import pytest

import grail_hip as G
import oracle_lib as O
from grail_hip import workload as W

pytestmark = pytest.mark.gpu

CANARY = 0x7FC0DEAD            # a quiet NaN no arithmetic of the kernels produces
SPARE_ROWS = 2                 # rows behind the batch's own: no launch may touch them
SEGMENTS, LENGTH, BLEND = 2, 0.1, 2.0 ** -5     # 9 600 samples a row: several runs of calm tiles
N_MAX = 130
_cache = {}


def ovoices(voices):
    return [O.Voice.from_buffer_copy(bytes(v)) for v in voices]


def equal_rows():
    """The 130 utterances of the corpus (64 and 65 are its first rows) and the oracle's rows, computed once."""
    if "equal" not in _cache:
        voices = W.single_voice()
        batch = W.make_batch(N_MAX, segments=SEGMENTS, length=LENGTH, blend_length=BLEND)
        ref, ref_len = O.synthesize_batch(ovoices(voices), *batch, W.max_samples(segments=SEGMENTS, length=LENGTH))
        ref.setflags(write=False)
        ref_len.setflags(write=False)
        _cache["equal"] = (voices, batch, ref, ref_len)
    return _cache["equal"]


def first_rows(n):
    voices, (segs, offs, vids, seeds), ref, ref_len = equal_rows()
    return voices, (segs[:offs[n]], offs[:n + 1], vids[:n], seeds[:n]), ref[:n], ref_len[:n]


def render(ctx, batch, n_utt, stride, base_offset=0):
    """The batch into a canary-filled buffer of n_utt + SPARE_ROWS rows that starts base_offset bytes into its allocation.
    Returns (rows as uint32 [n_utt + SPARE_ROWS, stride], lengths, the kernel's name)."""
    rows = n_utt + SPARE_ROWS
    d_out, d_len = ctx.device_alloc(rows * stride * 4 + base_offset), ctx.device_alloc(n_utt * 4)
    try:
        out = C.c_void_p(d_out.value + base_offset)
        fill = np.full(rows * stride, CANARY, dtype=np.uint32)
        ctx.h2d(out, fill, fill.nbytes)
        batch.synthesize_async(out, stride, d_len)
        ctx.sync()
        name = ctx.last_kernel_name()
        got = np.zeros((rows, stride), dtype=np.uint32)
        lens = np.zeros(n_utt, dtype=np.uint32)
        ctx.d2h(got, out, got.nbytes)
        ctx.d2h(lens, d_len, lens.nbytes)
    finally:
        ctx.device_free(d_out)
        ctx.device_free(d_len)
    return got, lens, name


def render_sparse(ctx, batch, ref_len, stride, behind=64):
    """The same for strides too long to fill: only each row's own samples and `behind` words after them are set to the
    canary and read back.  Returns (list of uint32 rows of ref_len[u] + behind words, lengths, the kernel's name)."""
    n_utt = len(ref_len)
    d_out, d_len = ctx.device_alloc(n_utt * stride * 4), ctx.device_alloc(n_utt * 4)
    try:
        for u in range(n_utt):
            fill = np.full(int(ref_len[u]) + behind, CANARY, dtype=np.uint32)
            ctx.h2d(C.c_void_p(d_out.value + u * stride * 4), fill, fill.nbytes)
        batch.synthesize_async(d_out, stride, d_len)
        ctx.sync()
        name = ctx.last_kernel_name()
        got = []
        for u in range(n_utt):
            row = np.zeros(int(ref_len[u]) + behind, dtype=np.uint32)
            ctx.d2h(row, d_out, row.nbytes, offset=u * stride * 4)
            got.append(row)
        lens = np.zeros(n_utt, dtype=np.uint32)
        ctx.d2h(lens, d_len, lens.nbytes)
    finally:
        ctx.device_free(d_out)
        ctx.device_free(d_len)
    return got, lens, name


def assert_rows_and_canary(got, lens, ref, ref_len, what):
    """got: rows of uint32 (a 2-d array, the rows behind the batch's own included, or a list of the rows' heads)."""
    n_utt = len(ref_len)
    assert np.array_equal(lens, ref_len), f"{what}: lengths differ {lens[:8]} vs {ref_len[:8]}"
    for u in range(n_utt):
        n = int(ref_len[u])
        want = ref[u, :n].view(np.uint32)
        if not np.array_equal(got[u][:n], want):
            i = int(np.argmax(got[u][:n] != want))
            raise AssertionError(f"{what}: utterance {u} first differs at sample {i} of {n} "
                                 f"({int((got[u][:n] != want).sum())} differ)")
        past = got[u][n:]
        if not np.all(past == CANARY):
            i = n + int(np.argmax(past != CANARY))
            raise AssertionError(f"{what}: row {u} of {n} samples was written at {i} ({int((past != CANARY).sum())} words past its count)")
    if isinstance(got, np.ndarray):
        assert np.all(got[n_utt:] == CANARY), f"{what}: a row the batch does not own was written"


def assert_exact_one_lane_kernel(name):
    assert name.startswith("synth_kernel<L=1,T=32,W=1,1,") and "NFA=4" in name and "FAST" not in name, name


def check_equal_rows(ctx, n_utt, strides, what, base_offset=0):
    voices, (segs, offs, vids, seeds), ref, ref_len = first_rows(n_utt)
    ctx.set_voices(voices)
    ctx.set_option("lanes_per_utterance", 1)
    batch = ctx.upload(segs, offs, vids, seeds)
    try:
        for stride in strides:
            got, lens, name = render(ctx, batch, n_utt, stride, base_offset)
            assert_exact_one_lane_kernel(name)
            assert_rows_and_canary(got, lens, ref, ref_len, f"{what}, stride {stride} ({name})")
    finally:
        batch.free()
        ctx.set_option("lanes_per_utterance", 0)


def aligned_stride():
    return (int(equal_rows()[3].max()) + 3) // 4 * 4


@pytest.mark.parametrize("n_utt", [64, 65, 130])
def test_whole_and_partial_waves(gpu_ctx, n_utt):
    """64 rows are one full wave: every tile inside a run takes the full-tile flush.  65 and 130 rows leave a wave with
    idle lanes, whose runs go through flush_rows."""
    check_equal_rows(gpu_ctx, n_utt, (aligned_stride(),), f"{n_utt} equal rows")


def test_unaligned_strides_and_an_offset_base(gpu_ctx):
    """The full wave again with a stride that is the rows' length rounded up to four samples, that + 1 and + 2 (rows that
    do not start 16-byte aligned keep a head per tile and their own flush), and into a buffer that starts 4 bytes into its
    allocation (aligned stride, unaligned rows)."""
    s = aligned_stride()
    check_equal_rows(gpu_ctx, 64, (s, s + 1, s + 2), "64 equal rows")
    check_equal_rows(gpu_ctx, 64, (s,), "64 equal rows, base + 4 bytes", base_offset=4)


@pytest.mark.parametrize("sort", [0, 1])
def test_rows_of_different_lengths_under_the_sorted_slot_order(gpu_ctx, sort):
    """128 rows of 0.02 - 0.35 s in the caller's order and in the length-sorted slot assignment, where a lane's row is not
    its slot (the rows are looked up, the new addressing does not apply): two full waves whose lanes end one after another."""
    rng = np.random.default_rng(12)
    n_utt = 128
    voices = W.single_voice()
    segs, offs, vids, seeds = W.make_batch(n_utt, segments=SEGMENTS, length=LENGTH, blend_length=BLEND)
    segs["length"] = rng.uniform(0.01, 0.175, len(segs)).astype(np.float32)
    stride = (int(SEGMENTS * 0.175 * 48000) + 8 + 3) // 4 * 4
    ref, ref_len = O.synthesize_batch(ovoices(voices), segs, offs, vids, seeds, stride)
    gpu_ctx.set_voices(voices)
    gpu_ctx.set_option("lanes_per_utterance", 1)
    gpu_ctx.set_option("sort_by_length", sort)
    batch = gpu_ctx.upload(segs, offs, vids, seeds)
    try:
        got, lens, name = render(gpu_ctx, batch, n_utt, stride)
        assert_exact_one_lane_kernel(name)
        assert_rows_and_canary(got, lens, ref, ref_len, f"ragged rows, sort_by_length={sort} ({name})")
    finally:
        batch.free()
        gpu_ctx.set_option("sort_by_length", 1)
        gpu_ctx.set_option("lanes_per_utterance", 0)


@pytest.mark.parametrize("stride", [2 ** 26 - 64, 2 ** 26])
def test_strides_on_both_sides_of_the_32_bit_offset(gpu_ctx, stride):
    """64 rows 2^26 - 64 and 2^26 samples apart (a buffer of 17 GB): the last row group of the wave starts 56 rows, some
    15 GB, behind the first.  Only each row's samples and 64 words behind them are filled and checked."""
    voices, (segs, offs, vids, seeds), ref, ref_len = first_rows(64)
    gpu_ctx.set_voices(voices)
    gpu_ctx.set_option("lanes_per_utterance", 1)
    batch = gpu_ctx.upload(segs, offs, vids, seeds)
    try:
        got, lens, name = render_sparse(gpu_ctx, batch, ref_len, stride)
        assert_exact_one_lane_kernel(name)
        assert_rows_and_canary(got, lens, ref, ref_len, f"64 equal rows, stride {stride} ({name})")
    finally:
        batch.free()
        gpu_ctx.set_option("lanes_per_utterance", 0)


def test_the_full_wave_in_fast_arithmetic(gpu_ctx):
    """The first case in tolerance arithmetic: within GRAIL_FAST_TOLERANCE of the oracle, lengths the oracle's, canary intact."""
    voices, (segs, offs, vids, seeds), ref, ref_len = first_rows(64)
    stride = aligned_stride()
    gpu_ctx.set_voices(voices)
    gpu_ctx.set_option("lanes_per_utterance", 1)
    gpu_ctx.set_option("arithmetic", 1)
    batch = gpu_ctx.upload(segs, offs, vids, seeds)
    try:
        got, lens, name = render(gpu_ctx, batch, 64, stride)
    finally:
        batch.free()
        gpu_ctx.set_option("arithmetic", 0)
        gpu_ctx.set_option("lanes_per_utterance", 0)
    assert np.array_equal(lens, ref_len), name
    for u in range(64):
        n = int(ref_len[u])
        worst = float(np.max(np.abs(got[u, :n].view(np.float32).astype(np.float64) - ref[u, :n].astype(np.float64))))
        assert worst <= G.FAST_TOLERANCE, (name, u, worst)
        assert np.all(got[u, n:] == CANARY), (name, u)
    assert np.all(got[64:] == CANARY), name
