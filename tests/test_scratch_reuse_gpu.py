"""The device scratch that a context and a live stream keep from call to call (DeviceBuffer::reserve: grown when too small,
never shrunk): one context called small, then large, then small again.  The large call after the small one frees a
buffer under a stream that has used it; the small call after the large one reads a scratch whose cells beyond its own
hold the large call's numbers.  Every result is what the numpy models and the oracle give, bit for bit, and the third
call's equals the first's."""
import numpy as np
import pytest

import grail_hip as G
import oracle_lib as O
from grail_hip import workload as W
from test_levels_gpu import Dev, _awkward, _oracle, _place, fold, same_bits
from test_levels_host import gains_model, row_model
from test_limiter_host import limiter_model
from test_loudness_host import gate_model, kweight_hops_model
from test_loudness_segmented_host import segmented_hops_model
from test_true_peak_host import true_peak_model

pytestmark = pytest.mark.gpu
RATE = 8000
HOP = RATE // 10
SHAPES = {"A": (4096, [0, 1, 4096]), "B": (20000, [20000, 12289, 4097, 800, 0])}      # stride, lengths: 5 and 25 hops a row
ORDER = ["A", "B", "A"]


@pytest.fixture
def ctx(built):
    """a context of the test's own: its scratch starts empty"""
    with G.Context(0) as c:
        yield c


@pytest.fixture
def dev(ctx):
    d = Dev(ctx)
    yield d
    d.free()


def _finite(rng, n):
    """quiet noise with a hot sample every few hundred: something for the limiter to hold down"""
    x = (rng.standard_normal(n) * 0.1).astype(np.float32)
    x[::257] = np.float32(0.9)
    return x


@pytest.fixture(scope="module")
def rows_and_models():
    """the rows of A and B, awkward (for the measurements) and finite (for the limiter), with what the models say of them —
    computed once and never changed"""
    rng = np.random.default_rng(2026)
    coef = G.kweighting(RATE)
    out = {}
    for name, (stride, lengths) in SHAPES.items():
        rows = [_awkward(rng, n) for n in lengths]
        finite = [_finite(rng, n) for n in lengths]
        for x in rows + finite:
            x.setflags(write=False)
        serial = kweight_hops_model(rows, RATE, coef)
        segmented = segmented_hops_model(rows, RATE, coef)
        out[name] = dict(
            stride=stride, rows=rows, finite=finite,
            levels=[row_model(x) for x in rows],
            true_peak=[true_peak_model(x) for x in rows],
            loudness=[(gate_model(h, HOP), b) for h, b in serial],
            segmented=[(gate_model(h, HOP), b) for h, b in segmented],
            limit=limiter_model(finite, np.float32(0.5), 5, group=1))
    assert sum(m[2] for m in out["B"]["levels"]) > 100 and out["B"]["loudness"][0][0] > 0
    assert np.count_nonzero(out["B"]["limit"][2]) >= 4 and np.count_nonzero(out["A"]["limit"][2]) >= 1
    return out


def _placed(ctx, dev, S, key):
    n = len(S["rows"])
    return _place(ctx, dev, S[key], list(range(n)), n, S["stride"])[:2] + (n,)


def _three_times(ctx, dev, models, key, call):
    """call(rows_dev, stride, d_len, n, S) on A, B and A again -> the three results"""
    placed = {name: _placed(ctx, dev, models[name], key) for name in SHAPES}
    return [call(*placed[name], models[name]) for name in ORDER]


def test_levels(ctx, dev, rows_and_models):
    def call(rows_dev, d_len, n, S):
        sumsq, peak, bad = ctx.levels(rows_dev, S["stride"], d_len, n)
        assert same_bits(sumsq, np.array([m[0] for m in S["levels"]], np.float64))
        assert same_bits(peak, np.array([m[1] for m in S["levels"]], np.float32))
        assert np.array_equal(bad, [m[2] for m in S["levels"]])
        return sumsq, peak, bad

    first, _, third = _three_times(ctx, dev, rows_and_models, "rows", call)
    assert same_bits(first[0], third[0]) and same_bits(first[1], third[1]) and np.array_equal(first[2], third[2])


def test_true_peak(ctx, dev, rows_and_models):
    def call(rows_dev, d_len, n, S):
        tp, bad = ctx.true_peak(rows_dev, S["stride"], d_len, n)
        assert same_bits(tp, np.array([m[0] for m in S["true_peak"]], np.float64))
        assert np.array_equal(bad, [m[1] for m in S["true_peak"]])
        return tp, bad

    first, _, third = _three_times(ctx, dev, rows_and_models, "rows", call)
    assert same_bits(first[0], third[0]) and np.array_equal(first[1], third[1])


@pytest.mark.parametrize("which", ["loudness", "segmented"])
def test_loudness_through_the_contexts_hop_scratch(ctx, dev, rows_and_models, which):
    """no hop sums asked for: they go through the context's scratch (the segmented call: the hops' non-finite counts too)"""
    measure = ctx.loudness if which == "loudness" else ctx.loudness_segmented

    def call(rows_dev, d_len, n, S):
        gated, hops, bad = measure(rows_dev, S["stride"], d_len, n, RATE, hops=False)
        assert hops is None
        assert same_bits(gated, np.array([m[0] for m in S[which]], np.float64))
        assert np.array_equal(bad, [m[1] for m in S[which]])
        return gated, bad

    first, _, third = _three_times(ctx, dev, rows_and_models, "rows", call)
    assert same_bits(first[0], third[0]) and np.array_equal(first[1], third[1])


def test_limit(ctx, dev, rows_and_models):
    def call(rows_dev, d_len, n, S):
        stride = S["stride"]
        d_out = dev.up(np.full(n * stride, -7.25, np.float32))
        min_gain, n_limited, bad = ctx.limit(rows_dev, stride, d_len, n, 0.5, 5, d_out, stride, 1)
        out = dev.down(d_out, (n, stride), np.float32)
        w_out, w_gain, w_limited, w_bad = S["limit"][:4]
        assert same_bits(min_gain, w_gain) and np.array_equal(n_limited, w_limited) and np.array_equal(bad, w_bad)
        for i, z in enumerate(w_out):
            assert same_bits(out[i, :len(z)], z), i
            assert np.all(out[i, len(z):] == -7.25), i
        return out, min_gain, n_limited

    first, _, third = _three_times(ctx, dev, rows_and_models, "finite", call)
    assert same_bits(first[0], third[0]) and same_bits(first[1], third[1]) and np.array_equal(first[2], third[2])


def test_limited_leveled_mix(ctx, dev):
    """grail_batch_mix_leveled_limited (RMS) on 4 short utterances, on 12 twice as long, on the 4 again: the block of rows,
    the plan's buffers and the block's numbers all grow under the stream and are then reused"""
    voices = W.preset_voices(2)
    ctx.set_voices(voices)
    results = {}
    for name, n, scale, seed in (("small", 4, 0.1, 51), ("large", 12, 0.2, 52)):
        segs, offs, vids, seeds, stride = W.speech_like_batch(n, np.random.default_rng(seed), n_voices=2, scale=scale)
        ref, ref_len = _oracle(voices, segs, offs, vids, seeds, stride)
        rng = np.random.default_rng(seed + 10)
        item_rows = np.concatenate([np.arange(n), rng.integers(0, n, n)]).astype(np.uint32)
        level_db = rng.uniform(-30.0, -10.0, len(item_rows)).astype(np.float32)
        # a ceiling that about half of the items reach, by the models: the leveled gain times the row's true peak
        rows = [ref[u, :ref_len[u]] for u in range(n)]
        leveled, _ = gains_model(G.LEVEL_RMS, level_db, item_rows, sumsq=np.array([row_model(x)[0] for x in rows]),
                                 row_len=ref_len)
        reach = leveled.astype(np.float64) * np.array([true_peak_model(x)[0] for x in rows])[item_rows]
        results[name] = dict(batch=(segs, offs, vids, seeds), ref=ref, ref_len=ref_len, item_rows=item_rows, level_db=level_db,
                             ceiling_db=float(np.float32(20.0 * np.log10(np.median(reach)))),
                             item_tracks=(item_rows % 2).astype(np.uint32),
                             item_offs=rng.integers(0, 3000, len(item_rows)).astype(np.uint64),
                             track_len=3000 + int(ref_len.max()))
    assert results["large"]["ref_len"].max() > 1.5 * results["small"]["ref_len"].max()
    got = []
    for name in ("small", "large", "small"):
        R = results[name]
        track_len = R["track_len"]
        track_stride = (track_len + 63) // 64 * 64
        b = ctx.upload(*R["batch"])
        try:
            d_t = dev.alloc(2 * track_stride * 4)
            out_len, gains, unleveled, limited = b.mix_leveled_limited(
                R["item_rows"], R["item_offs"], R["level_db"], d_t, track_stride, 2, track_len, ceiling_db=R["ceiling_db"],
                item_tracks=R["item_tracks"], mode=G.LEVEL_RMS)
        finally:
            b.free()
        assert np.array_equal(out_len, R["ref_len"]) and unleveled == 0 and 0 < limited < len(R["item_rows"]), (name, limited)
        tracks = dev.down(d_t, (2, track_stride), np.float32)[:, :track_len]
        assert same_bits(tracks, fold(R["ref"], R["ref_len"], R["item_rows"], R["item_tracks"], R["item_offs"], gains, 2,
                                      track_len)), name
        got.append((tracks, gains, limited))
    assert same_bits(got[0][0], got[2][0]) and same_bits(got[0][1], got[2][1]) and got[0][2] == got[2][2]


def test_live_stream_staging_grows_under_the_stream(ctx):
    """4 utterances: one segment each, then 200 segments in one call (the device staging of an append, sized for the first,
    is freed and allocated anew behind a pull that is still queued), then one each; pulled to the end, the rows are the
    one-shot rendering's bits"""
    voices = W.preset_voices(4)
    ctx.set_voices(voices)
    rng = np.random.default_rng(77)
    n_utt, per = 4, 52
    vids = np.arange(n_utt, dtype=np.uint32)
    seeds = (np.arange(n_utt) * 7919 + 3).astype(np.uint32)
    scripts = []
    for u in range(n_utt):
        ph = rng.choice([G.PH_A, G.PH_E, G.PH_SILENCE, G.PH_STOP], size=per, p=[0.4, 0.4, 0.15, 0.05])
        ln = rng.uniform(0.004, 0.012, size=per).astype(np.float32)
        bl = (2.0 ** -rng.integers(6, 9, size=per)).astype(np.float32)
        hz = (rng.uniform(90.0, 220.0, size=per) / 48000.0).astype(np.float32)
        scripts.append(G.segments(list(zip(ph.tolist(), ln.tolist(), bl.tolist(), hz.tolist()))))
    stride, rows = 8192, [[] for _ in range(n_utt)]
    d_out, d_len = ctx.device_alloc(n_utt * stride * 4), ctx.device_alloc(n_utt * 4)
    d_head, d_head_len = ctx.device_alloc(n_utt * 64 * 4), ctx.device_alloc(n_utt * 4)
    st = G.LiveStream(ctx, n_utt, vids, seeds, ring_segments=64)

    def collect(d_rows, d_lens, row_stride):
        ctx.sync()
        lens = np.zeros(n_utt, np.uint32)
        ctx.d2h(lens, d_lens, n_utt * 4)
        buf = np.zeros((n_utt, row_stride), np.float32)
        ctx.d2h(buf, d_rows, buf.nbytes)
        for u in range(n_utt):
            rows[u].append(buf[u, :lens[u]].copy())
        return int(lens.max())

    def append(first, k):
        st.append(np.concatenate([s[first:first + k] for s in scripts]), np.arange(n_utt + 1) * k)

    try:
        append(0, 1)                                            # 4 segments: the staging's first size
        st.next_async(16, d_head, 64, d_head_len)               # queued, not waited for (a Sequencer whose next segment
        append(1, per - 2)                                      # is not there yet may pause: 0 to 16 samples a row)
        assert collect(d_head, d_head_len, 64) <= 16            # 200 segments: the staging grew behind that pull
        append(per - 1, 1)
        st.finish()
        for _ in range(64):
            st.next_async(stride, d_out, stride, d_len)
            if collect(d_out, d_len, stride) == 0:
                break
        else:
            raise AssertionError("the live stream never ended")
    finally:
        st.close()
        for p in (d_out, d_len, d_head, d_head_len):
            ctx.device_free(p)
    ov = [O.Voice.from_buffer_copy(bytes(v)) for v in voices]
    for u in range(n_utt):
        ref, n = O.synthesize_phonemes(ov[vids[u]], scripts[u], int(seeds[u]))
        got = np.concatenate(rows[u])
        assert len(got) == n, (u, len(got), n)
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), u
