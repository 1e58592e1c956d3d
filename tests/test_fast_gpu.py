"""Fast mode ("arithmetic" = 1, the tolerance north_star allows) against the oracle.

Contract (include/grail_hip.h): |fast - reference| <= GRAIL_FAST_TOLERANCE = 64 * 2^-23 of full
scale, sample for sample; lengths identical; the discontinuous state (segment boundaries, jitter
wraps, saw edges) never moves, so the error is rounding-level everywhere, never an O(1) glitch.
The yardstick printed beside it is the reference's own rounding noise: the oracle's binary32
rendering against the same formulas evaluated in double precision on the same parameter track.
"""
import os

import numpy as np
import pytest

import grail_hip as G
import oracle_lib as O
from grail_hip import workload as W

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
TOL = G.FAST_TOLERANCE          # 64 * 2^-23


def _ovoices(voices):
    return [O.Voice.from_buffer_copy(bytes(v)) for v in voices]


def _render(ctx, fast, segs, offs, vids, seeds, stride, lanes=0):
    ctx.set_option("arithmetic", 1 if fast else 0)
    ctx.set_option("lanes_per_utterance", lanes)
    try:
        return ctx.synthesize(segs, offs, vids, seeds, out_stride=stride)
    finally:
        ctx.set_option("arithmetic", 0)
        ctx.set_option("lanes_per_utterance", 0)


def _worst_rel(a, b, lens):
    """Largest |a - b| of any utterance in units of 2^-23 of max(1, that utterance's peak in b): the contract."""
    k = 0.0
    for u in range(len(lens)):
        n = int(lens[u])
        if n:
            d = float(np.max(np.abs(a[u, :n].astype(np.float64) - b[u, :n].astype(np.float64))))
            k = max(k, d / max(1.0, float(np.max(np.abs(b[u, :n])))))
    return k / ULP


def _worst(a, b, lens):
    k = 0.0
    for u in range(len(lens)):
        n = int(lens[u])
        if n:
            k = max(k, float(np.max(np.abs(a[u, :n].astype(np.float64) - b[u, :n].astype(np.float64)))))
    return k / ULP


@pytest.mark.parametrize("n_voices", [1, 8])
@pytest.mark.parametrize("lanes", [0, 1, 2, 4, 8])
def test_fast_mode_within_tolerance_of_the_oracle(gpu_ctx, n_voices, lanes):
    """Configs 3 / 4 in miniature (same corpus generator, 0.25 s segments), every lane mapping."""
    voices = W.single_voice() if n_voices == 1 else W.preset_voices(8)
    gpu_ctx.set_voices(voices)
    n_utt = 96
    segs, offs, vids, seeds = W.make_batch(n_utt, n_voices=n_voices, length=0.25, blend_length=0.25)
    stride = W.max_samples(length=0.25)
    out, out_len = _render(gpu_ctx, True, segs, offs, vids, seeds, stride, lanes)
    assert "FAST" in gpu_ctx.last_kernel_name()
    ref, ref_len = O.synthesize_batch(_ovoices(voices), segs, offs, vids, seeds, stride)
    assert np.array_equal(out_len, ref_len)
    k = _worst(out, ref, ref_len)
    print(f"fast vs oracle: voices={n_voices} lanes={lanes}: max |d| = {k:.1f} * 2^-23")
    assert k * ULP <= TOL
    assert k > 0.0          # it IS a different arithmetic: an exact match would mean the option was ignored


def test_fast_mode_error_is_of_the_order_of_the_references_own_rounding_noise(gpu_ctx):
    """k(fast vs reference) next to k0(reference vs its own formulas in double precision)."""
    voices = W.preset_voices(8)
    gpu_ctx.set_voices(voices)
    n_utt = 64
    segs, offs, vids, seeds = W.make_batch(n_utt, n_voices=8)        # full 2 s utterances
    stride = W.max_samples()
    out, out_len = _render(gpu_ctx, True, segs, offs, vids, seeds, stride)
    ov = _ovoices(voices)
    ref, ref_len = O.synthesize_batch(ov, segs, offs, vids, seeds, stride)
    O.set_precise(True)
    try:
        ref64, len64 = O.synthesize_batch(ov, segs, offs, vids, seeds, stride)
    finally:
        O.set_precise(False)
    assert np.array_equal(out_len, ref_len) and np.array_equal(len64, ref_len)
    k = _worst(out, ref, ref_len)
    k0 = _worst(ref, ref64, ref_len)
    k64 = _worst(out, ref64, ref_len)
    print(f"config-4 corpus, 64 x 2 s: fast vs reference {k:.1f}, reference vs double precision {k0:.1f}, "
          f"fast vs double precision {k64:.1f}  (units of 2^-23)")
    assert k * ULP <= TOL
    assert k <= 16.0 * max(k0, 1.0)


def test_fast_mode_keeps_every_edge_case_structurally_exact(gpu_ctx):
    """Ragged lists, empty utterances, silent pairs, blend lengths that are not powers of two, a
    blend shorter than the segment (the alpha kink), one-sample segments: lengths equal the
    oracle's and every sample is within tolerance (event tiles run the exact steps)."""
    voices = W.single_voice()
    gpu_ctx.set_voices(voices)
    A, E, S = G.PH_A, G.PH_E, G.PH_SILENCE
    f = 120.0 / 48000.0
    utts = [
        [(S, 0.05, 0.05, f), (A, 0.05, 0.05, f)],
        [(A, 0.08, 0.02, f), (E, 0.08, 0.02, 1.3 * f), (A, 0.03, 0.01, f)],      # kink: blend < length
        [(E, 0.07, 0.03, f), (S, 0.04, 0.03, f), (S, 0.04, 0.03, f), (A, 0.05, 0.03, f)],  # non-2^k blends
        [],
        [(A, 1.0 / 48000.0, 0.5, f), (E, 0.05, 0.05, f)],                        # one-sample segment
        [(A, 0.2, 0.2, 0.9 * f)],
        [(G.PH_STOP, 0.03, 0.03, f), (G.PH_GLIDE, 0.03, 0.03, f), (E, 0.06, 0.06, 2 * f)],
    ] * 5
    segs = G.segments([s for u in utts for s in u])
    offs = np.cumsum([0] + [len(u) for u in utts]).astype(np.uint32)
    seeds = np.arange(len(utts), dtype=np.uint32) * 77
    stride = 16384
    ref, ref_len = O.synthesize_batch(_ovoices(voices), segs, offs, None, seeds, stride)
    for lanes in (0, 1, 2, 4, 8):
        out, out_len = _render(gpu_ctx, True, segs, offs, None, seeds, stride, lanes)
        assert np.array_equal(out_len, ref_len), lanes
        k = _worst(out, ref, ref_len)
        print(f"edge cases, lanes={lanes}: {k:.1f} * 2^-23")
        assert k * ULP <= TOL


def test_fast_mode_fuzz_on_random_voice_tables(gpu_ctx):
    """Random (sane) voice tables and segment lists: formants anywhere in (60 Hz, 0.4 fs), bandwidths
    30-600 Hz (two trials of three: at least frequency / 30, the sharpness of speech formants; the third: any,
    and what is sharper than the fast kernels keep their tolerance for goes to the exact kernels), every amplitude
    pattern, blends from 60 ms to 1 s (also longer than the segment, also not powers of two).  The tolerance holds
    relative to max(1, peak), no structure moves, and the fast tiles really ran (the guard sends too-fast
    parameter motion to shorter sub-tiles / exact steps)."""
    # GRAIL_FAST_FUZZ_SEED / GRAIL_FAST_FUZZ_TRIALS: soak runs (tools/fuzz_soak.sh); the default suite stays short
    rng = np.random.default_rng(int(os.environ.get("GRAIL_FAST_FUZZ_SEED", "20261002")))
    worst = 0.0
    tiles0 = gpu_ctx.get_option("fast_wave_tiles")
    for trial in range(int(os.environ.get("GRAIL_FAST_FUZZ_TRIALS", "6"))):
        voices = []
        centres = [np.exp(rng.uniform(np.log(150.0), np.log(12000.0), 8)) for _ in range(3)]
        for _ in range(3):
            v = G.voice_generic(48000.0)
            for p in range(2):
                # formant k sits within +-35 % of a centre shared by the voice's two phonemes
                freq, bw = centres[_] * rng.uniform(0.65, 1.35, 8), rng.uniform(30, 600, 8)
                if trial % 3 != 2:      # two trials of three: resonances as sharp as speech has them (Q <= 30)
                    bw = np.maximum(bw, freq / 30.0)
                e = G.elem_new_phoneme(freq, bw,
                                       rng.uniform(200, 4000, 8), rng.uniform(0, 1, 8), rng.uniform(0, 1, 8),
                                       rng.uniform(0.0, 1, 8) * (rng.uniform(0, 1, 8) > 0.3) + 1e-3)
                v.phonemes[p] = G.elem_resample(e, 44100.0, 48000.0)
            voices.append(v if trial % 3 == 2 else W.tame_voice(v))    # (bandwidths widened until served)
        gpu_ctx.set_voices(voices)
        # sharper tables are rendered by the second tier — the reference's own filter coefficients at every sample
        # (include/grail_hip.h, grail_fast_sharpness): the tolerance is the same
        served = all(G.fast_sharpness(v) <= G.FAST_SHARPNESS_LIMIT for v in voices)
        assert gpu_ctx.get_option("fast_arithmetic_served") == (1 if served else 2)
        assert served or trial % 3 == 2
        n_utt = 40
        utts = []
        for u in range(n_utt):
            n = int(rng.integers(1, 5))
            utts.append([(int(rng.choice([G.PH_A, G.PH_E, G.PH_SILENCE])), float(rng.uniform(0.05, 0.3)),
                          float(rng.choice([0.0625, 0.125, 0.25, 0.5, 1.0, 0.3, 0.07])),
                          float(rng.uniform(80, 400) / 48000.0)) for _ in range(n)])
        segs = G.segments([s for u in utts for s in u])
        offs = np.cumsum([0] + [len(u) for u in utts]).astype(np.uint32)
        vids = rng.integers(0, 3, n_utt).astype(np.uint32)
        seeds = rng.integers(0, 2 ** 32, n_utt, dtype=np.uint64).astype(np.uint32)
        stride = 65536
        ref, ref_len = O.synthesize_batch(_ovoices(voices), segs, offs, vids, seeds, stride)
        for lanes in (0, 1, 4):
            out, out_len = _render(gpu_ctx, True, segs, offs, vids, seeds, stride, lanes)
            assert np.array_equal(out_len, ref_len)
            # (a batch is judged by the voices it uses; the second tier has one-lane and time-split kernels only: a pinned
            # wider mapping gets the exact kernels, and left to itself the library takes whichever is faster — the exact
            # kernels' bits satisfy any tolerance)
            used = all(G.fast_sharpness(voices[int(i)]) <= G.FAST_SHARPNESS_LIMIT for i in set(vids.tolist()))
            ran = gpu_ctx.get_option("last_launch_fast")
            assert ran == 1 if used else (ran == 2 if lanes == 1 else ran == 0 if lanes == 4 else ran in (0, 2)), (trial, lanes, ran)
            k = _worst_rel(out, ref, ref_len)
            worst = max(worst, k)
            assert k * ULP <= TOL, (trial, lanes, k)
    print(f"fuzz: worst {worst:.1f} * 2^-23 (relative to max(1, peak of the utterance))")
    tiles = gpu_ctx.get_option("fast_wave_tiles") - tiles0
    steps = gpu_ctx.get_option("general_wave_steps")
    print(f"fuzz: {tiles} wave-tiles rendered in fast arithmetic")
    assert worst > 0.0 and tiles > 500
    gpu_ctx.set_voices(W.single_voice())


@pytest.mark.parametrize("config", [2, 3, 4])
def test_fast_mode_full_size_against_exact_mode_on_the_device(gpu_ctx, config):
    """BASELINE configs 2, 3, 4 at full size: fast rows against exact rows (which are bit-identical
    to the oracle) compared on the device; 64 utterances spread over the batch also against the oracle."""
    n_utt = 4096 if config == 2 else 65536
    n_voices = 8 if config == 4 else 1
    voices = W.single_voice() if n_voices == 1 else W.preset_voices(8)
    ctx = gpu_ctx
    ctx.set_voices(voices)
    segs, offs, vids, seeds = W.make_batch(n_utt, n_voices=n_voices)
    stride = W.max_samples()
    batch = ctx.upload(segs, offs, vids, seeds)
    d_a = ctx.device_alloc(n_utt * stride * 4)
    d_b = ctx.device_alloc(n_utt * stride * 4)
    d_la = ctx.device_alloc(n_utt * 4)
    d_lb = ctx.device_alloc(n_utt * 4)
    try:
        ctx.set_option("arithmetic", 0)
        batch.synthesize_async(d_a, stride, d_la)
        ctx.sync()
        ctx.set_option("arithmetic", 1)
        batch.synthesize_async(d_b, stride, d_lb)
        ctx.sync()
        assert "FAST" in ctx.last_kernel_name()
        md, sq, bad = ctx.compare(d_a, d_b, stride, d_la, d_lb, n_utt)
        lens = np.zeros(n_utt, dtype=np.uint32)
        ctx.d2h(lens, d_la, n_utt * 4)
        assert int(bad.sum()) == 0
        k = float(md.max()) / ULP
        rms = float(np.sqrt(sq.sum() / float(lens.astype(np.uint64).sum()))) / ULP
        print(f"config {config}: fast vs exact over {n_utt} utterances: max {k:.1f}, rms {rms:.2f} (2^-23)")
        assert md.max() <= TOL
        # and a spread sample of the fast rows against the oracle itself
        pick = np.linspace(0, n_utt - 1, 64).astype(np.int64)
        ps = segs.reshape(n_utt, -1)[pick].reshape(-1)
        po = (np.arange(len(pick) + 1) * W.SEGMENTS_PER_UTT).astype(np.uint32)
        ref, ref_len = O.synthesize_batch(_ovoices(voices), ps, po, vids[pick], seeds[pick], stride)
        row = np.zeros(stride, dtype=np.float32)
        worst = 0.0
        for i, u in enumerate(pick):
            ctx.d2h(row, d_b, stride * 4, offset=int(u) * stride * 4)
            n = int(ref_len[i])
            assert n == int(lens[u])
            worst = max(worst, float(np.max(np.abs(row[:n].astype(np.float64) - ref[i, :n]))))
        print(f"config {config}: 64 spread utterances, fast vs oracle: {worst / ULP:.1f} * 2^-23")
        assert worst <= TOL
    finally:
        ctx.set_option("arithmetic", 0)
        for p in (d_a, d_b, d_la, d_lb):
            ctx.device_free(p)
        batch.free()
        ctx.set_voices(W.single_voice())


# ---- the time-parallel scan kernel (small batches, fast arithmetic) ------------------------------
@pytest.mark.parametrize("split", [1, 0])
@pytest.mark.parametrize("n_voices", [1, 8])
def test_scan_kernel_small_batch_within_tolerance(gpu_ctx, n_voices, split):
    """Few utterances in fast mode go to scan_kernels.hip: lanes = time, recurrences by parallel scan.
    Lengths equal the oracle's (the chain is exact), samples within the fast-mode tolerance.  Both
    flavours: three-stage workgroups (the carrier phase on a wave of its own, few utterances) and
    two-stage ones (many utterances)."""
    voices = W.single_voice() if n_voices == 1 else W.preset_voices(8)
    gpu_ctx.set_voices(voices)
    n_utt = 48
    segs, offs, vids, seeds = W.make_batch(n_utt, n_voices=n_voices)          # full 2 s utterances
    stride = W.max_samples()
    split_default = gpu_ctx.get_option("time_parallel_scan_split_max_utterances")
    gpu_ctx.set_option("time_parallel_scan_split_max_utterances", split_default if split else 0)
    try:
        out, out_len = _render(gpu_ctx, True, segs, offs, vids, seeds, stride)
    finally:
        gpu_ctx.set_option("time_parallel_scan_split_max_utterances", split_default)
    assert gpu_ctx.last_kernel_name() == "scan_kernel<pairs=%d,%sFAST>" % (2 if n_voices == 1 else 4, "SPLIT," if split else "")
    ref, ref_len = O.synthesize_batch(_ovoices(voices), segs, offs, vids, seeds, stride)
    assert np.array_equal(out_len, ref_len)
    k = _worst(out, ref, ref_len)
    print(f"scan kernel, voices={n_voices}: max |d| = {k:.1f} * 2^-23")
    assert 0.0 < k * ULP <= TOL
    # the option switches it off (A/B).  The cost model then takes the next best family for a batch this small: the
    # time-split kernels (3.1 ms where the pipelined exact workgroups take 6.5); with those switched off as well the
    # pipelined EXACT workgroups — faster than the fast lane kernels there, and exact bits satisfy the tolerance; with
    # the lane mapping pinned the fast lane kernels run
    gpu_ctx.set_option("time_parallel_scan", 0)
    try:
        out1, len1 = _render(gpu_ctx, True, segs, offs, vids, seeds, stride)
        assert "SPLIT" in gpu_ctx.last_kernel_name() and np.array_equal(len1, ref_len)
        assert 0.0 < _worst(out1, ref, ref_len) * ULP <= TOL
        gpu_ctx.set_option("time_split", 0)
        out2, len2 = _render(gpu_ctx, True, segs, offs, vids, seeds, stride)
        assert "PIPE" in gpu_ctx.last_kernel_name() and np.array_equal(len2, ref_len)
        assert gpu_ctx.get_option("last_launch_fast") == 0      # (what ran, not what was asked for)
        assert _worst(out2, ref, ref_len) == 0.0
        out3, len3 = _render(gpu_ctx, True, segs, offs, vids, seeds, stride, lanes=8)
        assert "FAST" in gpu_ctx.last_kernel_name() and np.array_equal(len3, ref_len)
        assert 0.0 < _worst(out3, ref, ref_len) * ULP <= TOL
    finally:
        gpu_ctx.set_option("time_parallel_scan", 1)
        gpu_ctx.set_option("time_split", 1)
    gpu_ctx.set_voices(W.single_voice())


def test_scan_kernel_edge_cases(gpu_ctx):
    """Ragged lists, an empty utterance, silent pairs, specials, two-sample segments, rows cut at
    out_stride: structure identical to the oracle, samples within tolerance."""
    voices = W.single_voice()
    gpu_ctx.set_voices(voices)
    A, E, S = G.PH_A, G.PH_E, G.PH_SILENCE
    f = 120.0 / 48000.0
    utts = [
        [(S, 0.05, 0.0625, f), (A, 0.05, 0.0625, f)],
        [(A, 0.08, 0.03125, f), (E, 0.08, 0.03125, 1.3 * f), (A, 0.03, 0.015625, f)],
        [(E, 0.07, 0.0625, f), (S, 0.04, 0.0625, f), (S, 0.04, 0.0625, f), (A, 0.05, 0.0625, f)],
        [],
        [(A, 2.5 / 48000.0, 0.5, f), (E, 0.05, 0.0625, f)],
        [(A, 0.7, 0.25, 0.9 * f)],
        [(G.PH_STOP, 0.03, 0.03125, f), (G.PH_GLIDE, 0.03, 0.03125, f), (E, 0.06, 0.0625, 2 * f)],
        # 4 ms blends: the coefficients move too fast for the eight-sample interpolation, its guard sends
        # the super-tiles of the blend to the direct evaluation
        [(A, 0.2, 0.00390625, f), (E, 0.2, 0.00390625, 1.2 * f), (A, 0.1, 0.00390625, 0.8 * f)],
    ] * 3
    segs = G.segments([s for u in utts for s in u])
    offs = np.cumsum([0] + [len(u) for u in utts]).astype(np.uint32)
    seeds = np.arange(len(utts), dtype=np.uint32) * 1234567
    split_default = gpu_ctx.get_option("time_parallel_scan_split_max_utterances")
    for stride, split in ((40000, 1), (2048, 1), (40000, 0), (2048, 0)):    # 2048 cuts the long rows
        ref, ref_len = O.synthesize_batch(_ovoices(voices), segs, offs, None, seeds, stride)
        ref_len = np.minimum(ref_len, stride)
        gpu_ctx.set_option("arithmetic", 1)
        gpu_ctx.set_option("time_parallel_scan_split_max_utterances", split_default if split else 0)
        try:
            out, out_len = gpu_ctx.synthesize(segs, offs, None, seeds, out_stride=stride, allow_truncation=True)
        finally:
            gpu_ctx.set_option("arithmetic", 0)
            gpu_ctx.set_option("time_parallel_scan_split_max_utterances", split_default)
        assert gpu_ctx.last_kernel_name().startswith("scan_kernel") and ("SPLIT" in gpu_ctx.last_kernel_name()) == bool(split)
        assert np.array_equal(out_len, ref_len), stride
        k = _worst(out, ref, ref_len)
        print(f"scan kernel edge cases, stride {stride}, split {split}: {k:.1f} * 2^-23")
        assert k * ULP <= TOL


@pytest.mark.parametrize("split", [1, 0])
def test_scan_kernel_runs_of_short_segments(gpu_ctx, split):
    """Consecutive segments of 2 - 5 ms (96 - 240 samples): every super-tile of 512 samples opens a new
    parameter epoch, so the three-stage workgroups have three epochs in flight — one parameter block per
    super-tile in flight (the block ring had two entries once: the chain wave overwrote the block the filter
    wave was still reading).  Run several times: the fault was a race."""
    voices = W.single_voice()
    gpu_ctx.set_voices(voices)
    rng = np.random.default_rng(5)
    A, E, S = G.PH_A, G.PH_E, G.PH_SILENCE
    f = 120.0 / 48000.0
    utts = [[(int(rng.choice([A, E, E, A, S])), float(rng.uniform(0.002, 0.005)),
              float(rng.choice([0.00390625, 0.001953125, 0.0078125])), f * float(rng.uniform(0.8, 1.6)))
             for _ in range(60)] for _ in range(24)]
    segs = G.segments([s for u in utts for s in u])
    offs = np.cumsum([0] + [len(u) for u in utts]).astype(np.uint32)
    seeds = np.arange(len(utts), dtype=np.uint32) * 977 + 3
    stride = 16384
    ref, ref_len = O.synthesize_batch(_ovoices(voices), segs, offs, None, seeds, stride)
    split_default = gpu_ctx.get_option("time_parallel_scan_split_max_utterances")
    gpu_ctx.set_option("time_parallel_scan_split_max_utterances", split_default if split else 0)
    try:
        for attempt in range(4):
            out, out_len = _render(gpu_ctx, True, segs, offs, None, seeds, stride)
            assert gpu_ctx.last_kernel_name().startswith("scan_kernel") and ("SPLIT" in gpu_ctx.last_kernel_name()) == bool(split)
            assert np.array_equal(out_len, ref_len)
            k = _worst(out, ref, ref_len)
            assert k * ULP <= TOL, (attempt, k)
        print(f"scan kernel, runs of short segments, split {split}: {k:.1f} * 2^-23")
    finally:
        gpu_ctx.set_option("time_parallel_scan_split_max_utterances", split_default)


def test_scan_kernel_gate_sends_unsafe_tables_elsewhere(gpu_ctx):
    """A table outside the safe window (a formant at frequency 0: the reference emits NaN) does not take
    the scan kernel.  Blend lengths that are not powers of two do (the chain wave then takes the IEEE
    quotient clk / blend_length instead of the product with the exact reciprocal)."""
    v = G.voice_generic(48000.0)
    v.phonemes[0].formant_freq[7] = 0.0
    gpu_ctx.set_voices([v])
    segs, offs, vids, seeds = W.make_batch(8, length=0.05, blend_length=0.0625)
    out, out_len = _render(gpu_ctx, True, segs, offs, vids, seeds, 16384)
    assert not gpu_ctx.last_kernel_name().startswith("scan_kernel")
    voices = W.single_voice()
    gpu_ctx.set_voices(voices)
    segs, offs, vids, seeds = W.make_batch(8, length=0.05, blend_length=0.03)
    out, out_len = _render(gpu_ctx, True, segs, offs, vids, seeds, 16384)
    assert gpu_ctx.last_kernel_name().startswith("scan_kernel<pairs=2")      # four live formants: two pairs
    ref, ref_len = O.synthesize_batch(_ovoices(voices), segs, offs, vids, seeds, 16384)
    assert np.array_equal(out_len, ref_len)
    k = _worst(out, ref, ref_len)
    print(f"scan kernel, blend length 0.03 s: max |d| = {k:.1f} * 2^-23")
    assert 0.0 < k * ULP <= TOL


def test_fast_mode_pcm16_rows_are_the_conversion_of_the_fast_f32_rows(gpu_ctx):
    """i16 rows in fast mode (lane kernels and scan kernel): exactly `(x * 32767) as i16` of the f32 rows the
    same kernels produce (examples/cli.rs:49), i.e. the conversion is fused, not a different rendering."""
    voices = W.single_voice()
    gpu_ctx.set_voices(voices)
    for n_utt, scan in ((24, 1), (24, 0)):
        segs, offs, vids, seeds = W.make_batch(n_utt, length=0.05, blend_length=0.0625)
        stride = 16384
        gpu_ctx.set_option("arithmetic", 1)
        gpu_ctx.set_option("time_parallel_scan", scan)
        try:
            f32, n32 = gpu_ctx.synthesize(segs, offs, vids, seeds, out_stride=stride)
            name32 = gpu_ctx.last_kernel_name()
            i16, n16 = gpu_ctx.synthesize_pcm16(segs, offs, vids, seeds, out_stride=stride)
            assert gpu_ctx.last_kernel_name() == name32 and name32.startswith("scan_kernel") == bool(scan)
        finally:
            gpu_ctx.set_option("arithmetic", 0)
            gpu_ctx.set_option("time_parallel_scan", 1)
        assert np.array_equal(n32, n16)
        want = np.clip(np.trunc(f32.astype(np.float32) * np.float32(32767.0)), -32768, 32767).astype(np.int16)
        for u in range(n_utt):
            assert np.array_equal(i16[u, :n16[u]], want[u, :n16[u]]), (scan, u)


@pytest.mark.parametrize("lanes", [0, 1, 4, 8])
def test_fast_mode_streams(gpu_ctx, lanes):
    """Resumable streams in fast mode: ragged chunk sizes, f32; the concatenation has the oracle's
    lengths and is within the fast-mode tolerance of the oracle's samples."""
    voices = W.single_voice()
    gpu_ctx.set_voices(voices)
    n_utt = 70
    segs, offs, vids, seeds = W.make_batch(n_utt, length=0.06, blend_length=0.0625)
    total = W.max_samples(length=0.06)
    ref, ref_len = O.synthesize_batch(_ovoices(voices), segs, offs, vids, seeds, total)
    gpu_ctx.set_option("lanes_per_utterance", lanes)
    gpu_ctx.set_option("arithmetic", 1)
    batch = gpu_ctx.upload(segs, offs, vids, seeds)
    chunk_cap = 1024
    d_out = gpu_ctx.device_alloc(n_utt * chunk_cap * 4)
    d_len = gpu_ctx.device_alloc(n_utt * 4)
    got = np.zeros((n_utt, total), dtype=np.float32)
    pos = np.zeros(n_utt, dtype=np.int64)
    try:
        st = G.Stream(batch)
        for chunk in [96, 33, 1000, 7, 512] * 20:
            st.next_async(chunk, d_out, chunk_cap, d_len)
            gpu_ctx.sync()
            name = gpu_ctx.last_kernel_name()
            # (a few streams on the library's own mapping take the pipelined exact workgroups: the faster kernels at this
            # size, and the reference's bits are inside any tolerance)
            assert "STREAM" in name and ("FAST" in name or (lanes == 0 and "PIPE" in name)), name
            lens = np.zeros(n_utt, dtype=np.uint32)
            gpu_ctx.d2h(lens, d_len, n_utt * 4)
            buf = np.zeros((n_utt, chunk_cap), dtype=np.float32)
            gpu_ctx.d2h(buf, d_out, buf.nbytes)
            for u in range(n_utt):
                got[u, pos[u]:pos[u] + lens[u]] = buf[u, :lens[u]]
            pos += lens
            if not lens.any():
                break
        st.close()
    finally:
        gpu_ctx.set_option("arithmetic", 0)
        gpu_ctx.set_option("lanes_per_utterance", 0)
        gpu_ctx.device_free(d_out)
        gpu_ctx.device_free(d_len)
        batch.free()
    assert np.array_equal(pos.astype(np.uint32), ref_len)
    k = _worst(got, ref, ref_len)
    print(f"fast streams, lanes={lanes}: {k:.1f} * 2^-23 ({name})")
    assert k * ULP <= TOL and (k > 0.0 or "PIPE" in name)


@pytest.mark.parametrize("sharpen,lanes,want", [(6.0, 1, 2), (6.0, 4, 0), (1.0, 1, 1)])
def test_streams_of_sharp_voices_run_the_second_tier_on_one_lane_per_utterance(gpu_ctx, sharpen, lanes, want):
    """Resumable kernels of the second tolerance tier (the reference's own coefficients): streams of a voice sharper than
    the interpolating tier allows, laid out one lane per utterance; on a wider mapping the exact kernels; a mild voice
    the interpolating tier.  Chunks concatenate to the oracle's lengths, samples within the tolerance (exact: its bits)."""
    v = G.voice_generic(48000.0)
    for p in range(2):
        for i in range(8):
            v.phonemes[p].formant_bw[i] /= sharpen
    gpu_ctx.set_voices([v])
    n_utt = 40
    segs, offs, vids, seeds = W.make_batch(n_utt, length=0.06, blend_length=0.0625)
    total = W.max_samples(length=0.06)
    ref, ref_len = O.synthesize_batch(_ovoices([v]), segs, offs, vids, seeds, total)
    gpu_ctx.set_option("lanes_per_utterance", lanes)
    gpu_ctx.set_option("arithmetic", 1)
    batch = gpu_ctx.upload(segs, offs, vids, seeds)
    d_out = gpu_ctx.device_alloc(n_utt * 1024 * 4)
    d_len = gpu_ctx.device_alloc(n_utt * 4)
    got = np.zeros((n_utt, total), dtype=np.float32)
    pos = np.zeros(n_utt, dtype=np.int64)
    try:
        st = G.Stream(batch)
        for chunk in [96, 33, 1000, 7, 512] * 20:
            st.next_async(chunk, d_out, 1024, d_len)
            gpu_ctx.sync()
            assert gpu_ctx.get_option("last_launch_fast") == want and ("MID" in gpu_ctx.last_kernel_name()) == (want == 2)
            lens = np.zeros(n_utt, dtype=np.uint32)
            gpu_ctx.d2h(lens, d_len, n_utt * 4)
            buf = np.zeros((n_utt, 1024), dtype=np.float32)
            gpu_ctx.d2h(buf, d_out, buf.nbytes)
            for u in range(n_utt):
                got[u, pos[u]:pos[u] + lens[u]] = buf[u, :lens[u]]
            pos += lens
            if not lens.any():
                break
        st.close()
    finally:
        gpu_ctx.set_option("arithmetic", 0)
        gpu_ctx.set_option("lanes_per_utterance", 0)
        gpu_ctx.device_free(d_out)
        gpu_ctx.device_free(d_len)
        batch.free()
        gpu_ctx.set_voices(W.single_voice())
    assert np.array_equal(pos.astype(np.uint32), ref_len)
    k = _worst_rel(got, ref, ref_len)
    print(f"streams, bandwidths / {sharpen}, lanes={lanes}: tier {want}, {k:.1f} * 2^-23")
    assert (k == 0.0) if want == 0 else (0.0 < k * ULP <= TOL)


# ---------------------------------------------------------------------------------------------
# Time-split fast kernels (synth_kernel<..., SPLIT>): one lane per (utterance, chunk of its time axis).
# A chunk's lane fast-forwards the exact chain, warms its filters up from zero state and renders its chunk.

def _split(ctx, chunks, span=0):
    ctx.set_option("time_split_chunks", chunks)
    ctx.set_option("time_split_span_samples", span)


@pytest.mark.parametrize("n_voices", [1, 8])
@pytest.mark.parametrize("chunks", [2, 5, 16])
def test_time_split_within_tolerance_of_the_oracle(gpu_ctx, n_voices, chunks):
    """Full 2 s utterances cut into 2 / 5 / 16 chunks: lengths are the oracle's, every sample within the
    tolerance — chunk seams included (the warm-up residual is part of the measured distance)."""
    voices = W.single_voice() if n_voices == 1 else W.preset_voices(8)
    gpu_ctx.set_voices(voices)
    n_utt = 80
    segs, offs, vids, seeds = W.make_batch(n_utt, n_voices=n_voices)
    stride = W.max_samples()
    try:
        _split(gpu_ctx, chunks)
        out, out_len = _render(gpu_ctx, True, segs, offs, vids, seeds, stride)
        assert "SPLIT" in gpu_ctx.last_kernel_name(), gpu_ctx.last_kernel_name()
        assert gpu_ctx.get_option("last_launch_chunks") == chunks
    finally:
        _split(gpu_ctx, 0)
    ref, ref_len = O.synthesize_batch(_ovoices(voices), segs, offs, vids, seeds, stride)
    assert np.array_equal(out_len, ref_len)
    k = _worst(out, ref, ref_len)
    print(f"time split, {chunks} chunks, voices={n_voices}: max |d| = {k:.1f} * 2^-23")
    assert 0.0 < k * ULP <= TOL


def test_time_split_fuzz_on_random_voice_tables(gpu_ctx):
    """Random voice tables (formants anywhere in (150 Hz, 0.35 fs), bandwidths 30 - 600 Hz — i.e. warm-up lengths
    from a few hundred to ~8 000 samples, different for every voice of the table, so the lanes of a wave reset
    their filters at different tiles), random segment lists, random chunk grids: lengths are the oracle's and the
    tolerance holds at every seam (relative to max(1, peak))."""
    rng = np.random.default_rng(int(os.environ.get("GRAIL_FAST_FUZZ_SEED", "31337")))
    worst = 0.0
    try:
        for trial in range(int(os.environ.get("GRAIL_FAST_FUZZ_TRIALS", "5"))):
            voices = []
            for _ in range(3):
                centre = np.exp(rng.uniform(np.log(150.0), np.log(12000.0), 8))
                v = G.voice_generic(48000.0)
                for p in range(2):
                    freq, bw = centre * rng.uniform(0.65, 1.35, 8), rng.uniform(30, 600, 8)
                    if trial % 3 != 2:      # (as in the fuzz of the lane kernels: the third trial is any sharpness)
                        bw = np.maximum(bw, freq / 30.0)
                    e = G.elem_new_phoneme(freq, bw,
                                           rng.uniform(200, 4000, 8), rng.uniform(0, 1, 8), rng.uniform(0, 1, 8),
                                           rng.uniform(0.0, 1, 8) * (rng.uniform(0, 1, 8) > 0.3) + 1e-3)
                    v.phonemes[p] = G.elem_resample(e, 44100.0, 48000.0)
                voices.append(v if trial % 3 == 2 else W.tame_voice(v))
            gpu_ctx.set_voices(voices)
            served = all(G.fast_sharpness(v) <= G.FAST_SHARPNESS_LIMIT for v in voices)
            assert gpu_ctx.get_option("fast_arithmetic_served") == (1 if served else 2)
            assert served or trial % 3 == 2
            n_utt = 70
            utts = []
            for u in range(n_utt):
                n = int(rng.integers(1, 6))
                utts.append([(int(rng.choice([G.PH_A, G.PH_E, G.PH_SILENCE])), float(rng.uniform(0.05, 0.3)),
                              float(rng.choice([0.0625, 0.125, 0.25, 0.5, 0.3, 0.07])),
                              float(rng.uniform(80, 400) / 48000.0)) for _ in range(n)])
            segs = G.segments([s for u in utts for s in u])
            offs = np.cumsum([0] + [len(u) for u in utts]).astype(np.uint32)
            vids = rng.integers(0, 3, n_utt).astype(np.uint32)
            seeds = rng.integers(0, 2 ** 32, n_utt, dtype=np.uint64).astype(np.uint32)
            stride = 81920
            ref, ref_len = O.synthesize_batch(_ovoices(voices), segs, offs, vids, seeds, stride)
            for chunks, span in ((2, 0), (3, int(rng.integers(20000, 70000))), (6, 0)):
                _split(gpu_ctx, chunks, span)
                out, out_len = _render(gpu_ctx, True, segs, offs, vids, seeds, stride)
                # (sharper tables: the time-split kernels of the second tier)
                used = all(G.fast_sharpness(voices[int(i)]) <= G.FAST_SHARPNESS_LIMIT for i in set(vids.tolist()))
                assert "SPLIT" in gpu_ctx.last_kernel_name() and ("MID" in gpu_ctx.last_kernel_name()) == (not used), \
                    gpu_ctx.last_kernel_name()
                assert np.array_equal(out_len, ref_len), (trial, chunks)
                k = _worst_rel(out, ref, ref_len)
                worst = max(worst, k)
                assert k * ULP <= TOL, (trial, chunks, span, k)
        print(f"time-split fuzz: worst {worst:.1f} * 2^-23 (relative to max(1, peak of the utterance))")
    finally:
        _split(gpu_ctx, 0)
        gpu_ctx.set_voices(W.single_voice())


def test_time_split_ragged_lengths_short_and_empty_utterances(gpu_ctx):
    """Utterances that end before, inside and exactly around chunk boundaries, empty ones, one-sample segments,
    non-2^k blends and a blend kink: each length is written by exactly one lane and equals the oracle's."""
    voices = W.single_voice()
    gpu_ctx.set_voices(voices)
    A, E, S = G.PH_A, G.PH_E, G.PH_SILENCE
    f = 120.0 / 48000.0
    rng = np.random.default_rng(11)
    utts = [[], [(A, 1.0 / 48000.0, 0.5, f)], [(S, 0.01, 0.01, f)]]
    for i in range(61):
        n_seg = int(rng.integers(1, 6))
        utts.append([(int(rng.choice([A, E, S])), float(rng.uniform(0.02, 0.25)),
                      float(rng.choice([0.5, 0.25, 0.03, 0.1, 0.0625])), f * float(rng.uniform(0.8, 1.9)))
                     for _ in range(n_seg)])
    # lengths that put the end of the utterance on / next to the uniform 4-chunk grid of a 36 864-sample span
    for target in (9216, 9216 + 1, 9216 - 1, 18432, 27648 + 63, 27648 - 64):
        utts.append([(A, (target + 0.5) / 48000.0, 0.25, f)])
    segs = G.segments([s for u in utts for s in u])
    offs = np.cumsum([0] + [len(u) for u in utts]).astype(np.uint32)
    seeds = np.arange(len(utts), dtype=np.uint32) * 31 + 5
    stride = 65536
    ref, ref_len = O.synthesize_batch(_ovoices(voices), segs, offs, None, seeds, stride)
    try:
        for chunks, span in ((4, 36864), (7, 0), (2, 12800)):
            _split(gpu_ctx, chunks, span)
            gpu_ctx.set_option("time_split_ff_cost_permille", 0 if span else 165)   # 0: a uniform grid
            out, out_len = _render(gpu_ctx, True, segs, offs, None, seeds, stride)
            assert "SPLIT" in gpu_ctx.last_kernel_name()
            assert np.array_equal(out_len, ref_len), (chunks, np.nonzero(out_len != ref_len)[0][:8])
            k = _worst(out, ref, ref_len)
            print(f"time split edge cases, {chunks} chunks over {span or 'auto'}: {k:.1f} * 2^-23")
            assert k * ULP <= TOL
    finally:
        _split(gpu_ctx, 0)
        gpu_ctx.set_option("time_split_ff_cost_permille", 165)


def test_time_split_truncation_and_pcm16(gpu_ctx):
    """A row capacity below the utterance length: the last chunk's lane reports the cut; i16 rows are the
    conversion of the f32 rows."""
    voices = W.single_voice()
    gpu_ctx.set_voices(voices)
    segs, offs, vids, seeds = W.make_batch(70, length=0.25, blend_length=0.25)
    stride = W.max_samples(length=0.25)
    try:
        _split(gpu_ctx, 4)
        gpu_ctx.set_option("arithmetic", 1)
        full, full_len = gpu_ctx.synthesize(segs, offs, vids, seeds, out_stride=stride)
        with pytest.raises(G.GrailError):
            gpu_ctx.synthesize(segs, offs, vids, seeds, out_stride=30016)
        pcm, pcm_len = gpu_ctx.synthesize_pcm16(segs, offs, vids, seeds, out_stride=stride)
        assert "SPLIT" in gpu_ctx.last_kernel_name()
        assert np.array_equal(pcm_len, full_len)
        want = np.clip(np.trunc(full.astype(np.float32) * np.float32(32767.0)), -32768, 32767).astype(np.int16)
        for u in range(70):
            n = int(full_len[u])
            assert np.array_equal(pcm[u, :n], want[u, :n]), u
    finally:
        _split(gpu_ctx, 0)
        gpu_ctx.set_option("arithmetic", 0)


# ---------------------------------------------------------------------------------------------
# Batch invariance of the tolerance mode, within a kernel family (src/lib.rs:594, :786-797: the
# chain is a pure function of (segments, voice, seed)).  A lane decides calm / general, its sub-tile length and
# its smoothness flavour from its own state only, so an utterance's samples do not depend on its wave-mates.

def _ragged_corpus(n_utt, first=0, n_voices=8):
    """Utterances whose events (segment ends, blend kinks, silent pairs) fall at different samples, so the lanes
    of a wave disagree about which tiles are calm.  Utterance u depends on u only."""
    segs, offs, vids, seeds = W.make_batch(n_utt, first_utt=first, n_voices=n_voices, length=0.05, blend_length=0.03125)
    u = (np.arange(n_utt, dtype=np.uint64) + first).repeat(W.SEGMENTS_PER_UTT)
    i = np.tile(np.arange(W.SEGMENTS_PER_UTT, dtype=np.uint64), n_utt)
    h = ((u * 2654435761 + i * 40503) % 1000).astype(np.float32) / 1000.0
    segs["length"] = (0.02 + 0.06 * h).astype(np.float32)
    segs["blend_length"] = np.where(h > 0.7, 0.0625, np.where(h > 0.4, 0.03125, 0.015625)).astype(np.float32)
    return segs, offs, vids, seeds


@pytest.mark.parametrize("lanes", [1, 2, 4, 8])
def test_fast_mode_is_batch_invariant_for_a_fixed_lane_mapping(gpu_ctx, lanes):
    voices = W.preset_voices(8)
    voices[3].phonemes[0].formant_smooth[2] *= 1.5        # one voice without a shared smoothness: the other flavour
    gpu_ctx.set_voices(voices)
    stride = 16384
    segs, offs, vids, seeds = _ragged_corpus(300)
    full, full_len = _render(gpu_ctx, True, segs, offs, vids, seeds, stride, lanes)
    assert "FAST" in gpu_ctx.last_kernel_name()
    ref, ref_len = O.synthesize_batch(_ovoices(voices), segs, offs, vids, seeds, stride)
    assert np.array_equal(full_len, ref_len)
    assert _worst(full, ref, ref_len) * ULP <= TOL
    for first, n in [(37, 1), (100, 33), (150, 64), (0, 7), (263, 37)]:
        s2, o2, v2, j2 = _ragged_corpus(n, first)
        part, part_len = _render(gpu_ctx, True, s2, o2, v2, j2, stride, lanes)
        assert np.array_equal(part_len, full_len[first:first + n])
        for r in range(n):
            m = int(part_len[r])
            assert np.array_equal(part[r, :m].view(np.uint32), full[first + r, :m].view(np.uint32)), (first, n, r)
    # a permutation of the batch: other wave-mates for everybody
    perm = np.random.default_rng(3).permutation(300)
    sp = np.concatenate([segs[offs[u]:offs[u + 1]] for u in perm])
    op = np.cumsum([0] + [int(offs[u + 1] - offs[u]) for u in perm]).astype(np.uint32)
    out, out_len = _render(gpu_ctx, True, sp, op, vids[perm], seeds[perm], stride, lanes)
    for r, u in enumerate(perm):
        m = int(full_len[u])
        assert out_len[r] == m
        assert np.array_equal(out[r, :m].view(np.uint32), full[u, :m].view(np.uint32)), (r, u)
    gpu_ctx.set_voices(W.single_voice())


def test_time_split_is_batch_invariant_for_a_fixed_grid(gpu_ctx):
    voices = W.preset_voices(8)
    gpu_ctx.set_voices(voices)
    stride = 16384
    segs, offs, vids, seeds = _ragged_corpus(200)
    try:
        _split(gpu_ctx, 3, 12800)
        full, full_len = _render(gpu_ctx, True, segs, offs, vids, seeds, stride)
        assert "SPLIT" in gpu_ctx.last_kernel_name()
        for first, n in [(37, 1), (100, 33), (120, 80)]:
            s2, o2, v2, j2 = _ragged_corpus(n, first)
            part, part_len = _render(gpu_ctx, True, s2, o2, v2, j2, stride)
            assert np.array_equal(part_len, full_len[first:first + n])
            for r in range(n):
                m = int(part_len[r])
                assert np.array_equal(part[r, :m].view(np.uint32), full[first + r, :m].view(np.uint32)), (first, n, r)
    finally:
        _split(gpu_ctx, 0)
        gpu_ctx.set_voices(W.single_voice())


def test_length_sorted_slot_assignment_is_invisible_in_fast_mode(gpu_ctx):
    """sort_by_length permutes wave-mates: the fast rows may not notice."""
    voices = W.single_voice()
    gpu_ctx.set_voices(voices)
    segs, offs, vids, seeds = _ragged_corpus(150, n_voices=1)
    stride = 16384
    try:
        rows = {}
        for sort in (1, 0):
            gpu_ctx.set_option("sort_by_length", sort)
            for lanes in (1, 2, 4, 8):
                rows[sort, lanes] = _render(gpu_ctx, True, segs, offs, vids, seeds, stride, lanes)
        for lanes in (1, 2, 4, 8):
            a, al = rows[1, lanes]
            b, bl = rows[0, lanes]
            assert np.array_equal(al, bl)
            for u in range(150):
                m = int(al[u])
                assert np.array_equal(a[u, :m].view(np.uint32), b[u, :m].view(np.uint32)), (lanes, u)
    finally:
        gpu_ctx.set_option("sort_by_length", 1)


def test_scan_kernel_flavours_and_batches_give_the_same_bits(gpu_ctx):
    """One workgroup per utterance: the scan kernel's samples cannot depend on the batch, and its three-stage and
    two-stage workgroups run the same arithmetic (the header promises "same results either way")."""
    voices = W.preset_voices(8)
    gpu_ctx.set_voices(voices)
    stride = 16384
    segs, offs, vids, seeds = _ragged_corpus(120)
    split_default = gpu_ctx.get_option("time_parallel_scan_split_max_utterances")
    try:
        gpu_ctx.set_option("time_split", 0)
        rows = {}
        for split in (1, 0):
            gpu_ctx.set_option("time_parallel_scan_split_max_utterances", split_default if split else 0)
            rows[split] = _render(gpu_ctx, True, segs, offs, vids, seeds, stride)
            assert gpu_ctx.last_kernel_name().startswith("scan_kernel") and ("SPLIT" in gpu_ctx.last_kernel_name()) == bool(split)
        assert np.array_equal(rows[0][1], rows[1][1])
        for u in range(120):
            m = int(rows[0][1][u])
            assert np.array_equal(rows[0][0][u, :m].view(np.uint32), rows[1][0][u, :m].view(np.uint32)), u
        s2, o2, v2, j2 = _ragged_corpus(17, 50)
        part, part_len = _render(gpu_ctx, True, s2, o2, v2, j2, stride)
        for r in range(17):
            m = int(part_len[r])
            assert m == rows[0][1][50 + r]
            assert np.array_equal(part[r, :m].view(np.uint32), rows[0][0][50 + r, :m].view(np.uint32)), r
    finally:
        gpu_ctx.set_option("time_parallel_scan_split_max_utterances", split_default)
        gpu_ctx.set_option("time_split", 1)
        gpu_ctx.set_voices(W.single_voice())


def test_host_output_blocks_share_one_kernel_family_in_fast_mode(gpu_ctx):
    """The host-output calls render in blocks of up to 4096 rows; the short last block takes the kernel family of
    the full ones (synthesize.cpp synthesize_rows, family_rows), so a row's fast-mode samples depend neither on its
    position nor on n_utt modulo the block size.  Utterance u depends on u only: rows 4100.. of one batch sit in
    its short last block, the same utterances sit inside the full first block of a batch that starts 150 later."""
    voices = W.preset_voices(8)
    gpu_ctx.set_voices(voices)
    stride = 16384
    n = 4096 + 150
    try:
        gpu_ctx.set_option("time_split_span_samples", 15360)     # the grid may not follow each batch's longest row
        a, a_len = _render(gpu_ctx, True, *_ragged_corpus(n), stride)
        family = gpu_ctx.last_kernel_name()
        b, b_len = _render(gpu_ctx, True, *_ragged_corpus(n, first=150), stride)
        assert gpu_ctx.last_kernel_name() == family
        assert np.array_equal(a_len[4100:n], b_len[3950:4096])
        for r in range(4100, n):
            m = int(a_len[r])
            assert m > 0
            assert np.array_equal(a[r, :m].view(np.uint32), b[r - 150, :m].view(np.uint32)), r
        # and against the oracle, the short block's rows
        ref, ref_len = O.synthesize_batch(_ovoices(voices), *_ragged_corpus(40, first=4200), stride)
        assert np.array_equal(a_len[4200:4240], ref_len)
        assert _worst(a[4200:4240], ref, ref_len) * ULP <= TOL
    finally:
        gpu_ctx.set_option("time_split_span_samples", 0)
        gpu_ctx.set_voices(W.single_voice())


def test_sharp_voices_get_the_reference_coefficients_or_the_exact_kernels(gpu_ctx):
    """grail_fast_sharpness above "fast_sharpness_limit": "arithmetic" = 1 is served by the second tier — the reference's
    own band-pass coefficients at every sample, fast arithmetic elsewhere — which stays far inside the tolerance where
    the interpolating tier does not; with "fast_exact_coefficients" = 0 by the exact kernels (the oracle's bits); with
    the limit lifted by the interpolating kernels (which deviate as predicted)."""
    v = G.voice_generic(48000.0)
    for p in range(2):
        for i in range(8):
            v.phonemes[p].formant_bw[i] /= 6.0           # 10 - 33 Hz: sharpness ~ 90
    assert G.fast_sharpness(v) > 2 * G.FAST_SHARPNESS_LIMIT
    gpu_ctx.set_voices([v])
    try:
        assert gpu_ctx.get_option("fast_arithmetic_served") == 2
        stride = 16384
        k_mid = 0.0
        for n, lanes in ((3, 1), (200, 1), (3000, 1), (200, 0)):
            segs, offs, vids, seeds = _ragged_corpus(n, n_voices=1)
            ref, ref_len = O.synthesize_batch(_ovoices([v]), segs, offs, vids, seeds, stride)
            out, out_len = _render(gpu_ctx, True, segs, offs, vids, seeds, stride, lanes)
            assert np.array_equal(out_len, ref_len)
            if lanes == 1:     # one lane per utterance pinned: the second tier's lane kernel
                assert "MID" in gpu_ctx.last_kernel_name() and gpu_ctx.get_option("last_launch_fast") == 2, gpu_ctx.last_kernel_name()
                k_mid = max(k_mid, _worst_rel(out, ref, ref_len))
            else:              # left to the library: a batch this small is rendered faster by the exact pipelined workgroups
                assert "PIPE" in gpu_ctx.last_kernel_name() and gpu_ctx.get_option("last_launch_fast") == 0
                assert np.array_equal(out.view(np.uint32), ref.view(np.uint32))
        # (oracle model of the tier over 3 000 random tables: at most 16; here a sharpness of ~195, and the kernel also
        # interpolates amplitudes and the low-pass factor: 22.5 measured)
        assert 0.0 < k_mid <= 32.0, k_mid
        segs, offs, vids, seeds = _ragged_corpus(200, n_voices=1)
        ref, ref_len = O.synthesize_batch(_ovoices([v]), segs, offs, vids, seeds, stride)
        # the second tier switched off: the exact kernels, the oracle's bits
        gpu_ctx.set_option("fast_exact_coefficients", 0)
        assert gpu_ctx.get_option("fast_arithmetic_served") == 0
        out, out_len = _render(gpu_ctx, True, segs, offs, vids, seeds, stride)
        assert "FAST" not in gpu_ctx.last_kernel_name() and gpu_ctx.get_option("last_launch_fast") == 0
        assert np.array_equal(out_len, ref_len) and np.array_equal(out.view(np.uint32), ref.view(np.uint32))
        gpu_ctx.set_option("fast_exact_coefficients", 1)
        # the limit lifted: the interpolating tier, off by about what the sharpness predicts
        gpu_ctx.set_option("fast_sharpness_limit", 1000)
        assert gpu_ctx.get_option("fast_arithmetic_served") == 1
        out, out_len = _render(gpu_ctx, True, segs, offs, vids, seeds, stride)
        assert "FAST" in gpu_ctx.last_kernel_name() and "MID" not in gpu_ctx.last_kernel_name()
        assert np.array_equal(out_len, ref_len)
        k = _worst(out, ref, ref_len) / max(1.0, float(np.abs(ref).max()))
        print(f"sharpness {G.fast_sharpness(v):.0f}: second tier {k_mid:.1f}, interpolating tier (limit lifted) {k:.1f} * 2^-23")
        assert k_mid < k <= 4.0 * G.fast_sharpness(v)
        # "arithmetic" = 2 asks for the second tier whatever the voices
        gpu_ctx.set_option("fast_sharpness_limit", int(G.FAST_SHARPNESS_LIMIT))
        gpu_ctx.set_voices(W.single_voice())
        gpu_ctx.set_option("arithmetic", 2)
        gpu_ctx.set_option("lanes_per_utterance", 1)
        segs, offs, vids, seeds = W.make_batch(64, length=0.125, blend_length=0.125)
        out, out_len = gpu_ctx.synthesize(segs, offs, vids, seeds, out_stride=W.max_samples(length=0.125))
        assert "MID" in gpu_ctx.last_kernel_name()
        ref, ref_len = O.synthesize_batch(_ovoices(W.single_voice()), segs, offs, vids, seeds, W.max_samples(length=0.125))
        assert np.array_equal(out_len, ref_len) and 0.0 < _worst_rel(out, ref, ref_len) <= 20.0
    finally:
        gpu_ctx.set_option("arithmetic", 0)
        gpu_ctx.set_option("lanes_per_utterance", 0)
        gpu_ctx.set_option("fast_exact_coefficients", 1)
        gpu_ctx.set_option("fast_sharpness_limit", int(G.FAST_SHARPNESS_LIMIT))
        gpu_ctx.set_voices(W.single_voice())


def test_fast_mode_batch_invariance_fuzz(gpu_ctx):
    """Batch invariance on random material: random served voice tables (one in three voices without a shared
    smoothness), random segment lists; the full batch against random sub-batches in random order, bit for bit,
    for each pinned kernel family — lane kernels L = 1, 2, 4, 8, the time-split kernels on a pinned grid, the
    scan kernel.  GRAIL_FAST_FUZZ_SEED / GRAIL_FAST_FUZZ_TRIALS as in the other fuzz tests."""
    rng = np.random.default_rng(int(os.environ.get("GRAIL_FAST_FUZZ_SEED", "424242")))
    stride = 65536
    families = [("lanes", 1), ("lanes", 2), ("lanes", 4), ("lanes", 8), ("split", 3), ("scan", 0)]
    try:
        for trial in range(int(os.environ.get("GRAIL_FAST_FUZZ_TRIALS", "2"))):
            voices = []
            for i in range(3):
                centre = np.exp(rng.uniform(np.log(150.0), np.log(8000.0), 8))
                rate = 44100.0 if (i == 1 and trial % 2) else 48000.0      # (odd trials: two sample rates in the table)
                v = G.voice_generic(rate)
                smooth = rng.uniform(200, 4000, 8) if i == 2 else np.full(8, rng.uniform(200, 4000))
                for p in range(2):
                    e = G.elem_new_phoneme(centre * rng.uniform(0.8, 1.25, 8), rng.uniform(60, 600, 8), smooth,
                                           rng.uniform(0, 1, 8), rng.uniform(0, 1, 8),
                                           rng.uniform(0.0, 1, 8) * (rng.uniform(0, 1, 8) > 0.3) + 1e-3)
                    v.phonemes[p] = G.elem_resample(e, 44100.0, rate)
                voices.append(W.tame_voice(v))
            gpu_ctx.set_voices(voices)
            assert gpu_ctx.get_option("fast_arithmetic_served") == 1
            n_utt = 96
            utts = []
            for u in range(n_utt):
                n = int(rng.integers(1, 5))
                utts.append([(int(rng.choice([G.PH_A, G.PH_E, G.PH_SILENCE])), float(rng.uniform(0.02, 0.3)),
                              float(rng.choice([0.0625, 0.125, 0.25, 0.5, 0.3, 0.07])),
                              float(rng.uniform(80, 400) / 48000.0)) for _ in range(n)])
            vids = rng.integers(0, 3, n_utt).astype(np.uint32)
            seeds = rng.integers(0, 2 ** 32, n_utt, dtype=np.uint64).astype(np.uint32)
            # ... and the rows are the oracle's within the tolerance (both rates, every family below)
            ref, ref_len = O.synthesize_batch(_ovoices(voices), G.segments([s for u in utts for s in u]),
                                              np.cumsum([0] + [len(u) for u in utts]).astype(np.uint32), vids, seeds, stride)

            def batch_of(idx):
                segs = G.segments([s for u in idx for s in utts[u]])
                offs = np.cumsum([0] + [len(utts[u]) for u in idx]).astype(np.uint32)
                return segs, offs, vids[idx].copy(), seeds[idx].copy()

            for kind, arg in families:
                gpu_ctx.set_option("time_split", 1 if kind == "split" else 0)
                gpu_ctx.set_option("time_parallel_scan", 1 if kind == "scan" else 0)
                _split(gpu_ctx, arg if kind == "split" else 0, 49152 if kind == "split" else 0)
                lanes = arg if kind == "lanes" else 0
                full, full_len = _render(gpu_ctx, True, *batch_of(np.arange(n_utt)), stride, lanes)
                name = gpu_ctx.last_kernel_name()
                if kind == "scan" and "scan" not in name:
                    continue                      # (the scan kernel's own window may reject a table)
                assert (name.startswith("synth_kernel") and "SPLIT" in name) == (kind == "split"), name
                assert ("scan" in name) == (kind == "scan"), name
                assert np.array_equal(full_len, ref_len), (trial, kind, arg)
                assert _worst_rel(full, ref, ref_len) * ULP <= TOL, (trial, kind, arg)
                for _ in range(3):
                    idx = rng.permutation(n_utt)[:int(rng.integers(1, 70))]
                    part, part_len = _render(gpu_ctx, True, *batch_of(idx), stride, lanes)
                    # (the instantiation may differ — a sub-batch without odd blend lengths takes the kernel without
                    # their division — the family may not)
                    sub = gpu_ctx.last_kernel_name()
                    assert (sub.startswith("synth_kernel") and "SPLIT" in sub) == (kind == "split"), (name, sub)
                    assert ("scan" in sub) == (kind == "scan") and "FAST" in sub, (name, sub)
                    assert np.array_equal(part_len, full_len[idx])
                    for r, u in enumerate(idx):
                        m = int(part_len[r])
                        assert np.array_equal(part[r, :m].view(np.uint32), full[u, :m].view(np.uint32)), \
                            (trial, kind, arg, r, u, name, sub)
    finally:
        gpu_ctx.set_option("time_split", 1)
        gpu_ctx.set_option("time_parallel_scan", 1)
        _split(gpu_ctx, 0)
        gpu_ctx.set_voices(W.single_voice())


@pytest.mark.parametrize("blend,seed", [(0.02, 79), (0.011, 80)])
def test_scan_kernel_clock_across_binade_boundaries(gpu_ctx, blend, seed):
    """The scan kernel's closed-form Sequencer clock (csrc/scan_kernels.hip, `extend`): a falling clock that lands
    exactly on a power of two has left the binade above it — the exact difference rounds on the finer grid below.
    Taking it for a member of the upper binade put the clock off by an ulp for the rest of the segment, one
    segment in a few hundred; alpha, the pitch of a blend and from there the carrier phase followed (a saw 6e-4
    off at its edges).  1 500 utterances of random segment lengths with short blends between distant pitches,
    fast (scan kernel) against exact rows on the device: 222 / 235 * 2^-23 before the fix, below 10 after."""
    rng = np.random.default_rng(seed)
    n_utt = 1500
    gpu_ctx.set_voices(W.single_voice())
    segs, offs, vids, seeds = W.make_batch(n_utt)
    k = len(segs)
    segs["length"] = rng.uniform(0.03, 0.3 if blend == 0.02 else 0.2, k).astype(np.float32)
    segs["blend_length"] = np.float32(blend)
    segs["frequency"] = (np.where(np.arange(k) % 2 == 0, 70.0, 400.0) / 48000.0).astype(np.float32)
    segs["phoneme"] = np.where(np.arange(k) % 4 == 0, G.PH_SILENCE, G.PH_A)
    stride = 4 * 14400 + 64
    b = gpu_ctx.upload(segs, offs, vids, seeds)
    d = [gpu_ctx.device_alloc(n_utt * stride * 4) for _ in range(2)]
    dl = [gpu_ctx.device_alloc(n_utt * 4) for _ in range(2)]
    try:
        gpu_ctx.set_option("time_split", 0)
        gpu_ctx.set_option("arithmetic", 0)
        b.synthesize_async(d[0], stride, dl[0])
        gpu_ctx.sync()
        gpu_ctx.set_option("arithmetic", 1)
        b.synthesize_async(d[1], stride, dl[1])
        gpu_ctx.sync()
        assert "scan" in gpu_ctx.last_kernel_name()
        md, sq, bad = gpu_ctx.compare(d[0], d[1], stride, dl[0], dl[1], n_utt)
        assert int(bad.sum()) == 0
        worst = float(md.max()) / ULP
        print(f"scan kernel, 1500 utterances with pitch jumps: worst |fast - exact| {worst:.1f} * 2^-23")
        assert worst <= 32.0
    finally:
        gpu_ctx.set_option("arithmetic", 0)
        gpu_ctx.set_option("time_split", 1)
        for x in d + dl:
            gpu_ctx.device_free(x)
        b.free()


def test_a_sharp_voice_takes_fast_arithmetic_only_from_the_batches_that_use_it(gpu_ctx):
    """the sharpness is judged over the voices a batch references, not over the whole table; what a launch
    actually ran is readable afterwards ("last_launch_fast")."""
    mild = G.voice_generic(48000.0)
    sharp = G.voice_generic(48000.0)
    for p in range(2):
        for i in range(8):
            sharp.phonemes[p].formant_bw[i] /= 6.0
    assert G.fast_sharpness(mild) <= G.FAST_SHARPNESS_LIMIT < G.fast_sharpness(sharp)
    gpu_ctx.set_voices([mild, sharp])
    assert gpu_ctx.get_option("fast_arithmetic_served") == 2          # the table as a whole: the second tier
    n_utt = 40
    segs, offs, _, seeds = W.make_batch(n_utt, length=0.125, blend_length=0.125)
    stride = W.max_samples(length=0.125)
    ov = _ovoices([mild, sharp])
    try:
        for vids, want_fast in ((np.zeros(n_utt, dtype=np.uint32), 1), (None, 1), (np.ones(n_utt, dtype=np.uint32), 2),
                                ((np.arange(n_utt) % 2).astype(np.uint32), 2)):
            # (one lane per utterance pinned: left to itself the library renders a batch this small of the sharp voice
            # with the exact kernels on a wider mapping — faster, and exact bits satisfy any tolerance)
            out, out_len = _render(gpu_ctx, True, segs, offs, vids, seeds, stride, lanes=1)
            assert gpu_ctx.get_option("last_launch_fast") == want_fast, vids
            ref, ref_len = O.synthesize_batch(ov, segs, offs, vids, seeds, stride)
            assert np.array_equal(out_len, ref_len)
            k = _worst_rel(out, ref, ref_len)
            assert 0.0 < k * ULP <= TOL
            out, out_len = _render(gpu_ctx, True, segs, offs, vids, seeds, stride)
            assert gpu_ctx.get_option("last_launch_fast") in ((1,) if want_fast == 1 else (0, 2))
            assert np.array_equal(out_len, ref_len) and _worst_rel(out, ref, ref_len) * ULP <= TOL
        gpu_ctx.set_option("fast_exact_coefficients", 0)              # without the second tier: the exact kernels
        out, out_len = _render(gpu_ctx, True, segs, offs, np.ones(n_utt, dtype=np.uint32), seeds, stride)
        assert gpu_ctx.get_option("last_launch_fast") == 0
        ref, ref_len = O.synthesize_batch(ov, segs, offs, np.ones(n_utt, dtype=np.uint32), seeds, stride)
        assert np.array_equal(out.view(np.uint32), ref.view(np.uint32))
    finally:
        gpu_ctx.set_option("fast_exact_coefficients", 1)
        gpu_ctx.set_voices(W.single_voice())


def test_one_pinned_family_makes_fast_mode_a_function_of_the_utterance_alone(gpu_ctx):
    """include/grail_hip.h, determinism contract: with "lanes_per_utterance" = 1 an utterance's fast-mode samples do
    not depend on the batch it is rendered in — a batch of 3, of 700 (scan / time-split territory when left to the
    library), a composite-sized one on a small machine, any position."""
    voices = W.preset_voices(8)
    gpu_ctx.set_voices(voices)
    stride = 16384
    segs, offs, vids, seeds = _ragged_corpus(1500)
    try:
        gpu_ctx.set_option("assume_compute_units", 4)            # 1 500 utterances > 1 024 lanes: several rounds
        big, big_len = _render(gpu_ctx, True, segs, offs, vids, seeds, stride, lanes=1)
        assert "FAST" in gpu_ctx.last_kernel_name() and gpu_ctx.get_option("last_launch_blocks") == 1
        gpu_ctx.set_option("assume_compute_units", 0)
        for first, n in ((0, 3), (100, 700), (1499, 1), (640, 64)):
            lo, hi = int(offs[first]), int(offs[first + n])
            sub_offs = (offs[first:first + n + 1] - offs[first]).astype(np.uint32)
            part, part_len = _render(gpu_ctx, True, segs[lo:hi], sub_offs, vids[first:first + n], seeds[first:first + n], stride, lanes=1)
            assert np.array_equal(part_len, big_len[first:first + n])
            for r in range(n):
                m = int(part_len[r])
                assert np.array_equal(part[r, :m].view(np.uint32), big[first + r, :m].view(np.uint32)), (first, r)
        # ... whereas left to itself the library renders the small batch with another family: same tolerance, other bits
        lo, hi = int(offs[100]), int(offs[800])
        auto, _ = _render(gpu_ctx, True, segs[lo:hi], (offs[100:801] - offs[100]).astype(np.uint32), vids[100:800], seeds[100:800], stride)
        assert "FAST" in gpu_ctx.last_kernel_name()
        assert not np.array_equal(auto[:, :2000].view(np.uint32), big[100:800, :2000].view(np.uint32))
    finally:
        gpu_ctx.set_option("assume_compute_units", 0)
        gpu_ctx.set_voices(W.single_voice())


def _custom_phoneme_set(rng, n, sharp):
    """n caller-built elems of a voice with more phonemes than the reference's two, the upper three formants silent.
    sharp: formants up to 0.08 fs with bandwidths of 60 - 200 Hz at 48 kHz (second tolerance tier); else formants below
    0.05 fs with bandwidths of 0.008 fs and more (first tier)."""
    elems = []
    for _ in range(n):
        e = np.zeros(49, dtype=np.float32)
        e[0] = 0.0025
        e[1:9] = np.sort(rng.uniform(0.005, 0.08 if sharp else 0.05, 8))
        e[9:17] = rng.uniform(0.00125, 0.004, 8) if sharp else rng.uniform(0.008, 0.02, 8)
        e[17:25] = rng.uniform(0.03, 0.12)
        e[25:33] = rng.uniform(0.0, 0.3, 8)
        e[33:41] = rng.uniform(0.0, 0.3, 8)
        amp = rng.uniform(0.2, 1.0, 8)
        amp[5:] = 0.0
        e[41:49] = amp / amp.sum()
        elems.append(e)
    return elems


@pytest.mark.parametrize("sharp", [False, True])
@pytest.mark.parametrize("n_utt", [90, 700, 5000])
def test_time_split_serves_caller_built_elems(gpu_ctx, n_utt, sharp):
    """grail_synthesize_batch_elems in fast mode, small and mid-size batches: the scan and time-split kernels take caller-built
    SequenceElems too — the warm-up length comes from the batch's own elems (computed at upload over the distinct ones)
    instead of a voice's phonemes.  Against the oracle on sampled utterances (utterances of half a second here; the
    bench corpus as elems: tools/elems_split_bench.py)."""
    rng = np.random.default_rng(500 + n_utt + int(sharp))
    v = G.voice_generic(48000.0)
    gpu_ctx.set_voices([v])
    ov = O.Voice.from_buffer_copy(bytes(v))
    phonemes = _custom_phoneme_set(rng, 6, sharp)
    gsegs, osegs, offs = [], [], [0]
    for u in range(n_utt):
        for i in range(4):
            has = i > 0 and bool(rng.integers(0, 6))
            e = phonemes[int(rng.integers(0, len(phonemes)))].copy()
            e[0] = np.float32(rng.uniform(90, 220)) / np.float32(48000.0)
            ln, bl = 0.125, float(rng.choice([0.125, 0.0625, 0.03]))
            gsegs.append(G.SequenceElem(int(has), G.SynthesisElem.from_np(e), ln, bl))
            osegs.append(O.SequenceElem(int(has), O.SynthesisElem.from_buffer_copy(e.tobytes()), ln, bl))
        offs.append(len(gsegs))
    seeds = rng.integers(0, 2 ** 32, n_utt, dtype=np.uint64).astype(np.uint32)
    stride = 24064
    gpu_ctx.set_option("arithmetic", 1)
    try:
        split_ms = lane_ms = 1e9
        for _ in range(3):                       # (kernel time: the best of three, the first launch runs on idle clocks)
            out, out_len = gpu_ctx.synthesize_elems(gsegs, offs, None, seeds, out_stride=stride)
            split_ms = min(split_ms, gpu_ctx.last_kernel_ms())
        name = gpu_ctx.last_kernel_name()
        chunks = gpu_ctx.get_option("last_launch_chunks")
        gpu_ctx.set_option("time_split", 0)
        for _ in range(3):
            lane, lane_len = gpu_ctx.synthesize_elems(gsegs, offs, None, seeds, out_stride=stride)
            lane_ms = min(lane_ms, gpu_ctx.last_kernel_ms())
        lane_name = gpu_ctx.last_kernel_name()
    finally:
        gpu_ctx.set_option("time_split", 1)
        gpu_ctx.set_option("arithmetic", 0)
    if n_utt <= 700 and not sharp:
        # few utterances of the first tier: the time-parallel scan kernel (it reads caller-built elems like phonemes)
        assert "scan_kernel" in name, name
    elif n_utt == 90:
        pass                                         # (sharp and few: second-tier time-split or an exact family, by cost)
    elif sharp:
        # second-tier time-split kernels, or the exact pipelined workgroups where those are cheaper (they take any blend length)
        assert ("SPLIT" in name and "MID" in name and chunks >= 2) or "PIPE" in name, (name, chunks)
    else:
        assert "SPLIT" in name and chunks >= 2 and "MID" not in name, (name, chunks)
    assert not ("synth_kernel" in lane_name and "SPLIT" in lane_name), lane_name
    assert np.array_equal(out_len, lane_len)
    worst = 0.0
    for u in rng.choice(n_utt, size=40, replace=False):
        ref = O.synthesize_sequence(ov, osegs[offs[u]:offs[u + 1]], int(seeds[u]))
        assert out_len[u] == len(ref), u
        peak = max(1.0, float(np.abs(ref).max()))
        worst = max(worst, float(np.abs(out[u, :len(ref)].astype(np.float64) - ref).max()) / peak)
        assert float(np.abs(lane[u, :len(ref)].astype(np.float64) - ref).max()) <= G.FAST_TOLERANCE * peak
    # (kernel times: tools/elems_split_bench.py — the one-call form renders in blocks of 4 096 rows, so the last
    # launch's time says little here)
    del split_ms, lane_ms
    print(f"caller-built elems ({'sharp' if sharp else 'tame'}), {n_utt} utterances: {name} x{chunks} (time_split = 0: {lane_name}); "
          f"worst |fast - oracle| = {worst * 2 ** 23:.1f} * 2^-23")
    assert worst <= G.FAST_TOLERANCE


@pytest.mark.parametrize("n_voices", [1, 8])
@pytest.mark.parametrize("family", ["L1", "L2", "L4", "L8", "split3", "split7", "scan", "mid", "mid split4"])
def test_every_fast_family_on_a_speech_like_corpus(gpu_ctx, family, n_voices):
    """Event-dense input — utterances of 8 - 32 phonemes with blends of any length, each lane with a segment boundary, the
    kink of alpha = min(time / blend_length, 1) and steep parameter ramps every few hundred samples at times of its own
    (workload.speech_like_batch, phonemes of 10 - 40 and of 4 - 16 ms) — through every kernel family of the tolerance
    mode against the oracle: the lengths are the reference's, every sample within GRAIL_FAST_TOLERANCE.  This is the
    input on which a lane's sub-tiles end at its own events and the wave takes slow samples (synth_kernel.h
    fast_render_tile); the aligned corpora of the tests above hardly ever get there."""
    voices = W.single_voice() if n_voices == 1 else W.preset_voices(8)
    gpu_ctx.set_voices(voices)
    worst = 0.0
    try:
        for scale, n_utt in ((0.25, 150), (0.1, 200)):
            segs, offs, vids, seeds, stride = W.speech_like_batch(n_utt, np.random.default_rng(int(scale * 100) + n_voices),
                                                                  n_voices=n_voices, scale=scale)
            ref, ref_len = O.synthesize_batch(_ovoices(voices), segs, offs, vids, seeds, stride)
            gpu_ctx.set_option("ragged_plan", 0)
            if family.startswith("mid"):
                gpu_ctx.set_option("arithmetic", 2)
            if "split" in family:
                _split(gpu_ctx, int(family.split("split")[1]))
                gpu_ctx.set_option("time_split_min_utterances", 0)
                gpu_ctx.set_option("time_parallel_scan", 0)
            elif family == "scan":
                gpu_ctx.set_option("time_split", 0)
                gpu_ctx.set_option("time_parallel_scan_max_utterances", 1 << 20)
            else:
                gpu_ctx.set_option("time_split", 0)
                gpu_ctx.set_option("time_parallel_scan", 0)
            lanes = int(family[1]) if family[0] == "L" else (1 if family == "mid" else 0)
            if family.startswith("mid"):
                gpu_ctx.set_option("lanes_per_utterance", lanes)
                out, out_len = gpu_ctx.synthesize(segs, offs, vids, seeds, out_stride=stride)
            else:
                out, out_len = _render(gpu_ctx, True, segs, offs, vids, seeds, stride, lanes)
            name = gpu_ctx.last_kernel_name()
            assert ("scan" in name) if family == "scan" else ("FAST" in name), name
            assert ("SPLIT" in name) == ("split" in family) or family == "scan", name
            assert ("MID" in name) == family.startswith("mid"), name
            assert np.array_equal(out_len, ref_len)
            k = _worst(out, ref, ref_len)
            worst = max(worst, k)
            assert 0.0 < k * ULP <= TOL, (family, scale, k)
            if family == "scan" and "SPLIT" in name:
                # ... and the two-stage flavour, which batches of a few thousand rows that differ in length get (eight live
                # formants: the only one)
                gpu_ctx.set_option("time_parallel_scan_split_max_utterances", 0)
                out, out_len = _render(gpu_ctx, True, segs, offs, vids, seeds, stride, 0)
                name = gpu_ctx.last_kernel_name()
                assert "scan" in name and "SPLIT" not in name, name
                assert np.array_equal(out_len, ref_len)
                k = _worst(out, ref, ref_len)
                worst = max(worst, k)
                assert 0.0 < k * ULP <= TOL, (family, scale, k, name)
    finally:
        for k_, v_ in (("arithmetic", 0), ("lanes_per_utterance", 0), ("ragged_plan", 1), ("time_split", 1), ("time_parallel_scan", 1),
                       ("time_split_min_utterances", -1), ("time_parallel_scan_max_utterances", -1),
                       ("time_parallel_scan_split_max_utterances", -1)):
            gpu_ctx.set_option(k_, v_)
        _split(gpu_ctx, 0)
    print(f"speech-like corpus, {family}, voices={n_voices}: max |d| = {worst:.1f} * 2^-23")


@pytest.mark.parametrize("n_voices,lanes", [(1, 2), (1, 4), (8, 4), (8, 8)])
def test_two_waves_per_simd_instantiations_give_the_same_bits(gpu_ctx, n_voices, lanes):
    """A tolerance-mode launch on 2 / 4 / 8 lanes per utterance with more wavefronts than the device has SIMDs takes the
    instantiations built for two wavefronts per SIMD (256 registers, no AGPR claim: csrc/family_cost.cpp family_cohabits;
    the device made small with "assume_compute_units").  Same source, same operations in the same order: the rows are
    bit-identical to the one-wave kernels' (option "two_waves_per_simd" = 0), and within the tolerance of the oracle."""
    voices = W.single_voice() if n_voices == 1 else W.preset_voices(8)
    gpu_ctx.set_voices(voices)
    n_utt = 700
    segs, offs, vids, seeds, stride = W.speech_like_batch(n_utt, np.random.default_rng(lanes), n_voices=n_voices, scale=0.1)
    ref, ref_len = O.synthesize_batch(_ovoices(voices), segs, offs, vids, seeds, stride)
    got = {}
    try:
        gpu_ctx.set_option("assume_compute_units", 2)          # 8 SIMDs: 700 utterances x L lanes are 22 ... 88 wavefronts
        gpu_ctx.set_option("ragged_plan", 0)
        gpu_ctx.set_option("time_split", 0)
        gpu_ctx.set_option("time_parallel_scan", 0)
        for two in (1, 0):
            gpu_ctx.set_option("two_waves_per_simd", two)
            out, out_len = _render(gpu_ctx, True, segs, offs, vids, seeds, stride, lanes)
            name = gpu_ctx.last_kernel_name()
            assert "FAST" in name and f"L={lanes}," in name and (",2," in name) == bool(two), name
            assert np.array_equal(out_len, ref_len)
            got[two] = out
    finally:
        for k_, v_ in (("assume_compute_units", 0), ("ragged_plan", 1), ("time_split", 1), ("time_parallel_scan", 1), ("two_waves_per_simd", 1)):
            gpu_ctx.set_option(k_, v_)
    for u in range(n_utt):
        assert np.array_equal(got[1][u, :ref_len[u]].view(np.uint32), got[0][u, :ref_len[u]].view(np.uint32)), u
    k = _worst(got[1], ref, ref_len)
    assert 0.0 < k * ULP <= TOL, k


@pytest.mark.parametrize("n_voices", [1, 8])
def test_time_split_lays_out_more_chunks_for_rows_that_differ_in_length(gpu_ctx, n_voices):
    """Speech-like rows on the time-split kernels: the upload keeps an upper bound of every utterance's length on the device,
    a chunk's lane whose utterance ends before the chunk begins renders nothing (no fast-forward, no warm-up) and a wave of
    such lanes is gone at once — so a batch whose grid would be coarse (a device made small here: 3 chunks) gets up to
    2 K - 1.  Same contract: lengths equal to the oracle's for every row, every sample within the tolerance; and the grid an
    aligned batch would get, pinned, likewise."""
    voices = W.single_voice() if n_voices == 1 else W.preset_voices(8)
    gpu_ctx.set_voices(voices)
    n = 1500
    segs, offs, vids, seeds, stride = W.speech_like_batch(n, np.random.default_rng(41), n_voices=n_voices, scale=0.25)
    try:
        gpu_ctx.set_option("assume_compute_units", 18)     # 72 SIMDs, 24 waves per chunk: 3 chunks
        gpu_ctx.set_option("time_parallel_scan", 0)
        gpu_ctx.set_option("ragged_plan", 0)               # (by its events the batch might go to a lane mapping)
        gpu_ctx.set_option("time_split_min_utterances", 0)
        out, out_len = _render(gpu_ctx, True, segs, offs, vids, seeds, stride)
        name, chunks = gpu_ctx.last_kernel_name(), gpu_ctx.get_option("last_launch_chunks")
        assert "SPLIT" in name and "FAST" in name, name
        assert 3 < chunks <= 5, chunks
        ref, ref_len = O.synthesize_batch(_ovoices(voices), segs, offs, vids, seeds, stride)
        assert np.array_equal(out_len, ref_len)
        k = _worst_rel(out, ref, ref_len)
        assert 0.0 < k <= TOL / ULP, k
        gpu_ctx.set_option("time_split_chunks", 3)
        pinned, pinned_len = _render(gpu_ctx, True, segs, offs, vids, seeds, stride)
        assert gpu_ctx.get_option("last_launch_chunks") == 3
        assert np.array_equal(pinned_len, ref_len) and _worst_rel(pinned, ref, ref_len) <= TOL / ULP
    finally:
        gpu_ctx.set_option("time_split_chunks", 0)
        gpu_ctx.set_option("time_split_min_utterances", -1)
        gpu_ctx.set_option("ragged_plan", 1)
        gpu_ctx.set_option("time_parallel_scan", 1)
        gpu_ctx.set_option("assume_compute_units", 0)
        gpu_ctx.set_voices(W.single_voice())
