"""Every compiled instantiation of the synthesis kernels launched under its whole name (tests/synth_ledger.py, readable
as tests/SYNTH_KERNELS.md): one case per ledger entry.  A case sets the entry's options, renders its corpus into buffers
with canary words around every row (tests/footprint.py), asserts that grail_last_kernel_name is the entry's name — the
whole string, before a sample is looked at — and holds the rows to the oracle: exact arithmetic bit for bit, tolerance
arithmetic within G.FAST_TOLERANCE x max(1, peak) (the header's contract), i16 rows as tests/test_store_footprint_gpu.py
holds them (the conversion of the oracle's rows) — after the f32 rows of the same batch and stride, bit for bit, so every
exact instantiation is held in f32.  One-shot cells launch at the corpus' own stride and at a capacity of
1021, which cuts inside a tile (the time-split kernels at the former only: a capacity that short gives no grid of two
chunks); stream cells pull 1, 63 and 65 samples, then 2000 per pull until the stream ends, and the chunks concatenate to the
oracle's rows.

Rows: two workgroups and three rows, so that the last workgroup is partly filled.  A lane kernel's workgroup holds
(64 / L) x WAVES rows (synth_launch_impl.h lane_grid); a pipelined workgroup 16 or 8 — when it is filled: a one-shot launch
of rows that differ in length is spread one utterance to a workgroup on a device this large (csrc/family_cost.cpp
pipe_fill_for), so the one-shot PIPE cells switch "pipeline_spread" off, and the case works the fill out from the options
and compute units the context reads back.  The kernels built for two waves per SIMD run only when a launch has more waves
than the device is assumed to have SIMDs (family_cohabits): those cells assume one compute unit and take 200 rows.  The
arithmetic of each is asserted in the case (_assert_rows)."""
import numpy as np
import pytest

import footprint as F
import grail_hip as G
import synth_ledger as SL
import test_store_footprint_gpu as SF
from grail_hip import workload as W

SIMDS_PER_CU = 4


def _assert_rows(ctx, e):
    """The row count does what the docstring says: by the launch code's rules, the name's L and WAVES and the context's options."""
    args = SL.synth_args(e.name)
    if args is None:
        assert e.rows == SL.SCAN_ROWS >= 2                    # scan_kernel: a workgroup per row
        return
    L, waves, minw, stream, pipe = args[0], args[2], args[3], args[4], args[8]
    if minw == 2:
        # family_cohabits: ceil(rows * L / 64) waves > the SIMDs of the device the context plans for
        assert ctx.get_option("two_waves_per_simd") == 1
        assert (e.rows * L + 63) // 64 > SIMDS_PER_CU * ctx.get_option("compute_units"), (e.rows, L)
        return
    if pipe:
        # what a workgroup of THIS launch holds, by the options and the compute units the context reads back
        # (family_cost.cpp pipe_fill_for, launch_pipe4 / launch_pipe8): every slot, 16 with four formants or 8
        per_block = SL.pipe_fill(e.rows, 64 // L, ctx.get_option("compute_units"), ctx.get_option("pipeline_spread"), True,
                                 bool(stream))
        assert per_block == {4: 16, 8: 8}[L], (e.name, per_block)
    else:
        per_block = (64 // L) * waves           # synth_launch_impl.h lane_grid; 64 lanes per chunk of a time-split grid
    assert -(-e.rows // per_block) == 2 and e.rows % per_block == 3 and e.rows == per_block + 3, (e.rows, per_block)


def _one_shot(ctx, e, c):
    voices, segs, offs, vids, seeds, ref, ref_len, S = c
    n_utt = len(ref_len)
    pcm16 = e.form == "i16"
    batch = ctx.upload(segs, offs, vids, seeds)
    try:
        for stride in e.launches:
            stride = S if stride == "S" else stride
            counts = np.minimum(ref_len, stride).astype(np.uint32)
            cut = bool(np.any(ref_len > stride))
            what = f"{e.corpus}[{n_utt}] {e.options} f32 stride {stride}"
            own, name = SF.launch_guarded(ctx, batch.synthesize_async, n_utt, stride, False, 0, counts, cut, {"name": e.name}, what)
            if pcm16:
                # the f32 rows bit for bit first, then the i16 rows of the same batch at the same stride
                assert e.arithmetic == "exact"
                F.check_bits(own, ref.view(np.uint32), counts, what)
                what = f"{e.corpus}[{n_utt}] {e.options} i16 stride {stride}"
                own, name = SF.launch_guarded(ctx, batch.synthesize_pcm16_async, n_utt, stride, True, 0, counts, cut,
                                              {"name": e.name}, what)
                F.check_bits(own, F.pcm16_of(ref).view(np.uint16), counts, what)
            elif e.arithmetic == "exact":
                F.check_bits(own, ref.view(np.uint32), counts, what)
            else:
                worst = F.check_tolerance(own, ref, counts, what)
                print(f"{what}: worst {worst / 2.0 ** -23:.1f} * 2^-23 of max(1, peak)")
    finally:
        batch.free()


def _pulls(e):
    for q in e.launches:
        yield q, 512
    while True:
        yield SL.REST, SL.REST + 1


def _batch_stream(ctx, e, c):
    voices, segs, offs, vids, seeds, ref, ref_len, S = c
    n_utt = len(ref_len)
    chunks = [[] for _ in range(n_utt)]
    batch = st = None
    try:
        batch = ctx.upload(segs, offs, vids, seeds)
        st = G.Stream(batch)
        for k, (q, stride) in enumerate(_pulls(e)):
            assert k < 100, "the stream never ended"
            what = f"stream of {e.corpus}[{n_utt}] {e.options}, pull {k}: quota {q} stride {stride}"
            rows, counts = SF.pull_guarded(ctx, st, q, stride, False, n_utt, {"name": e.name}, what)
            if counts.max(initial=0) == 0:
                break
            for u in range(n_utt):
                chunks[u].append((False, rows[u, :counts[u]].copy()))
    finally:
        if st is not None:
            st.close()
        if batch is not None:
            batch.free()
    worst = SF.check_concatenation(chunks, ref, ref_len, e.arithmetic == "exact", f"stream of {e.corpus} {e.options}")
    if e.arithmetic != "exact":
        print(f"stream of {e.corpus} {e.options}: worst {worst / 2.0 ** -23:.1f} * 2^-23 of max(1, peak)")


def _live_stream(ctx, e, c):
    """Segments appended two at a time between the pulls, as test_live_streams_store_only_their_chunks feeds them."""
    voices, segs, offs, vids, seeds, ref, ref_len, S = c
    n_utt = len(ref_len)
    st = G.LiveStream(ctx, n_utt, vids, seeds, ring_segments=8)
    chunks = [[] for _ in range(n_utt)]
    fed = offs[:-1].astype(np.int64).copy()
    finished = False
    try:
        for k, (q, stride) in enumerate(_pulls(e)):
            assert k < 100, "the live stream never ended"
            if not finished:
                upto = np.minimum(fed + 2, offs[1:].astype(np.int64))
                if np.any(upto > fed):
                    st.append(np.concatenate([segs[fed[u]:upto[u]] for u in range(n_utt)]),
                              np.concatenate([[0], np.cumsum(upto - fed)]).astype(np.uint32))
                    fed = upto
                else:
                    st.finish()
                    finished = True
            what = f"live stream of {e.corpus}[{n_utt}] {e.options}, pull {k}: quota {q} stride {stride}"
            rows, counts = SF.pull_guarded(ctx, st, q, stride, False, n_utt, {"name": e.name}, what)
            if finished and counts.max(initial=0) == 0:
                break
            for u in range(n_utt):
                chunks[u].append((False, rows[u, :counts[u]].copy()))
    finally:
        st.close()
    SF.check_concatenation(chunks, ref, ref_len, True, f"live stream of {e.corpus} {e.options}")


@pytest.mark.gpu
@pytest.mark.parametrize("e", [pytest.param(e, id=SL.cell_id(e)) for e in SL.ENTRIES])
def test_every_instantiation_runs_under_its_name_and_holds_to_the_oracle(gpu_ctx, e):
    ctx = gpu_ctx
    c = F.first_rows(SL.corpus(e.corpus), e.rows)
    assert len(c[6]) == e.rows
    saved = {k: ctx.get_option(k) for k in e.options}
    ctx.set_voices(c[0])
    try:
        for k, v in e.options.items():
            ctx.set_option(k, v)
        _assert_rows(ctx, e)
        {"f32": _one_shot, "i16": _one_shot, "batch-stream": _batch_stream, "live-stream": _live_stream}[e.form](ctx, e, c)
    finally:
        for k, v in saved.items():
            ctx.set_option(k, v)
        ctx.set_voices(W.single_voice())
