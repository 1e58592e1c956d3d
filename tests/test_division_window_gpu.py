"""Parity at the edges of the division window, with the slow-path counters as witness (tests/division_window_cases.py
holds the cases, tests/test_division_window_host.py checks them without a GPU).

Inside an operand window the exact kernels replace IEEE division by v_rcp_f32 plus Newton and remainder steps; a gate
(pair_is_safe, blend_div_ok, clk_floor on the device, live4_ok / scan_voice_ok / the planner's pitch tests on the host)
decides per segment pair which body a lane takes.  Here every threshold of the gate is visited from both sides, one
float apart: the rows equal the oracle's bit for bit on either side (they are finite and audible: nothing is masked),
and the read-only options "slow_division_wave_steps" / "general_wave_steps" say which body ran — a gate that admits
too much, refuses everything or differs between host and device by one float fails here."""
import numpy as np
import pytest

import division_window_cases as D
import grail_hip as G
from grail_hip import workload as W
from test_stream_gpu import stream_all

pytestmark = pytest.mark.gpu
f32 = np.float32

# (name, lanes_per_utterance, n_utt): every lane mapping with three utterances per voice, and the default plan for 17
# and 300 utterances (the pipelined workgroups)
FAMILIES = [("L1", 1, None), ("L2", 2, None), ("L4", 4, None), ("L8", 8, None), ("plan17", 0, 17), ("plan300", 0, 300)]


@pytest.fixture
def ctx(gpu_ctx):
    """The suite's one context (session-scoped), handed back with voices::generic() as its table."""
    yield gpu_ctx
    gpu_ctx.set_voices(W.single_voice())


def witness(ctx):
    return np.array([ctx.get_option("slow_division_wave_steps"), ctx.get_option("general_wave_steps")], dtype=np.int64)


def one_shot(ctx, r, lanes=0, arithmetic=0):
    """(out, out_len, slow steps, general steps, kernel name) of one launch of a rendered case's batch."""
    ctx.set_voices(r.voices)
    ctx.set_option("lanes_per_utterance", lanes)
    ctx.set_option("arithmetic", arithmetic)
    try:
        before = witness(ctx)
        out, out_len = ctx.synthesize(r.segs, r.offs, r.vids, r.seeds, out_stride=r.stride)
        slow, general = witness(ctx) - before
        name = ctx.last_kernel_name()
    finally:
        ctx.set_option("lanes_per_utterance", 0)
        ctx.set_option("arithmetic", 0)
    return out, out_len, int(slow), int(general), name


def assert_side(side, slow, what):
    if side == "in":
        assert slow == 0, f"{what}: {slow} wave-steps took the IEEE body with every pair inside the window"
    else:
        assert slow > 0, f"{what}: no wave-step took the IEEE body with phoneme A outside the window"


@pytest.mark.parametrize("name", [t.name for t in D.all_tables()])
def test_every_family_is_bit_exact_on_its_side_of_the_gate(ctx, name):
    t = D.table(name)
    for family, lanes, n_utt in FAMILIES:
        r = D.rendered_table(t, n_utt)
        out, out_len, slow, _, kernel = one_shot(ctx, r, lanes)
        what = f"{name} {family} {kernel}"
        print(f"{what}: slow {slow}")
        if lanes == 0:          # (either side: four-formant workgroups inside, eight formants laid out beyond)
            assert ctx.get_option("last_launch_pipelined") == 1, what
        D.assert_bits(out, out_len, r.ref, r.ref_len, what)
        assert_side(t.side, slow, what)


def _live_rows(ctx, r, chunk):
    n = len(r.vids)
    st = G.LiveStream(ctx, n, r.vids, r.seeds, ring_segments=8)
    d_out, d_len = ctx.device_alloc(n * chunk * 4), ctx.device_alloc(n * 4)
    rows = [[] for _ in range(n)]
    try:
        st.append(r.segs, r.offs)
        st.finish()
        for _ in range(64):
            st.next_async(chunk, d_out, chunk, d_len)
            ctx.sync()
            lens = np.zeros(n, dtype=np.uint32)
            ctx.d2h(lens, d_len, n * 4)
            if lens.max(initial=0) == 0:
                break
            buf = np.zeros((n, chunk), dtype=np.float32)
            ctx.d2h(buf, d_out, buf.nbytes)
            for u in range(n):
                rows[u].append(buf[u, :lens[u]].copy())
        else:
            raise AssertionError("the live stream never ended")
    finally:
        st.close()
        ctx.device_free(d_out)
        ctx.device_free(d_len)
    return [np.concatenate(x) if x else np.zeros(0, dtype=np.float32) for x in rows]


@pytest.mark.parametrize("name", [t.name for t in D.all_tables()])
def test_streams_carry_the_gate_across_their_saved_state(ctx, name):
    """Chunks of 1 000 samples: a pair's verdict (pair_safe) is saved and loaded with the lane's filter state, in the
    middle of pairs on either side of the gate — as a stream of an uploaded batch and as a live stream."""
    t = D.table(name)
    r = D.rendered_table(t)
    ctx.set_voices(r.voices)
    for kind in ("batch", "live"):
        before = witness(ctx)
        if kind == "batch":
            b = ctx.upload(r.segs, r.offs, r.vids, r.seeds)
            try:
                rows = stream_all(ctx, b, len(r.vids), [1000], stride=1024)
            finally:
                b.free()
        else:
            rows = _live_rows(ctx, r, 1000)
        slow = int((witness(ctx) - before)[0])
        what = f"{name} {kind} stream {ctx.last_kernel_name()}"
        print(f"{what}: slow {slow}")
        D.assert_bits(rows, [len(x) for x in rows], r.ref, r.ref_len, what)
        assert_side(t.side, slow, what)


@pytest.mark.parametrize("side", ["in", "out"])
def test_pitch_at_the_gate(ctx, side):
    """The lowest admitted pitch in a phoneme batch (every lane mapping and the default plan), the highest in caller-built
    elems, and the floats beyond them."""
    r = D.pitch_phoneme_case(side)
    for lanes in (0, 1, 2, 4, 8):
        out, out_len, slow, _, kernel = one_shot(ctx, r, lanes)
        D.assert_bits(out, out_len, r.ref, r.ref_len, f"pitch {side} L={lanes} {kernel}")
        assert_side(side, slow, f"pitch {side} L={lanes} {kernel}")
    e = D.pitch_elems_case(side)
    ctx.set_voices(e.voices)
    for lanes in (0, 1, 8):
        ctx.set_option("lanes_per_utterance", lanes)
        try:
            before = witness(ctx)
            out, out_len = ctx.synthesize_elems(e.elems, e.offs, e.vids, e.seeds, out_stride=e.stride)
            slow = int((witness(ctx) - before)[0])
        finally:
            ctx.set_option("lanes_per_utterance", 0)
        what = f"pitch of elems {side} L={lanes} {ctx.last_kernel_name()}"
        D.assert_bits(out, out_len, e.ref, e.ref_len, what)
        assert_side(side, slow, what)


@pytest.mark.parametrize("family,lanes,n_utt", FAMILIES)
def test_blend_lengths_at_the_edges_of_the_short_division(ctx, family, lanes, n_utt):
    """clk / blend_length: 2^-6 multiplies (the control), its neighbours, 0.013 and 1.5 * 2^-59 take the short division,
    as do the last floats inside blend_div_ok's bounds (2^-59 <= blend_length <= 2^59: 1.5 * 2^58 and the float below
    2^59, quotients near 2^-65; the float above 2^-59); the first floats beyond them, 1.5 * 2^59, 1.5 * 2^60 and
    1.5 * 2^-61 fail blend_div_ok and send every step of every pair through the general step.  All pairs
    are inside the window (no wave-step may count as slow); "general_wave_steps" is the witness: a launch whose every
    step is a general step counts at least the samples of its longest row, and more than any launch of the same rows
    that takes the short division (which still sends a few steps there: segment starts, jitter wraps, and — not a power
    of two — a clock below 2^-59)."""
    general = {}
    for c in D.blend_cases():
        r = D.rendered_blend(c, n_utt)
        out, out_len, slow, general[c.name], kernel = one_shot(ctx, r, lanes)
        what = f"blend length {c.name} {family} {kernel}"
        print(f"{what}: general {general[c.name]} slow {slow}")
        D.assert_bits(out, out_len, r.ref, r.ref_len, what)
        assert slow == 0, what
        if c.kind == "general":
            assert general[c.name] >= int(r.ref_len.max()), what
    for c in D.blend_cases():
        if c.kind == "general":
            assert all(general[c.name] > general[o.name] for o in D.blend_cases() if o.kind != "general"), general
        else:
            assert general[c.name] > 0, (c.name, general)


EDGES = sorted({t.name.rsplit("-", 1)[0] for t in D.all_tables()})


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("formant", [0, 1])
@pytest.mark.parametrize("edge", EDGES)
def test_one_refused_lane_in_a_wave_of_admitted_ones(ctx, edge, formant, lanes):
    """130 utterances of admitted voices but for utterance 37, whose voice is one float outside: every row bit-exact, the
    counter sees the one lane, and the 129 others are the rows they are without it."""
    t_in, t_out = D.table(f"{edge}-in"), D.table(f"{edge}-out")
    voices = t_in.voices + [t_out.voices[formant]]
    n, odd = 130, 37
    segs, offs, _, seeds = D.batch_with_voiced_row(n, odd)                        # the odd one does use its phoneme A
    vids = (np.arange(n) % 2).astype(np.uint32)
    calm = D.render(("calm", edge, n), t_in.voices, segs, offs, vids, seeds)
    vids = vids.copy()
    vids[odd] = 2
    r = D.render(("odd", edge, formant, n), voices, segs.copy(), offs.copy(), vids, seeds.copy())
    out, out_len, slow, _, kernel = one_shot(ctx, r, lanes)
    what = f"{edge} formant {D.FORMANTS[formant] + 1} L={lanes} {kernel}"
    D.assert_bits(out, out_len, r.ref, r.ref_len, what)
    assert slow > 0, f"{what}: the refused lane does not show in the counter"
    out0, out_len0, slow0, _, _ = one_shot(ctx, calm, lanes)
    assert slow0 == 0, what
    D.assert_bits(out0, out_len0, calm.ref, calm.ref_len, what + " without the odd one")
    others = np.arange(n) != odd
    assert np.array_equal(out_len[others], out_len0[others])
    assert np.array_equal(out[others].view(np.uint32), out0[others].view(np.uint32)), what


@pytest.mark.parametrize("lanes", [1, 2, 4])
def test_the_host_gate_of_the_four_formant_kernels_at_its_thresholds(ctx, lanes):
    """live4_ok: formants 5-8 of every phoneme at each threshold keep the four-formant kernels, one float beyond they are
    laid out — and the rows are the oracle's either way."""
    ctx.set_option("row_groups", 0)
    try:
        for c in D.host_gate_cases():
            r = D.rendered_host_gate(c)
            out, out_len, _, _, kernel = one_shot(ctx, r, lanes)
            what = f"{c.name} L={lanes} {kernel}"
            assert ctx.get_option("last_launch_formants") == (4 if c.side == "in" else 8), what
            D.assert_bits(out, out_len, r.ref, r.ref_len, what)
    finally:
        ctx.set_option("row_groups", 1)


@pytest.mark.parametrize("edge", EDGES)
def test_fast_arithmetic_at_the_gate(ctx, edge):
    """arithmetic = 1 on the fast lane kernels and on a batch small enough for the scan kernel, which has no IEEE body:
    the host's gate is its only protection.  Admitted voices stay within the tolerance; refused ones too, are kept off
    the scan kernel and take more general steps.  A bandwidth of 2^-39 is too sharp for the interpolating tier: the host
    says so and serves another one (the bound holds there as well), as it does for an audible formant next to 0.5 at
    generic()'s bandwidth; of those tables the silent formant-7 voice alone is rendered too, which is served the
    interpolating tier and reaches the scan kernel at that edge."""
    t_in, t_out = D.table(f"{edge}-in"), D.table(f"{edge}-out")
    pairs = [(t_in, t_out)]
    if t_in.sharp:      # the silent formant-7 voice alone is served the interpolating tier: this edge's way to the scan kernel
        pairs.append((D.silent_formant_only(t_in), D.silent_formant_only(t_out)))
    for t_in, t_out in pairs:
        for lanes in (0, 1):
            general = {}
            for t in (t_in, t_out):
                r = D.rendered_table(t)
                ctx.set_voices(r.voices)
                served = ctx.get_option("fast_arithmetic_served")
                assert (served != 1) if t.sharp else (served == 1), (t.name, served)
                out, out_len, _, general[t.side], kernel = one_shot(ctx, r, lanes, arithmetic=1)
                what = f"{t.name} fast L={lanes} tier {served} {kernel}"
                worst = D.worst_deviation(out, out_len, r.ref, r.ref_len, what)
                print(f"{what}: {worst / 2.0 ** -23:.1f} * 2^-23, general {general[t.side]}")
                assert worst <= G.FAST_TOLERANCE, what
                if t.side == "out":
                    assert "scan_kernel" not in kernel, what
                elif lanes == 0 and not t.sharp:
                    assert "scan_kernel" in kernel, what
            assert general["out"] > general["in"], (t_in.name, lanes, general)
