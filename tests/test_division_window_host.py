"""The case table of the division window (tests/division_window_cases.py), checked where no GPU is needed: the restated
gate puts every edge value on its side, and the oracle renders every case to finite, audible rows — so that the GPU
tests compare whole rows bit for bit, nothing masked, and the witness alone tells which body of the kernels ran."""
import numpy as np
import pytest

import division_window_cases as D
import grail_hip as G

f32 = np.float32


def _finite_and_audible(ref, ref_len, what, want_len):
    assert int(ref_len.min()) == int(ref_len.max()) == want_len, (what, int(ref_len.min()), int(ref_len.max()))
    for u in range(len(ref_len)):
        row = ref[u, :ref_len[u]]
        assert np.isfinite(row).all(), f"{what}: row {u} is not finite"
        assert float(np.abs(row).max()) > D.PEAK_FLOOR, f"{what}: row {u} peaks at {float(np.abs(row).max())}"


def test_the_edges_are_one_ulp_apart_and_on_their_sides():
    v = D.generic()
    jm = D.jitter_margin(v.jitter_delta_formant_frequency)
    jf = D.jitter_margin(v.jitter_delta_frequency)
    assert abs(float(jm) - 1.2525e-4) < 1e-8
    for margin, edges in ((jm, D.formant_edges(v.jitter_delta_formant_frequency)), (f32(0), D.formant_edges(0.0))):
        for name, e in edges.items():
            ok = D.bw_ok if name.startswith("bw") else (lambda f: D.freq_ok(f, margin))
            assert ok(e.inside) and not ok(e.outside), name
            assert abs(int(f32(e.inside).view(np.uint32)) - int(f32(e.outside).view(np.uint32))) == 1, name
    for name, e in D.pitch_edges(v.jitter_delta_frequency).items():
        assert D.pitch_ok(e.inside, jf) and not D.pitch_ok(e.outside, jf), name
    # the values the gate of csrc/division_window.h gives, pinned: a drift of the restatement shows here
    H = float.fromhex
    generic_jitter, no_jitter = D.formant_edges(v.jitter_delta_formant_frequency), D.formant_edges(0.0)
    pitch = D.pitch_edges(v.jitter_delta_frequency)
    assert float(generic_jitter["freq_lo"].inside) == H("0x1.08eee8p-13") and float(generic_jitter["freq_hi"].inside) == H("0x1.ff5cp-2")
    assert float(no_jitter["freq_lo"].inside) == H("0x1.00419ap-20") and float(no_jitter["freq_hi"].inside) == H("0x1.ff7ccep-2")
    assert float(pitch["pitch_lo"].inside) == H("0x1.08eee8p-13") and float(pitch["pitch_hi"].inside) == H("0x1.ff6ca8p-1")
    # the thresholds themselves are floats: the bandwidth edges are the constants
    e = D.formant_edges(0.0)
    assert e["bw_lo"].inside == f32(2.0 ** -39) and e["bw_hi"].inside == f32(512.0)
    assert e["freq_lo"].inside > f32(2.0 ** -20) and e["freq_hi"].inside < f32(0.5)


@pytest.mark.parametrize("name", [t.name for t in D.all_tables()])
def test_every_voice_table_is_on_its_side_finite_and_audible(name):
    t = D.table(name)
    assert len(t.voices) == len(D.FORMANTS)
    for v in t.voices:
        assert D.voice_admitted(v) == (t.side == "in"), name
        # ... and by phoneme A alone: E and silent() stay admitted
        a = v.phonemes[0]
        jm = D.jitter_margin(v.jitter_delta_formant_frequency)
        refused = [i for i in range(G.NUM_FORMANTS) if not (D.freq_ok(a.formant_freq[i], jm) and D.bw_ok(a.formant_bw[i]))]
        assert refused == ([] if t.side == "in" else [D.FORMANTS[t.voices.index(v)]]), (name, refused)
    r = D.rendered_table(t)
    assert D.changed_phoneme_is_entered_and_left(r), name
    _finite_and_audible(r.ref, r.ref_len, name, 5759)
    if t.sharp:
        r = D.rendered_table(D.silent_formant_only(t))
        assert D.changed_phoneme_is_entered_and_left(r), name
        _finite_and_audible(r.ref, r.ref_len, name + ", formant 7 alone", 5759)


@pytest.mark.parametrize("side", ["in", "out"])
def test_pitch_cases_are_on_their_sides_finite_and_audible(side):
    jf = D.jitter_margin(D.generic().jitter_delta_frequency)
    r = D.pitch_phoneme_case(side)
    pitches = np.asarray(r.segs["frequency"])
    assert all(D.pitch_ok(p, jf) for p in pitches[np.arange(len(pitches)) % D.SEGMENTS != 2])
    assert all(D.pitch_ok(p, jf) == (side == "in") for p in pitches[2::D.SEGMENTS])
    voiced = np.asarray(r.segs["phoneme"])[2::D.SEGMENTS] >= G.PH_A
    assert voiced.any() and not voiced.all()        # (a Silence segment's pitch is never looked at)
    _finite_and_audible(r.ref, r.ref_len, f"pitch {side}", 5759)
    e = D.pitch_elems_case(side)
    at = [s.elem.frequency for s in e.elems]
    assert all(D.pitch_ok(p, jf) == (side == "in" or i % 5 != 2) for i, p in enumerate(at))
    _finite_and_audible(e.ref, e.ref_len, f"pitch of elems {side}", 4799)


def test_blend_cases_take_the_step_the_table_says_and_are_finite_and_audible():
    cases = D.blend_cases()
    # (blend_div_ok asks for 2^-59 <= blend_length <= 2^59: 1.5 * 2^-59 is inside, 1.5 * 2^59 already beyond, like
    # 1.5 * 2^60 and 1.5 * 2^-61 — the bounds keep a factor of two to the proven window on either side)
    assert [(c.name, c.kind) for c in cases] == [
        ("2^-6", "pow2"), ("below 2^-6", "short"), ("above 2^-6", "short"), ("0.013", "short"),
        ("1.5*2^59", "general"), ("1.5*2^-59", "short"), ("1.5*2^60", "general"), ("1.5*2^-61", "general"),
        ("1.5*2^58", "short"), ("below 2^59", "short"), ("above 2^59", "general"),
        ("above 2^-59", "short"), ("below 2^-59", "general")]
    assert all(D.voice_admitted(v) for v in D.blend_table().voices)
    for c in cases:
        r = D.rendered_blend(c)
        assert D.changed_phoneme_is_entered_and_left(r)
        _finite_and_audible(r.ref, r.ref_len, f"blend length {c.name}", 5759)


@pytest.mark.parametrize("name", [c.name for c in D.host_gate_cases()])
def test_host_gate_cases_are_finite_and_audible(name):
    c = next(c for c in D.host_gate_cases() if c.name == name)
    r = D.rendered_host_gate(c)
    _finite_and_audible(r.ref, r.ref_len, name, 5759)
