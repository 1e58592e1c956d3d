"""The edges of the operand window of the short exact division (csrc/division_window.h; pair_is_safe, blend_div_ok and
clk_floor on the device, live4_elems_ok, scan_elems_ok and the planner's pitch tests on the host), as voice tables and
batches.  A plain helper module for tests/test_division_window_host.py and tests/test_division_window_gpu.py; it holds
no test and no fixture, and nothing here needs a GPU.

The gate is restated here in np.float32, one operation per rounding, and every edge value is found from the restatement
by bisection over the bit patterns: `inside` is the last value the gate admits, `outside` the float next to it.  The
GPU tests never assert these numbers themselves, only which body of the kernels ran for them (the read-only options
"slow_division_wave_steps" and "general_wave_steps").

Every case is voices::generic() at 48 kHz with one change to phoneme A, rendered over make_batch's A / E / Silence
draws: a lane enters and leaves the changed phoneme with its filter state alive.  Formant 2 is audible in generic(),
formant 7 silent."""
import collections

import numpy as np

import grail_hip as G
import oracle_lib as O
from grail_hip import workload as W

f32 = np.float32
RATE = 48000.0
SEGMENTS = 6
LENGTH = 0.02
BLEND = 2.0 ** -6
STRIDE = W.max_samples(segments=SEGMENTS, length=LENGTH)
FORMANTS = (1, 6)              # formant 2 (audible) and formant 7 (silent), as indices
PEAK_FLOOR = 0.05              # every row of every case is audible: there is something to compare

X_LO = f32(2.0 ** -20)
X_HI = f32(0.5) - X_LO
W_LO = f32(2.0 ** -39)
W_HI = f32(512.0)
PITCH_HI = f32(1.0)
BLEND_LO = f32(2.0 ** -59)
BLEND_HI = f32(2.0 ** 59)


# ---- the gate, restated ------------------------------------------------------
def jitter_margin(delta):
    """jm of a voice's jitter_delta_formant_frequency (jf of its jitter_delta_frequency)."""
    return f32(1.002) * np.abs(f32(delta))


def freq_low_ok(f, jm):
    return bool(f32(f32(f) * f32(0.999)) - f32(jm) >= X_LO)


def freq_high_ok(f, jm):
    return bool(f32(f32(f) * f32(1.001)) + f32(jm) <= X_HI)


def freq_ok(f, jm):
    return freq_low_ok(f, jm) and freq_high_ok(f, jm)


def bw_ok(w):
    return bool(f32(w) >= W_LO) and bool(f32(w) <= W_HI)


def pitch_low_ok(f, jf):
    return bool(f32(f32(f) * f32(0.999)) - f32(jf) >= X_LO)


def pitch_high_ok(f, jf):
    return bool(f32(f32(f) * f32(1.001)) + f32(jf) <= PITCH_HI)


def pitch_ok(f, jf):
    return pitch_low_ok(f, jf) and pitch_high_ok(f, jf)


def blend_div_ok(blend_length, length=LENGTH, sample_rate=RATE):
    b, n, d = f32(blend_length), f32(length), f32(1.0) / f32(sample_rate)
    return bool(b >= BLEND_LO) and bool(b <= BLEND_HI) and bool(n <= BLEND_HI) and bool(d >= BLEND_LO)


def is_pow2(x):
    bits = int(np.array(x, dtype=f32).view(np.uint32))
    return (bits & 0x7FFFFF) == 0 and 1 <= ((bits >> 23) & 0xFF) <= 253


def _bits(x):
    return int(np.array(x, dtype=f32).view(np.uint32))


def _float(bits):
    return np.array(bits, dtype=np.uint32).view(f32)[()]


Edge = collections.namedtuple("Edge", "inside outside")


def edge(admits, admitted, refused):
    """The last positive float `admits` admits on the way from `admitted` to `refused`, and the float next to it (the
    predicate is monotone in between: every operation of the gate is)."""
    a, r = _bits(admitted), _bits(refused)
    assert admits(_float(a)) and not admits(_float(r))
    while abs(a - r) > 1:
        m = (a + r) // 2
        if admits(_float(m)):
            a = m
        else:
            r = m
    inside, outside = _float(a), _float(r)
    assert np.nextafter(inside, outside) == outside
    return Edge(inside, outside)


def formant_edges(jitter_delta_formant_frequency):
    """{"freq_lo", "freq_hi", "bw_lo", "bw_hi"} -> Edge for a voice with this formant-frequency jitter."""
    jm = jitter_margin(jitter_delta_formant_frequency)
    return {"freq_lo": edge(lambda f: freq_low_ok(f, jm), 0.25, 2.0 ** -30),
            "freq_hi": edge(lambda f: freq_high_ok(f, jm), 0.25, 0.75),
            "bw_lo": edge(bw_ok, 1.0, 2.0 ** -60),
            "bw_hi": edge(bw_ok, 1.0, 2.0 ** 20)}


def pitch_edges(jitter_delta_frequency):
    jf = jitter_margin(jitter_delta_frequency)
    return {"pitch_lo": edge(lambda f: pitch_low_ok(f, jf), 0.25, 2.0 ** -30),
            "pitch_hi": edge(lambda f: pitch_high_ok(f, jf), 0.25, 1.5)}


# ---- voices -------------------------------------------------------------------
def generic():
    return G.voice_generic(RATE)


def ovoices(voices):
    return [O.Voice.from_buffer_copy(bytes(v)) for v in voices]


def changed_voice(formant, freq=None, bw=None, jitter_delta_formant_frequency=None):
    """generic() with phoneme A's formant `formant` moved."""
    v = generic()
    if jitter_delta_formant_frequency is not None:
        v.jitter_delta_formant_frequency = float(jitter_delta_formant_frequency)
    if freq is not None:
        v.phonemes[0].formant_freq[formant] = float(freq)
    if bw is not None:
        v.phonemes[0].formant_bw[formant] = float(bw)
    return v


def voice_admitted(v):
    """The restated gate over the whole table of a voice: every formant of every phoneme (silent()'s 0.25 / 0.25, which
    pairs with a Silence segment blend towards, is admitted under any jitter a voice here has)."""
    jm = jitter_margin(v.jitter_delta_formant_frequency)
    return all(freq_ok(p.formant_freq[i], jm) and bw_ok(p.formant_bw[i]) for p in v.phonemes for i in range(G.NUM_FORMANTS))


# a table: voices that sit on ONE side of ONE edge (side "in": every division of every pair may take the short path;
# "out": phoneme A may not).  sharp: the AUDIBLE formant-2 voice is too sharp for the interpolating tier of fast
# arithmetic (a bandwidth of 2^-39; a frequency next to 0.5 at generic()'s bandwidth: elems_sharpness grows with
# 1 / bw and with f^2), so a batch that names it never reaches the scan kernel; the silent formant-7 voice alone does.
Table = collections.namedtuple("Table", "name side voices sharp")
_cache = {}
_large = collections.OrderedDict()      # renderings of a hundred rows and more: the last few only
LARGE_ROWS, LARGE_KEPT = 100, 4


def gate_edge_tables():
    """The four thresholds of the formant gate under generic()'s own jitter, formants 2 and 7, either side."""
    if "gate" not in _cache:
        edges = formant_edges(generic().jitter_delta_formant_frequency)
        tables = []
        for name, e in edges.items():
            for side, value in (("in", e.inside), ("out", e.outside)):
                kw = {"freq" if name.startswith("freq") else "bw": value}
                tables.append(Table(f"{name}-{side}", side, [changed_voice(i, **kw) for i in FORMANTS], name in ("bw_lo", "freq_hi")))
        _cache["gate"] = tables
    return _cache["gate"]


def operand_tables():
    """The operand extremes the window still admits: no formant-frequency jitter, so the frequency edges sit at the
    window's own (den about 2^-19 at the low one), each with a bandwidth of 2^-39 and of 512 in the same formant
    (bw / freq about 2^29, 1 + g (g + k) about 2^40).  The side is the frequency's."""
    if "operand" not in _cache:
        edges = formant_edges(0.0)
        tables = []
        for fname in ("freq_lo", "freq_hi"):
            for bname, bw in (("bw_lo", W_LO), ("bw_hi", W_HI)):
                for side, value in (("in", edges[fname].inside), ("out", edges[fname].outside)):
                    voices = [changed_voice(i, freq=value, bw=bw, jitter_delta_formant_frequency=0.0) for i in FORMANTS]
                    tables.append(Table(f"{fname}+{bname}-{side}", side, voices, bname == "bw_lo"))
        _cache["operand"] = tables
    return _cache["operand"]


def all_tables():
    return gate_edge_tables() + operand_tables()


def table(name):
    return next(t for t in all_tables() if t.name == name)


def silent_formant_only(t):
    """The formant-7 voice of a table alone: nothing audible is moved, so fast arithmetic serves its interpolating tier."""
    return Table(t.name + "/formant7", t.side, [t.voices[FORMANTS.index(6)]], False)


# ---- batches and the oracle's rows of them -------------------------------------
Rendered = collections.namedtuple("Rendered", "voices segs offs vids seeds stride ref ref_len")


def batch(n_voices, n_utt=None, blend=BLEND, first_utt=0):
    """Three utterances per voice (or n_utt of them) of six segments of 20 ms: rows of 5 759 samples."""
    n = 3 * n_voices if n_utt is None else n_utt
    segs, offs, _, seeds = W.make_batch(n, first_utt=first_utt, n_voices=n_voices, segments=SEGMENTS, length=LENGTH,
                                        blend_length=blend)
    vids = (np.arange(n) % n_voices).astype(np.uint32)
    return segs, offs, vids, seeds


def render(key, voices, segs, offs, vids, seeds):
    """The oracle's rows, computed once per key and read-only afterwards.  Large renderings (the 130- and 300-row launches,
    each used by the one or two tests that follow each other) are kept only while they are the most recent few."""
    store = _large if len(vids) >= LARGE_ROWS else _cache
    if key not in store:
        ref, ref_len = O.synthesize_batch(ovoices(voices), segs, offs, vids, seeds, STRIDE)
        for a in (segs, offs, vids, seeds, ref, ref_len):
            a.setflags(write=False)
        store[key] = Rendered(voices, segs, offs, vids, seeds, STRIDE, ref, ref_len)
        while len(_large) > LARGE_KEPT:
            _large.popitem(last=False)
    return store[key]


def rendered_table(t, n_utt=None, blend=BLEND):
    return render(("table", t.name, n_utt, float(f32(blend))), t.voices, *batch(len(t.voices), n_utt, blend))


def mixed_tables(tables):
    """One table of the voices of several (same side): launches that need more rows than one edge's two voices give."""
    assert len({t.side for t in tables}) == 1
    return Table("+".join(t.name for t in tables), tables[0].side, [v for t in tables for v in t.voices],
                 any(t.sharp for t in tables))


def changed_phoneme_is_entered_and_left(r):
    """Does every voice of a rendered batch have an utterance with an A segment next to one that is not A?"""
    ph = np.asarray(r.segs["phoneme"]).reshape(len(r.vids), -1)
    ok = set()
    for u in range(len(r.vids)):
        a = ph[u] == G.PH_A
        if np.any(a[1:] != a[:-1]):
            ok.add(int(r.vids[u]))
    return ok == set(range(len(r.voices)))


def batch_with_voiced_row(n_utt, row):
    """batch(1, n_utt) from the first stretch of the corpus in which utterance `row` enters and leaves phoneme A."""
    for first in range(64):
        segs, offs, vids, seeds = batch(1, n_utt, first_utt=first)
        a = np.asarray(segs["phoneme"]).reshape(n_utt, -1)[row] == G.PH_A
        if np.any(a[1:] != a[:-1]):
            return segs, offs, vids, seeds
    raise AssertionError("no such stretch")


# ---- pitch ----------------------------------------------------------------------
def pitch_phoneme_case(side, n_utt=12):
    """Phoneme mode: segment 2 of every utterance at the lowest pitch the gate admits under generic()'s pitch jitter (in)
    or the float below it (out).  (A phoneme batch's pitch is capped at 0.5: the upper bound belongs to elems.)"""
    e = pitch_edges(generic().jitter_delta_frequency)["pitch_lo"]
    segs, offs, vids, seeds = batch(1, n_utt)
    segs["frequency"][2::SEGMENTS] = e.inside if side == "in" else e.outside
    return render(("pitch", side, n_utt), [generic()], segs, offs, vids, seeds)


PitchElems = collections.namedtuple("PitchElems", "voices elems offs vids seeds stride ref ref_len")


def pitch_elems_case(side, n_utt=6):
    """Caller-built elems (grail_synthesize_batch_elems takes any pitch): sequences of five elems, A and E in turn, 20 ms
    each; the third has the highest pitch the gate admits (in) or the float above it (out).  Rows of 4 799 samples."""
    key = ("pitch_elems", side, n_utt)
    if key not in _cache:
        e = pitch_edges(generic().jitter_delta_frequency)["pitch_hi"]
        v = generic()
        elems = []
        for u in range(n_utt):
            for i in range(5):
                s = G.SequenceElem()
                s.has_elem = 1
                s.elem = v.phonemes[i % 2]
                s.elem.frequency = float(e.inside if side == "in" else e.outside) if i == 2 else 0.003
                s.length, s.blend_length = LENGTH, BLEND
                elems.append(s)
        offs = (np.arange(n_utt + 1) * 5).astype(np.uint32)
        ov = ovoices([v])[0]
        ref, ref_len = np.zeros((n_utt, STRIDE), dtype=f32), np.zeros(n_utt, dtype=np.uint32)
        for u in range(n_utt):
            row = O.synthesize_sequence(ov, [O.SequenceElem.from_buffer_copy(bytes(s)) for s in elems[5 * u:5 * u + 5]], u)
            ref[u, :len(row)], ref_len[u] = row, len(row)
        ref.setflags(write=False)
        ref_len.setflags(write=False)
        _cache[key] = PitchElems([v], elems, offs, np.zeros(n_utt, dtype=np.uint32), np.arange(n_utt, dtype=np.uint32), STRIDE,
                                 ref, ref_len)
    return _cache[key]


# ---- blend lengths -----------------------------------------------------------------
# kind: "pow2" multiplies by 2^k (the control: no division); "short" divides the clock by the short exact division;
# "general": blend_div_ok fails, every step of the pair is a general step (IEEE division)
BlendCase = collections.namedtuple("BlendCase", "name blend kind")


def blend_cases():
    cases = [("2^-6", f32(BLEND)), ("below 2^-6", np.nextafter(f32(BLEND), f32(0))), ("above 2^-6", np.nextafter(f32(BLEND), f32(1))),
             ("0.013", f32(0.013)), ("1.5*2^59", f32(1.5 * 2.0 ** 59)), ("1.5*2^-59", f32(1.5 * 2.0 ** -59)),
             ("1.5*2^60", f32(1.5 * 2.0 ** 60)), ("1.5*2^-61", f32(1.5 * 2.0 ** -61)),
             # the admitted side of the upper bound (2^59 itself multiplies): quotients near 2^-65
             ("1.5*2^58", f32(1.5 * 2.0 ** 58)), ("below 2^59", np.nextafter(f32(2.0 ** 59), f32(0))),
             ("above 2^59", np.nextafter(f32(2.0 ** 59), f32(np.inf))),
             # ... and of the lower one
             ("above 2^-59", np.nextafter(f32(2.0 ** -59), f32(1))), ("below 2^-59", np.nextafter(f32(2.0 ** -59), f32(0)))]
    return [BlendCase(n, b, "pow2" if is_pow2(b) else "short" if blend_div_ok(b) else "general") for n, b in cases]


def blend_table():
    """The voices the blend lengths are rendered with: every admitted operand extreme (all pairs inside the window, so
    the blend length alone decides which step a pair takes)."""
    return mixed_tables([t for t in operand_tables() if t.side == "in"])


def rendered_blend(case, n_utt=None):
    return rendered_table(blend_table(), n_utt, case.blend)


# ---- the host's gate of the four-formant kernels (live4_ok) ---------------------------
HostGateCase = collections.namedtuple("HostGateCase", "name side voice")


def host_gate_cases():
    """generic() with formants 5-8 of EVERY phoneme at a threshold of live4_ok: the four formant edges, and
    jitter_delta_amplitude 0.5, breath, turbulence and smoothness 1.0 with the float beyond each."""
    if "host_gate" not in _cache:
        cases = []
        upper = range(G.NUM_FORMANTS // 2, G.NUM_FORMANTS)

        def with_upper(field, value):
            v = generic()
            for p in range(G.NUM_VOICED):
                for i in upper:
                    getattr(v.phonemes[p], field)[i] = float(value)
            return v
        for name, e in formant_edges(generic().jitter_delta_formant_frequency).items():
            field = "formant_freq" if name.startswith("freq") else "formant_bw"
            cases += [HostGateCase(f"{name}-in", "in", with_upper(field, e.inside)),
                      HostGateCase(f"{name}-out", "out", with_upper(field, e.outside))]
        for field in ("formant_breath", "formant_turb", "formant_smooth"):
            cases += [HostGateCase(f"{field}-in", "in", with_upper(field, 1.0)),
                      HostGateCase(f"{field}-out", "out", with_upper(field, np.nextafter(f32(1), f32(2))))]
        for side, value in (("in", f32(0.5)), ("out", np.nextafter(f32(0.5), f32(1)))):
            v = generic()
            v.jitter_delta_amplitude = float(value)
            cases.append(HostGateCase(f"jitter_delta_amplitude-{side}", side, v))
        _cache["host_gate"] = cases
    return _cache["host_gate"]


def rendered_host_gate(case, n_utt=24):
    return render(("host_gate", case.name, n_utt), [case.voice], *batch(1, n_utt))


# ---- comparisons ----------------------------------------------------------------------
def assert_bits(out, out_len, ref, ref_len, what):
    """Rows and lengths equal the oracle's bit for bit (the rows are finite: nothing to mask)."""
    assert np.array_equal(np.asarray(out_len), ref_len), f"{what}: lengths {np.asarray(out_len)[:8]} against {ref_len[:8]}"
    for u in range(len(ref_len)):
        n = int(ref_len[u])
        a, b = np.asarray(out[u][:n]).view(np.uint32), ref[u, :n].view(np.uint32)
        if not np.array_equal(a, b):
            i = int(np.argmax(a != b))
            raise AssertionError(f"{what}: row {u} first differs at sample {i} of {n}: {a[i]:#x} against {b[i]:#x} "
                                 f"({int((a != b).sum())} samples differ)")


def worst_deviation(out, out_len, ref, ref_len, what):
    """max over rows of |out - ref| / max(1, peak(ref)); lengths must be equal and every sample finite."""
    assert np.array_equal(np.asarray(out_len), ref_len), f"{what}: lengths {np.asarray(out_len)[:8]} against {ref_len[:8]}"
    worst = 0.0
    for u in range(len(ref_len)):
        n = int(ref_len[u])
        x, r = np.asarray(out[u][:n]).astype(np.float64), ref[u, :n].astype(np.float64)
        assert np.isfinite(x).all(), f"{what}: row {u} holds a non-finite sample"
        worst = max(worst, float(np.abs(x - r).max(initial=0.0)) / max(1.0, float(np.abs(r).max(initial=0.0))))
    return worst
